"""The lexical casts on the MI355X: RDFGPU_EX_CAST_STRING (xsd:string of a term's lexical form, a view) and RDFGPU_EX_CAST_LEX (the
numeric casts that parse a simple literal), in FilterExec, join filters, the input of SUM / AVG and computed columns.  The oracle does
not restate them: the expectation is lex_cases.py (recognisers, exact conversion through fractions.Fraction, and which rows
Eisel-Lemire as specified may decline).  Values are compared bit for bit."""
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi
from rdf_fusion_amd.engine import RdfGpuError, TV_DTYPE
from rdf_fusion_amd import plan as P
from rdf_fusion_amd.plan import PlanBuilder, col, ENC_TV, EBV
from test_gpu_parity import table_on_device
from test_aggregate_cpu import sum_agg, avg_agg, same
import lex_cases as L

TAGS = {"boolean": abi.TV_BOOLEAN, "int": abi.TV_INT, "integer": abi.TV_INTEGER, "decimal": abi.TV_DECIMAL, "float": abi.TV_FLOAT, "double": abi.TV_DOUBLE}
LANG, USD = 7, 9


class Zoo:
    """One small store: every case string as a simple literal (ids 1 ..), the same strings as other literals (`".."^^bsbm:USD`), then a
    few IRIs, language-tagged strings, numbers and a blank node; the last id is a simple literal, so its bytes end the heap."""

    def __init__(self):
        S = L.ALL_STRINGS
        rank = {s: r for r, s in enumerate(sorted(set(S) | {"abc", "2.5"}))}
        terms = [("simple", s) for s in S] + [("other", s) for s in S]
        self.iri, self.lang_num, self.lang_word = len(terms) + 1, len(terms) + 2, len(terms) + 3
        terms += [("iri", "http://example.org/12.5"), ("lang", "2.5"), ("lang", "abc")]
        self.integer, self.double, self.boolean, self.blank = (len(terms) + k for k in (1, 2, 3, 4))
        terms += [("integer", "42"), ("double", "2.5"), ("boolean", "true"), ("blank", "b0")]
        self.last = len(terms) + 1
        terms += [("simple", "2.5")]
        n = len(terms) + 1
        tv = np.zeros(n, TV_DTYPE)
        off = np.zeros(n + 1, np.uint64)
        heap = bytearray()
        for k, (kind, s) in enumerate(terms):
            i = k + 1
            b = s.encode("utf-8")
            if kind in ("simple", "lang"):
                tv[i] = (rank[s], LANG if kind == "lang" else 0, abi.TV_STRING, abi.TVF_EMPTY_STRING if not b else 0, 0)
            elif kind == "other":
                tv[i] = (i, USD, abi.TV_OTHER, 0, 0)
            elif kind == "iri":
                tv[i] = (i, 0, abi.TV_NAMED_NODE, 0, 0)
            elif kind == "blank":
                tv[i] = (i, 0, abi.TV_BLANK_NODE, 0, 0)
            elif kind == "integer":
                tv[i] = (42, 0, abi.TV_INTEGER, 0, 0)
            elif kind == "double":
                tv[i] = (struct.unpack("<q", struct.pack("<d", 2.5))[0], 0, abi.TV_DOUBLE, 0, 0)
            else:
                tv[i] = (1, 0, abi.TV_BOOLEAN, 0, 0)
            off[i] = len(heap)
            heap += b
            off[i + 1] = len(heap)
        self.terms, self.n_strings, self.tv = terms, len(S), tv
        self.simple = {s: 1 + k for k, s in enumerate(S)}
        self.other = {s: 1 + len(S) + k for k, s in enumerate(S)}
        self.gs = rf.GpuQuadStore()
        self.gs.set_typed_values(tv)
        self.gs.set_strings(off, bytes(heap))

    def lexical(self, i):
        """What xsd:string(ENC_TV(id)) is: the lexical form, None (the error value) or "fails" (a formatting cast)."""
        if i == 0 or i > len(self.terms):
            return None
        kind, s = self.terms[i - 1]
        return None if kind == "blank" else "fails" if kind in ("integer", "double", "boolean") else s


@pytest.fixture(scope="module")
def zoo():
    return Zoo()


def run(gs, cols, root_of, agg_columns=False):
    import torch
    pb = PlanBuilder()
    t = pb.table(0, len(cols))
    plan = gs.plan(pb.build(root_of(pb, t), agg_columns=agg_columns))
    keep, ptrs = table_on_device(torch, cols)
    plan.bind_table(0, ptrs, len(cols[0]))
    plan._keep_cols = keep
    plan.execute()
    return plan


def want(s, target):
    """(tag, lo, hi) as the device leaves the cast of the simple literal `s`, tag 0 for the error value; None where it may decline."""
    if s is None:
        return (0, 0, 0)
    st, bits, may = L.expected(s, target)
    if may or (st == "ok" and bits is None):
        return None
    if st != "ok":
        return (0, 0, 0)
    u = bits & ((1 << 128) - 1)
    s64 = lambda x: x - (1 << 64) if x >= 1 << 63 else x
    return (TAGS[target], s64(u & ((1 << 64) - 1)), s64(u >> 64) if target == "decimal" else 0)


def got_values(plan, column):
    v = plan.fetch_column_values(column)
    return [(int(v["tag"][r]), int(v["lo"][r]) & 0xFFFFFFFF if int(v["tag"][r]) == abi.TV_FLOAT else int(v["lo"][r]), int(v["hi"][r])) for r in range(len(v))]


def clean_ids(z, target, through_string):
    """Ids whose cast answers (does not fail the execute): simple literals — and, through xsd:string, other literals, the IRI, the
    language-tagged strings and the blank node; id 0 and an id beyond the table."""
    ids = [z.simple[s] for s in L.ALL_STRINGS if want(s, target) is not None] + [z.last, 0, len(z.tv) + 3]
    if through_string:
        ids += [z.other[s] for s in L.ALL_STRINGS if want(s, target) is not None] + [z.iri, z.lang_num, z.lang_word, z.blank]
    else:
        ids += [z.iri, z.lang_num, z.blank, z.other["2.5" if "2.5" in z.other else L.ALL_STRINGS[0]]]
    return ids


def expected_of(z, i, target, through_string):
    if through_string:
        return want(z.lexical(i), target)
    if 0 < i <= len(z.terms) and z.terms[i - 1][0] == "simple":
        return want(z.terms[i - 1][1], target)
    return (0, 0, 0)       # (of the ids used here: IRIs, language-tagged strings, other literals, blank nodes, null)


# ---------------------------------------------------------------------------------------------------
# 1. every target over the case tables, value for value (a computed column carries the cast's bits)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", L.TARGETS)
def test_cast_lex_row_for_row(torch_cuda, zoo, target):
    z = zoo
    for through_string in (False, True):
        ids = np.array(clean_ids(z, target, through_string), np.uint32)
        operand = P.xsd_string(ENC_TV(col(0))) if through_string else ENC_TV(col(0))
        plan = run(z.gs, [ids, np.arange(len(ids), dtype=np.uint32)], lambda pb, t: pb.extend(t, [P.CAST_LEX(operand, TAGS[target])]), agg_columns=True)
        rows = plan.fetch()[1].tolist()
        got = got_values(plan, 2)
        assert len(rows) == len(ids)
        for r, row in enumerate(rows):
            i = int(ids[row])
            assert got[r] == expected_of(z, i, target, through_string), (target, through_string, i, z.terms[i - 1] if 0 < i <= len(z.terms) else None, got[r])


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 257])
def test_cast_lex_in_a_filter(torch_cuda, zoo, n_rows):
    """FilterExec: EBV(EQ(cast, cast)) keeps the rows whose cast is a value (and no NaN), EBV(EQ(cast, literal)) the rows with that value;
    tables of 1, 63, 64, 65 and 257 rows: ragged waves and a ragged workgroup, strings of 0 to 400 bytes side by side in one wave."""
    z = zoo
    literal = {"boolean": P.boolean(True), "int": P.int32(7), "integer": P.integer(7), "decimal": P.decimal(5 * 10 ** 17),
               "float": P.float32(struct.unpack("<f", struct.pack("<I", 0x3F800001))[0]), "double": P.double(0.5)}
    value = {"boolean": 1, "int": 7, "integer": 7, "decimal": 5 * 10 ** 17, "float": 0x3F800001, "double": L.f64_bits(0.5)}
    for target in L.TARGETS:
        pool = clean_ids(z, target, True)
        first = {"float": "1.0000000596046448", "double": ".5", "integer": "+7", "int": "+7", "decimal": ".5", "boolean": "1"}[target]
        start = pool.index(z.simple[first])                 # the first row is one the literal filter keeps, at every table size
        ids = np.array([pool[(start + k) % len(pool)] for k in range(n_rows)], np.uint32)
        rowid = np.arange(1, n_rows + 1, dtype=np.uint32)
        cast = lambda: P.CAST_LEX(P.xsd_string(ENC_TV(col(0))), TAGS[target])
        exp = [expected_of(z, int(i), target, True) for i in ids]
        is_nan = lambda e: (target == "float" and (e[1] & 0x7FFFFFFF) > 0x7F800000) or (target == "double" and (e[1] & ((1 << 63) - 1)) > 0x7FF0000000000000)
        plan = run(z.gs, [ids, rowid], lambda pb, t: pb.filter(t, EBV(P.EQ(cast(), cast())), projection=[1]))
        np.testing.assert_array_equal(np.sort(plan.fetch()[0]), rowid[[e[0] != 0 and not is_nan(e) for e in exp]])
        plan = run(z.gs, [ids, rowid], lambda pb, t: pb.filter(t, EBV(P.EQ(cast(), literal[target])), projection=[1]))
        hit = [e[0] != 0 and ((e[1] & ((1 << 64) - 1)) | (e[2] << 64) if target == "decimal" else e[1]) == value[target] for e in exp]
        np.testing.assert_array_equal(np.sort(plan.fetch()[0]), rowid[hit])
        assert hit[0], target


# ---------------------------------------------------------------------------------------------------
# 2. the BI Q8 shape: filter=EBV(LT(xsd:float(xsd:string(ENC_TV(price))), avgPrice)) in an inner and a semi join
# ---------------------------------------------------------------------------------------------------
def f32_of(bits):
    return struct.unpack("<f", struct.pack("<I", bits & 0xFFFFFFFF))[0]


@pytest.mark.parametrize("join_type", [abi.JOIN_INNER, abi.JOIN_LEFT_SEMI, abi.JOIN_LEFT, abi.JOIN_LEFT_ANTI], ids=["inner", "semi", "left", "anti"])
def test_q8_join_filter(torch_cuda, zoo, join_type):
    import torch
    z = zoo
    prices = [s for s in L.ALL_STRINGS if want(s, "float") is not None]
    n = 300
    key = (np.arange(n, dtype=np.uint32) % 23) + 1
    price = np.array([z.other[prices[(5 * k) % len(prices)]] for k in range(n)], np.uint32)       # "…"^^bsbm:USD literals
    # the averages: one row per key, so AVG is that row's value — float literals of the store, made here
    avg_vals = [0.75, 2.5, 1e10, -1.0, 1e-40, 3.4e38, 100.0, 0.0]
    gs = rf.GpuQuadStore()
    tv = np.concatenate([z.tv, np.zeros(len(avg_vals), TV_DTYPE)])
    for k, v in enumerate(avg_vals):
        tv[len(z.tv) + k] = (L.f32_bits(v), 0, abi.TV_FLOAT, 0, 0)
    gs.set_typed_values(tv)
    off = np.zeros(len(tv) + 1, np.uint64)
    heap = bytearray()
    for i in range(1, len(z.tv)):
        b = z.terms[i - 1][1].encode("utf-8")
        off[i] = len(heap); heap += b; off[i + 1] = len(heap)
    off[len(z.tv):] = len(heap)
    gs.set_strings(off, bytes(heap))
    rkey = np.arange(1, 24, dtype=np.uint32)
    rval = np.array([len(z.tv) + (k % len(avg_vals)) for k in range(23)], np.uint32)
    pb = PlanBuilder()
    left, right = pb.table(0, 2), pb.table(1, 2)
    agg = pb.aggregate(right, [0], [(abi.AGG_AVG, 1)])
    flt = EBV(P.LT(P.xsd_float(P.xsd_string(ENC_TV(col(1))), lexical=True), ENC_TV(col(3))))
    root = pb.hash_join(left, agg, on=[(0, 0)], join_type=join_type, filter=flt, projection=[0, 1])
    plan = gs.plan(pb.build(root, agg_columns=True))
    k1, p1 = table_on_device(torch, [key, price])
    k2, p2 = table_on_device(torch, [rkey, rval])
    plan.bind_table(0, p1, n)
    plan.bind_table(1, p2, len(rkey))
    got = plan.execute().fetch()
    avg = {int(k): avg_vals[int(v) - len(z.tv)] for k, v in zip(rkey, rval)}            # the dict-and-loop reference
    exp, rest = [], []
    for k, p in zip(key.tolist(), price.tolist()):
        e = want(z.lexical(p), "float")
        (exp if e[0] and f32_of(e[1]) < np.float32(avg[k]) else rest).append((k, p))      # (every left row has one partner: inner = semi)
    assert 20 < len(exp) < n - 20
    # left outer: a row whose only partner fails the filter stays, unmatched — every left row once; anti: the rows semi drops
    want_rows = {abi.JOIN_INNER: exp, abi.JOIN_LEFT_SEMI: exp, abi.JOIN_LEFT: exp + rest, abi.JOIN_LEFT_ANTI: rest}[join_type]
    assert sorted(zip(got[0].tolist(), got[1].tolist())) == sorted(want_rows)


# ---------------------------------------------------------------------------------------------------
# 3. SUM / AVG over the cast, and the cast as a computed column that a SortExec orders
# ---------------------------------------------------------------------------------------------------
def py_value(e, target):
    if e[0] == 0:
        return (abi.TV_NULL, None)
    if target == "float":
        return (abi.TV_FLOAT, float(np.uint32(e[1]).view(np.float32)))
    return (abi.TV_DECIMAL, (e[2] << 64) + (e[1] & ((1 << 64) - 1)))      # (hi is signed)


def test_sum_and_avg_over_the_cast(torch_cuda, zoo):
    z = zoo
    for target, helper in (("float", P.xsd_float), ("decimal", P.xsd_decimal)):
        strings = [s for s in L.ALL_STRINGS if want(s, target) is not None]
        ids = np.array([z.other[s] for s in strings], np.uint32)
        key = (np.arange(len(ids), dtype=np.uint32) % 11) + 1
        e = lambda: helper(P.xsd_string(ENC_TV(col(1))), lexical=True)
        plan = run(z.gs, [key, ids], lambda pb, t: pb.aggregate(t, [0], [(abi.AGG_SUM, e()), (abi.AGG_AVG, e())]))
        keys = plan.fetch()[0].tolist()
        sums, avgs = plan.fetch_aggregate(0), plan.fetch_aggregate(1)
        assert sorted(keys) == list(range(1, 12))
        for r, k in enumerate(keys):
            vals = [py_value(want(s, target), target) for s, kk in zip(strings, key.tolist()) if kk == k]
            assert same(sum_agg(vals), (int(sums["tag"][r]), int(sums["lo"][r]), int(sums["hi"][r]))), (target, k)
            assert same(avg_agg(vals), (int(avgs["tag"][r]), int(avgs["lo"][r]), int(avgs["hi"][r]))), (target, k)
    # groups whose every row parses: the AVG is a value, not the error value
    good = [s for s in ("0.1", "0.3", "123456.78", "4.35", "5", "99999999") if s in z.other]
    ids = np.array([z.other[s] for s in good], np.uint32)
    plan = run(z.gs, [np.ones(len(ids), np.uint32), ids], lambda pb, t: pb.aggregate(t, [0], [(abi.AGG_AVG, P.xsd_decimal(P.xsd_string(ENC_TV(col(1))), lexical=True))]))
    v = plan.fetch_aggregate(0)
    assert same(avg_agg([py_value(want(s, "decimal"), "decimal") for s in good]), (int(v["tag"][0]), int(v["lo"][0]), int(v["hi"][0]))) and int(v["tag"][0]) == abi.TV_DECIMAL


def test_the_cast_as_a_computed_column_sorted(torch_cuda, zoo):
    z = zoo
    strings = [s for s in L.ALL_STRINGS if want(s, "float") not in (None, (0, 0, 0)) and (want(s, "float")[1] & 0x7FFFFFFF) <= 0x7F800000]   # values, no NaN
    ids = np.array([z.other[s] for s in strings], np.uint32)
    rowid = np.arange(len(ids), dtype=np.uint32) + 1

    def root(pb, t):
        e = pb.extend(t, [P.xsd_float(P.xsd_string(ENC_TV(col(0))), lexical=True)], names=["price"])
        return pb.sort(e, [(2, abi.SORT_BY_VALUE, True), (1, abi.SORT_BY_ID, False)])
    plan = run(z.gs, [ids, rowid], root, agg_columns=True)
    got_rows = plan.fetch()[1].tolist()
    # DESC by the value in IEEE total order (-0 below +0: RDFGPU_SORT_BY_VALUE), then ASC by the row id among equal values
    bits = {int(r): want(s, "float")[1] for r, s in zip(rowid, strings)}
    total = lambda b: (~b & 0xFFFFFFFF) if b >> 31 else b | 0x80000000
    assert got_rows == sorted(bits, key=lambda r: (-total(bits[r]), r))
    assert len({b for b in bits.values()}) < len(bits)          # (equal values exist: the tie-break is exercised)
    assert [got_values(plan, 2)[k][1] for k in range(len(got_rows))] == [want(strings[r - 1], "float")[1] for r in got_rows]


# ---------------------------------------------------------------------------------------------------
# 4. CAST_STRING by kind
# ---------------------------------------------------------------------------------------------------
def test_cast_string_by_kind(torch_cuda, zoo):
    z = zoo
    ids = np.array([z.iri, z.other["123456.78"], z.lang_num, z.lang_word, z.simple["123456.78"], z.simple[""], z.blank, 0, z.last], np.uint32)
    rowid = np.arange(1, len(ids) + 1, dtype=np.uint32)
    S = lambda: P.xsd_string(ENC_TV(col(0)))
    keep = lambda pred: np.sort(run(z.gs, [ids, rowid], lambda pb, t: pb.filter(t, EBV(pred), projection=[1])).fetch()[0]).tolist()
    lex = [z.lexical(int(i)) for i in ids]
    for n_chars in (0, 3, 9, 23):
        assert keep(P.EQ(P.STRLEN(S()), P.integer(n_chars))) == [int(r) for r, s in zip(rowid, lex) if s is not None and len(s) == n_chars]
    assert keep(P.STRSTARTS(S(), "http://")) == [1] and keep(P.STRSTARTS(S(), "1234")) == [2, 5] and keep(P.STRSTARTS(S(), "")) == [1, 2, 3, 4, 5, 6, 9]
    assert keep(P.EQ(S(), P.lit_str("2.5"))) == [3, 9]                                   # the language is gone: a simple literal
    # CAST_LEX of a SUBSTR of the view: "123456.78"[4:] = "456.78", "http://example.org/12.5"[20:] = "12.5"
    assert keep(P.EQ(P.xsd_decimal(P.SUBSTR(S(), P.integer(4)), lexical=True), P.decimal(45678 * 10 ** 16))) == [2, 5]
    assert keep(P.EQ(P.xsd_float(P.SUBSTR(S(), P.integer(20)), lexical=True), P.float32(12.5))) == [1]
    assert keep(P.EQ(P.xsd_integer(P.SUBSTR(S(), P.integer(1), P.integer(3)), lexical=True), P.integer(123))) == [2, 5]
    assert keep(P.EQ(P.xsd_double(P.lit_str("1e3"), lexical=True), P.double(1000.0))) == list(range(1, len(ids) + 1))   # a constant with bytes
    # a numeric row: the reference formats the value — the execute fails, and the plan is usable on the next table
    import torch
    pb = PlanBuilder()
    plan = z.gs.plan(pb.build(pb.filter(pb.table(0, 2), EBV(P.EQ(P.STRLEN(S()), P.integer(3))), projection=[1])))
    for bad in (z.integer, z.double, z.boolean):
        c = np.append(ids, bad).astype(np.uint32)
        k, p = table_on_device(torch, [c, np.arange(1, len(c) + 1, dtype=np.uint32)])
        plan.bind_table(0, p, len(c))
        with pytest.raises(RdfGpuError) as e:
            plan.execute()
        assert e.value.status == abi.ERR_UNSUPPORTED
        k, p = table_on_device(torch, [ids, rowid])
        plan.bind_table(0, p, len(ids))
        assert np.sort(plan.execute().fetch()[0]).tolist() == [3, 4, 9]


# ---------------------------------------------------------------------------------------------------
# 5. what fails the execute, loudly
# ---------------------------------------------------------------------------------------------------
def test_a_declining_literal_fails_the_execute(torch_cuda, zoo):
    import torch
    z = zoo
    cases = [("double", L.DECLINING), ("float", L.DECLINING_FLOAT), ("float", "-nan"), ("double", "+nan")]
    for target, s in cases:
        assert L.declines(s, target)
        pb = PlanBuilder()
        e = P.CAST_LEX(P.xsd_string(ENC_TV(col(0))), TAGS[target])
        plan = z.gs.plan(pb.build(pb.filter(pb.table(0, 2), EBV(P.EQ(e, e)), projection=[1])))
        good = np.array([z.other["0.1"], z.other["1e23"], z.simple["4.35"]], np.uint32)
        for with_it in (True, False, True):
            c = np.append(good, z.other[s]).astype(np.uint32) if with_it else good
            k, p = table_on_device(torch, [c, np.arange(1, len(c) + 1, dtype=np.uint32)])
            plan.bind_table(0, p, len(c))
            if with_it:
                with pytest.raises(RdfGpuError) as err:
                    plan.execute()
                assert err.value.status == abi.ERR_UNSUPPORTED and "CAST_LEX" in str(err.value)
            else:
                assert np.sort(plan.execute().fetch()[0]).tolist() == [1, 2, 3]


def test_plain_cast_of_a_simple_literal_still_fails_the_execute(torch_cuda, zoo):
    z = zoo
    ids = np.array([z.simple["4.35"], z.integer], np.uint32)
    with pytest.raises(RdfGpuError) as e:
        run(z.gs, [ids, ids], lambda pb, t: pb.filter(t, EBV(P.EQ(P.xsd_float(ENC_TV(col(0))), P.float32(4.35)))))
    assert e.value.status == abi.ERR_UNSUPPORTED
    # .. and the lexical form of the same cast answers
    plan = run(z.gs, [ids, ids], lambda pb, t: pb.filter(t, EBV(P.EQ(P.xsd_float(ENC_TV(col(0)), lexical=True), P.float32(4.35)))))
    assert plan.fetch()[0].tolist() == [z.simple["4.35"]]


def test_a_store_without_strings_refuses_the_plan(torch_cuda):
    """Both ops read lexical forms: like STR, a store without rdfgpu_store_set_strings refuses the plan at compile (otherwise every row
    would silently be the error value)."""
    gs = rf.GpuQuadStore()
    gs.set_typed_values(np.zeros(4, TV_DTYPE))
    for e in (P.EQ(P.xsd_string(ENC_TV(col(0))), P.xsd_string(ENC_TV(col(1)))), P.EQ(P.xsd_float(ENC_TV(col(0)), lexical=True), P.float32(1.0))):
        pb = PlanBuilder()
        with pytest.raises(RdfGpuError) as err:
            gs.plan(pb.build(pb.filter(pb.table(0, 2), EBV(e))))
        assert err.value.status == abi.ERR_INVALID and "rdfgpu_store_set_strings" in str(err.value)
    pb = PlanBuilder()                                          # .. and the same store takes a plan without them
    gs.plan(pb.build(pb.filter(pb.table(0, 2), EBV(P.EQ(P.xsd_float(ENC_TV(col(0))), P.float32(1.0))))))
