"""GROUP BY over value columns and up to 8 group columns (RDFGPU_PLAN_VALUE_KEYS, agg_groups_wide_kernel) on the MI355X against a Python
dict: groups and aggregate values compared as a set of rows.  Row counts at the wave, tile and second-tile edges of the group pass; one
group, all rows distinct, about n / 3 groups; one value key, the Wind Farm list (2 id + 5 value keys), 8 id keys, 5 id keys that differ
in the last column only; the terms a value key tells apart and the ones it merges; an aggregate's value column as key; both accumulate
forms, MIN / MAX beside AVG, HAVING and SortExec above the node, one plan over tables of two sizes; and which group pass ran.

(The header also says that `hi` of a record that is no decimal is ignored.  EXTEND and the aggregates write 0 there, so no plan can hold
such a record: the rule is the kernel's by construction — it reads `hi` under the decimal tag only — and is not exercised here.)"""
from collections import Counter, defaultdict

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi
from rdf_fusion_amd import plan as P
from rdf_fusion_amd.engine import TV_DTYPE
from rdf_fusion_amd.plan import PlanBuilder, col, ENC_TV, EBV
from test_gpu_parity import table_on_device
import numeric_ref as nr

E18 = 10 ** 18
INTEGER, INT, DEC, FLT, DBL, BOOL, NULL = abi.TV_INTEGER, abi.TV_INT, abi.TV_DECIMAL, abi.TV_FLOAT, abi.TV_DOUBLE, abi.TV_BOOLEAN, abi.TV_NULL
STAR, COUNT, SUM, AVG, MIN, MAX = abi.AGG_COUNT_STAR, abi.AGG_COUNT, abi.AGG_SUM, abi.AGG_AVG, abi.AGG_MIN, abi.AGG_MAX
ROW_COUNTS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049]      # wave, tile (1024 rows) and second-tile edges of the group pass
A, B, N_INT = 100, 3000, 2100                                # ids A + v and B + v are both xsd:integer v (v < N_INT): one value, two ids
X = 0x0123456789ABCDEF
# id -> (tag, lo, hi): the terms a value key tells apart, and the ones it merges
SPECIAL = {
    1: (FLT, 0x7FC00000, 0), 2: (FLT, 0x7FC00001, 0), 3: (FLT, 0xFFC12345, 0),          # NaNs of three payloads: one term
    4: (FLT, 0x00000000, 0), 5: (FLT, 0x80000000, 0),                                    # +0.0 and -0.0: two terms
    6: (DBL, 0x7FF8000000000000, 0), 7: (DBL, 0x7FF0000000000001, 0),
    8: (DBL, 0, 0), 9: (DBL, -(1 << 63), 0),
    10: (INTEGER, 5, 0), 11: (INT, 5, 0), 12: (DEC, 5 * E18, 0),                        # 5, 5 and 5.0: three terms
    13: (DEC, X, 0), 14: (DEC, X, 1),                                                    # equal in lo, different in hi: two terms
    15: (BOOL, 1, 0), 16: (INTEGER, 5, 0),                                               # a second id of xsd:integer 5: the term of id 10
    17: (FLT, 0x3FC00000, 0), 18: (DBL, 0x3FF8000000000000, 0),                          # 1.5 and 1.5: two terms
}
BEYOND = B + N_INT + 7                                         # an id behind the table: null, like id 0


def typed(i):
    """(tag, lo, hi) of object id i; None: unbound"""
    if i in SPECIAL:
        return SPECIAL[i]
    if A <= i < A + N_INT:
        return (INTEGER, i - A, 0)
    if B <= i < B + N_INT:
        return (INTEGER, i - B, 0)
    return None


def term(v):
    """the plain term a value stands for, as a group key: every NaN of a tag is one term, `hi` counts for a decimal only, unbound is one key"""
    if v is None or v[0] == NULL:
        return (NULL, 0, 0)
    tag, lo, hi = v
    return nr.device_bits(tag, lo - (1 << 64) if lo >= 1 << 63 else lo, hi)


@pytest.fixture(scope="module")
def gs(torch_cuda):
    tv = np.zeros(B + N_INT, TV_DTYPE)
    dec = []
    for i in range(1, len(tv)):
        v = typed(i)
        if v is None:
            continue
        tag, lo, hi = v
        if tag == DEC:
            dec.append((lo if lo < 1 << 63 else lo - (1 << 64), hi))
            lo = len(dec) - 1
        tv[i] = (np.uint64(lo & (2 ** 64 - 1)).astype(np.int64), 0, tag, 0, 0)
    store = rf.GpuQuadStore()
    store.set_typed_values(tv, np.array(dec, np.int64).reshape(-1, 2))
    return store


class Run:
    def __init__(self, gs, n_cols, root_of, form=None, value_keys=True):
        self.pb = PlanBuilder()
        self.root = root_of(self.pb, self.pb.table(0, n_cols))
        self.plan = gs.plan(self.pb.build(self.root, agg_columns=True, value_keys=value_keys))
        self.plan.enable_kernel_timing(True)
        if form:
            self.plan.set_option(form, 1)

    def execute(self, torch, cols):
        self.keep, ptrs = table_on_device(torch, cols)
        self.plan.bind_table(0, ptrs, len(cols[0]))
        self.plan.execute()
        return self

    def rows(self):
        """the result as a sorted list of rows: an id column's id, a value column's (tag, lo, hi)"""
        n, width = self.plan.result_info()
        ids = self.plan.fetch()
        out = []
        for q in range(width):
            if self.pb.values[self.root][q]:
                out.append([nr.device_bits(int(v["tag"]), int(v["lo"]), int(v["hi"])) for v in self.plan.fetch_column_values(q)])
            else:
                out.append([int(x) for x in ids[q][:n]])
        return sorted(zip(*out), key=repr) if width and n else []

    def kernels(self):
        return [s[0] for s in self.plan.kernel_stats() if s[1]]


def reference(cols, keys, aggs):
    """keys = [(column, is a value key)], aggs = [(fn, column of xsd:integer ids)] -> the sorted rows a plan must give"""
    groups = defaultdict(list)
    for r in range(len(cols[0])):
        groups[tuple(term(typed(int(cols[c][r]))) if by_value else int(cols[c][r]) for c, by_value in keys)].append(r)
    out = []
    for key, members in groups.items():
        row = list(key)
        for fn, c in aggs:
            xs = [typed(int(cols[c][r]))[1] for r in members] if c is not None else []
            if fn == STAR:
                row.append(nr.bits((INTEGER, len(members))))
            elif fn == SUM:
                row.append(nr.bits((INTEGER, sum(xs))))
            elif fn == AVG:
                row.append(nr.bits((DEC, nr.dec_div(sum(xs) * E18, len(xs) * E18))))
            else:
                row.append(nr.bits((INTEGER, min(xs) if fn == MIN else max(xs))))
        out.append(tuple(row))
    return sorted(out, key=repr)


def group_numbers(n, mode, rng):
    g = np.zeros(n, np.int64) if mode == "one" else np.arange(n) if mode == "distinct" else np.arange(n) % max(1, n // 3)
    return g[rng.permutation(n)] if n else g


def key_column(g, j, last, by_value, rng):
    """column j of a key list for group numbers g: the last key is the group number itself, the others a function of it — so tuples differ
    exactly where the group numbers do.  A value key reaches its xsd:integer through either of two ids, an id key through one."""
    v = g if last else (g * (2 * j + 3)) % 5
    base = np.where(rng.integers(0, 2, len(g)) == 1, B, A) if by_value else A
    return (v + base).astype(np.uint32)


# key lists: (name, [is a value key per key], constant leading keys)
KEY_LISTS = {
    "one_value_key": [True],
    "wind_farm_2_id_5_value": [False, False, True, True, True, True, True],
    "eight_id_keys": [False] * 8,
    "five_id_keys_last_differs": [False] * 5,
}


def build_case(name, n, mode, seed):
    """(table columns, keys for the builder, root_of): the id columns, then — for value keys — an EXTEND of ENC_TV(column)"""
    rng = np.random.default_rng(seed)
    kinds = KEY_LISTS[name]
    g = group_numbers(n, mode, rng)
    cols = []
    for j, by_value in enumerate(kinds):
        last = j == len(kinds) - 1
        c = key_column(g, j, last, by_value, rng)
        if name == "five_id_keys_last_differs" and not last:
            c = np.full(n, A + 1, np.uint32)                         # keys 0..3 constant: only right_keys[0] tells the groups apart
        cols.append(c)
    x = (rng.integers(0, 50, n) + A).astype(np.uint32)               # the aggregates' input: xsd:integer 0..49
    cols.append(x)
    xi = len(kinds)
    value_cols = [j for j, v in enumerate(kinds) if v]

    def root_of(pb, t):
        src, pos = t, {j: j for j in range(len(kinds))}
        if value_cols:
            src = pb.extend(t, [ENC_TV(col(j)) for j in value_cols], names=[f"v{j}" for j in value_cols])
            for q, j in enumerate(value_cols):
                pos[j] = len(kinds) + 1 + q
        return pb.aggregate(src, [pos[j] for j in range(len(kinds))], [(STAR, None), (SUM, xi)])
    return cols, [(j, v) for j, v in enumerate(kinds)], root_of, xi


@pytest.mark.parametrize("mode", ["one", "distinct", "third"])
@pytest.mark.parametrize("n", ROW_COUNTS)
@pytest.mark.parametrize("name", list(KEY_LISTS))
def test_groups_against_a_dict(torch_cuda, gs, name, n, mode):
    cols, keys, root_of, xi = build_case(name, n, mode, seed=n * 7 + len(name))
    run = Run(gs, len(cols), root_of).execute(torch_cuda, cols)
    want = reference(cols, keys, [(STAR, None), (SUM, xi)])
    assert run.plan.result_info() == (len(want), len(keys) + 2)
    assert run.rows() == want
    names = run.kernels()
    if n:
        assert any(k == "rdfgpu::agg_groups_wide_kernel" for k in names) and not any(k == "rdfgpu::agg_groups_kernel" for k in names), names
        assert any(k == "rdfgpu::agg_wide_keys_kernel" for k in names) == (len(keys) > 4 and len(want) > 0), names
    if mode == "one":
        assert len(want) == min(n, 1)
    if mode == "distinct":
        assert len(want) == n


def test_the_terms_a_value_key_tells_apart(torch_cuda, gs):
    rng = np.random.default_rng(3)
    ids = np.array((list(SPECIAL) + [0, BEYOND]) * 9, np.uint32)[rng.permutation(9 * (len(SPECIAL) + 2))]
    x = (rng.integers(0, 50, len(ids)) + A).astype(np.uint32)
    root_of = lambda pb, t: pb.aggregate(pb.extend(t, [ENC_TV(col(0))], names=["v"]), [2], [(STAR, None), (SUM, 1)])
    run = Run(gs, 2, root_of).execute(torch_cuda, [ids, x])
    want = reference([ids, x], [(0, True)], [(STAR, None), (SUM, 1)])
    assert run.rows() == want
    by_key = {r[0]: r[1][1] for r in want}
    assert len(want) == 15
    assert by_key[(FLT, "nan", 0)] == 27 and by_key[(DBL, "nan", 0)] == 18                      # NaNs of one tag: one group
    assert by_key[(FLT, 0, 0)] == 9 and by_key[(FLT, 0x80000000, 0)] == 9                        # +0.0 / -0.0
    assert by_key[(DBL, 0, 0)] == 9 and by_key[(DBL, -(1 << 63), 0)] == 9
    assert by_key[(INTEGER, 5, 0)] == 18 and by_key[(INT, 5, 0)] == 9 and by_key[nr.bits((DEC, 5 * E18))] == 9
    assert by_key[(DEC, X, 0)] == 9 and by_key[(DEC, X, 1)] == 9                                 # decimals: hi counts
    assert by_key[(NULL, 0, 0)] == 18                                                            # id 0 and an id behind the table: one "unbound"
    # the key stays a value column: the representative row's entry is bound exactly where the key is
    entries = run.plan.fetch()[0]
    vals = run.plan.fetch_column_values(0)
    assert [(e == 0) for e in entries.tolist()] == [int(v["tag"]) == NULL for v in vals]


def test_an_aggregates_value_column_as_key(torch_cuda, gs):
    """COUNT per k, then the groups of equal counts: a histogram of the counts"""
    rng = np.random.default_rng(11)
    k = (rng.integers(0, 300, 2049) ** 2 % 97 + A).astype(np.uint32)
    x = (rng.integers(0, 50, len(k)) + A).astype(np.uint32)
    x[::17] = 0                                                                                   # unbound: COUNT skips them
    root_of = lambda pb, t: pb.aggregate(pb.aggregate(t, [0], [(COUNT, 1)]), [1], [(STAR, None)])
    run = Run(gs, 2, root_of).execute(torch_cuda, [k, x])
    counts = Counter(int(a) for a, b in zip(k, x) if b != 0)
    for a in set(int(a) for a in k):
        counts.setdefault(a, 0)
    want = sorted(((INTEGER, c, 0), (INTEGER, m, 0)) for c, m in Counter(counts.values()).items())
    assert run.rows() == sorted(want, key=repr) and len(want) < len(counts)
    names = run.kernels()
    assert "rdfgpu::agg_groups_kernel" in names and "rdfgpu::agg_groups_wide_kernel" in names    # the id-key node below runs the old pass


@pytest.mark.parametrize("form", [None, "NO_AGG_LDS"])
def test_accumulate_forms_and_minmax_beside_avg(torch_cuda, gs, form):
    """24 groups by a value key and an id key: AVG, MIN and MAX of one column (the MINMAX instantiation and its refinement) in the LDS and
    the HBM form of the shared accumulate pass"""
    rng = np.random.default_rng(5)
    n = 1500
    g = rng.integers(0, 12, n)
    v = (g + np.where(rng.integers(0, 2, n) == 1, B, A)).astype(np.uint32)
    w = (rng.integers(0, 2, n) + A).astype(np.uint32)
    x = (rng.integers(0, 50, n) + A).astype(np.uint32)
    aggs = [(AVG, 2), (MIN, 2), (MAX, 2), (STAR, None)]
    root_of = lambda pb, t: pb.aggregate(pb.extend(t, [ENC_TV(col(0))], names=["v"]), [3, 1], aggs)
    run = Run(gs, 3, root_of, form=form).execute(torch_cuda, [v, w, x])
    assert run.rows() == reference([v, w, x], [(0, True), (1, False)], aggs)
    names = run.kernels()
    assert any(k.startswith("void rdfgpu::agg_accum_minmax") and k.endswith("<%s>" % ("false" if form else "true")) for k in names), names
    assert "rdfgpu::agg_groups_wide_kernel" in names and "rdfgpu::agg_wide_keys_kernel" not in names     # two keys: agg_final_kernel copies them


def test_having_and_sort_above_the_node(torch_cuda, gs):
    """FILTERs that read the value key and the COUNT, then SortExec by the key's value: the node's output works like any value column"""
    rng = np.random.default_rng(9)
    n = 1025
    g = rng.integers(0, 40, n) ** 2 % 31
    v = (g + np.where(rng.integers(0, 2, n) == 1, B, A)).astype(np.uint32)

    def root_of(pb, t):
        a = pb.aggregate(pb.extend(t, [ENC_TV(col(0))], names=["v"]), [1], [(STAR, None)])
        h = pb.sparql_having(a, P.AND(EBV(P.GT(ENC_TV(col(1)), P.integer(30))), EBV(P.GEQ(ENC_TV(col(0)), P.integer(4)))))
        return pb.sparql_order_by(h, [(0, True)])
    run = Run(gs, 1, root_of).execute(torch_cuda, [v])
    counts = Counter(int(x) for x in g)
    want = [(k, c) for k, c in sorted(counts.items(), reverse=True) if c > 30 and k >= 4]
    assert len(want) >= 3 and len(want) < len(counts)
    assert list(zip(run.plan.column_values(0), run.plan.column_values(1))) == want               # in SortExec's order: the key descending


def test_one_plan_over_tables_of_two_sizes(torch_cuda, gs):
    cols1, keys, root_of, xi = build_case("wind_farm_2_id_5_value", 65, "third", seed=1)
    cols2, _, _, _ = build_case("wind_farm_2_id_5_value", 1025, "third", seed=2)
    run = Run(gs, len(cols1), root_of)
    for cols in (cols1, cols2, cols1):
        run.execute(torch_cuda, cols)
        assert run.rows() == reference(cols, keys, [(STAR, None), (SUM, xi)])


def test_three_id_keys_in_a_value_keys_plan_run_the_old_group_pass(torch_cuda, gs):
    rng = np.random.default_rng(2)
    cols = [(rng.integers(0, 4, 2049) + A).astype(np.uint32) for _ in range(3)] + [(rng.integers(0, 50, 2049) + A).astype(np.uint32)]
    for value_keys in (True, False):
        run = Run(gs, 4, lambda pb, t: pb.aggregate(t, [0, 1, 2], [(STAR, None), (SUM, 3)]), value_keys=value_keys).execute(torch_cuda, cols)
        assert run.rows() == reference(cols, [(0, False), (1, False), (2, False)], [(STAR, None), (SUM, 3)])
        names = run.kernels()
        assert "rdfgpu::agg_groups_kernel" in names and not any("wide" in k for k in names), names


def test_refusals_reach_the_caller(torch_cuda, gs):
    pb = PlanBuilder()
    nine = pb.aggregate(pb.table(0, 9), list(range(9)), [])
    with pytest.raises(rf.engine.RdfGpuError, match=r"AggregateExec with 9 group columns \(at most 8\)"):
        gs.plan(pb.build(nine, agg_columns=True, value_keys=True))
    with pytest.raises(rf.engine.RdfGpuError, match=r"AggregateExec with 9 group columns \(at most 4\)"):
        gs.plan(pb.build(nine, agg_columns=True))
    d = pb.build(pb.aggregate(pb.table(0, 2), [0], []), agg_columns=True, value_keys=True)
    d.desc.flags = abi.PLAN_VALUE_KEYS                                                           # the flag alone
    with pytest.raises(rf.engine.RdfGpuError, match="RDFGPU_PLAN_VALUE_KEYS is valid only together with RDFGPU_PLAN_AGG_COLUMNS"):
        gs.plan(d)


# ---------------------------------------------------------------------------------------------------
# end to end: the Wind Farm GroupedProduction plan over a generated store, against a pure-Python evaluation
# ---------------------------------------------------------------------------------------------------
def timestamp_cmp(a, b):
    """PartialOrd for Timestamp (date_time.rs:1617-1654) over (value, has a timezone): -1 / 0 / 1, None where the order is not determined"""
    (x, tx), (y, ty) = a, b
    cmp = lambda p, q: (p > q) - (p < q)
    if tx == ty:
        return cmp(x, y)
    shift = 14 * 3600 * E18
    plus, minus = (cmp(x, y + shift), cmp(x, y - shift)) if tx else (cmp(x + shift, y), cmp(x - shift, y))
    return plus if plus == minus else None


def evaluate_grouped_production(ds, site_label, t_from, t_to):
    """the plan's answer from the triples alone: {(site label id, turbine label id, year, month, day, hour, minute_10): (sum, count)}"""
    import datepart_cases as D
    from rdf_fusion_amd import xsd
    by = defaultdict(lambda: defaultdict(list))
    for s, p, o in zip(ds.s.tolist(), ds.p.tolist(), ds.o.tolist()):
        by[p][s].append(o)
    pr, cl = ds.pred, ds.cls
    rev = lambda p: {o: s for s, os_ in by[pr[p]].items() for o in os_}                      # (functional in this store)
    node_of = rev("rds:hasFunctionalAspectNode")
    is_a = lambda x, c: cl[c] in by[pr["rdf:type"]].get(x, [])
    stamp = lambda t: (int(ds.decimals[ds.typed_values["lo"][t]][1]) << 64 | int(ds.decimals[ds.typed_values["lo"][t]][0]) & (2 ** 64 - 1),
                       bool(ds.typed_values["aux"][t] & 1), int(ds.typed_values["tz_minutes"][t]))
    lo, hi = (xsd.parse_date_time(t_from)[0], False), (xsd.parse_date_time(t_to)[0], False)
    out = defaultdict(lambda: [0, 0])
    for site, labels in by[pr["rdfs:label"]].items():
        if not is_a(site, "rds:Site") or ds.labels[site_label] not in labels:
            continue
        for wtur_asp in by[pr["rds:hasFunctionalAspect"]][site]:
            wtur = node_of[wtur_asp]
            assert is_a(wtur, "rds:A")
            for gensys_asp in by[pr["rds:hasFunctionalAspect"]][wtur]:
                gensys = node_of[gensys_asp]
                for gen_asp in by[pr["rds:hasFunctionalAspect"]][gensys]:
                    gen = node_of[gen_asp]
                    assert is_a(gensys, "rds:RA") and is_a(gen, "rds:GAA")
                    for ts in by[pr["ct:hasTimeseries"]][gen]:
                        if ds.labels["Production"] not in by[pr["rdfs:label"]][ts]:
                            continue
                        for dp in by[pr["ct:hasDataPoint"]][ts]:
                            (val,), (t,) = by[pr["ct:hasValue"]][dp], by[pr["ct:hasTimestamp"]][dp]
                            v, has, tz = stamp(t)
                            if timestamp_cmp((v, has), lo) not in (0, 1) or timestamp_cmp((v, has), hi) not in (0, -1):
                                continue
                            p = D.parts(v, has, tz)
                            for wl in by[pr["rdfs:label"]][wtur_asp]:
                                acc = out[(ds.labels[site_label], wl, p["year"], p["month"], p["day"], p["hours"], p["minutes"] // 10 * 10)]
                                acc[0] += int(ds.typed_values["lo"][val]); acc[1] += 1
    return out


def test_grouped_production_end_to_end(torch_cuda):
    """the smallest Wind Farm store (three turbines of the site asked for, a few thousand data points that straddle the end of August,
    timestamps in UTC, at +05:30 and without a timezone) through the whole plan: joins, the dateTime FILTER, one EXTEND, the 7-key AVG"""
    from rdf_fusion_amd import windfarm as wf
    ds = wf.generate(points_per_series=700)
    assert 3000 < ds.counts["data_points"] < 6000
    store = rf.GpuQuadStore()
    store.extend(ds.g, ds.s, ds.p, ds.o)
    store.set_typed_values(ds.typed_values, ds.decimals)
    t_from, t_to = "2022-08-31T21:07:00", "2022-09-02T18:43:00"
    pb, root = wf.grouped_production(ds, "Wind Mountain", None, t_from, t_to)
    plan = store.plan(pb.build(root, agg_columns=True, value_keys=True))
    plan.enable_kernel_timing(True)
    plan.execute()
    want = evaluate_grouped_production(ds, "Wind Mountain", t_from, t_to)
    turbines = {k[1] for k in want}
    assert len(turbines) == 3 and {k[3] for k in want} == {8, 9} and len(want) > 300               # three turbines, both months
    assert sum(c for _, c in want.values()) < 3 * 700                                             # the FILTER dropped rows (the edges, and 14 h of doubt)
    ids = plan.fetch()
    cols = [ids[0].tolist(), ids[1].tolist()] + [plan.column_values(q) for q in range(2, 8)]
    got = {}
    for row in zip(*cols):
        key = row[:6] + (int(row[6]),)
        assert key not in got and row[6].denominator == 1
        got[key] = row[7]
    assert set(got) == set(want)
    from fractions import Fraction
    for key, (total, count) in want.items():
        assert got[key] == Fraction(nr.dec_div(total * E18, count * E18), E18), key
    names = [s[0] for s in plan.kernel_stats() if s[1]]
    assert "rdfgpu::agg_groups_wide_kernel" in names and "rdfgpu::agg_wide_keys_kernel" in names and any("extend" in k for k in names)
