"""The functional forms (IF, COALESCE, IN / NOT IN), the term tests, LANG(x) = "tag" and the LeftMark join on the MI355X, row for row
against the Python references of forms_cases.py.

A predicate P is compared three-valued: a FilterExec over P keeps exactly the rows where the reference says true, one over NOT(P) exactly
those where it says false — the rest are errors.  A value is compared as the (tag, lo, hi) record of a computed column."""
from collections import Counter

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi
from rdf_fusion_amd import plan as P
from rdf_fusion_amd.engine import RdfGpuError
from rdf_fusion_amd.plan import PlanBuilder, col, ENC_TV, EBV
import forms_cases as F
from test_gpu_parity import table_on_device

SEMI, ANTI, MARK = abi.JOIN_LEFT_SEMI, abi.JOIN_LEFT_ANTI, abi.JOIN_LEFT_MARK
HASH, NLJ = abi.NODE_HASH_JOIN, abi.NODE_NESTED_LOOP_JOIN
N_MAX = max(F.ROW_COUNTS)


@pytest.fixture(scope="module")
def gs():
    st = rf.GpuQuadStore()
    st.set_typed_values(*F.typed_table())
    st.set_strings(*F.string_heap())
    return st


@pytest.fixture(scope="module")
def reference():
    """form name -> the reference's value on each of the N_MAX rows of id_columns (a shorter table is a prefix of it)"""
    cols = F.id_columns(N_MAX)
    rows = list(zip(*[c.tolist() for c in cols]))
    forms = dict(F.filter_forms())
    forms.update(F.value_forms())
    return {name: [x.fn(r) for r in rows] for name, x in forms.items()}


def execute(torch, gs, desc, tables, options=None, timing=False):
    keep, plan = [], gs.plan(desc)
    if timing:
        plan.enable_kernel_timing(True)
    for name, value in (options or {}).items():
        plan.set_option(name, value)
    for slot, cols in enumerate(tables):
        k, p = table_on_device(torch, cols)
        keep.append(k)
        plan.bind_table(slot, p, len(cols[0]))
    plan.execute()
    plan._tables = keep
    return plan


def rows(plan):
    n, _ = plan.result_info()
    return list(zip(*[c[:n].tolist() for c in plan.fetch()]))


def kept(torch, gs, pred, cols, rid):
    pb = PlanBuilder()
    plan = execute(torch, gs, pb.build(pb.filter(pb.table(0, len(cols)), pred, projection=[rid])), [cols])
    return sorted(r[0] for r in rows(plan))


def check_three_valued(torch, gs, x, cols, want, rid=3):
    """x: an X of kind TV(boolean | null); want: the reference's value per row"""
    e = P.EBV(x.expr)
    assert kept(torch, gs, e, cols, rid) == [i + 1 for i, v in enumerate(want) if v == F.tv_bool(True)]
    assert kept(torch, gs, P.NOT(e), cols, rid) == [i + 1 for i, v in enumerate(want) if v == F.tv_bool(False)]


def records(plan, column):
    return [(int(v["tag"]), int(v["lo"]), int(v["hi"])) for v in plan.fetch_column_values(column)]


# ---------------------------------------------------------------------------------------------------
# 1. the hand-written truth tables
# ---------------------------------------------------------------------------------------------------
def test_if_truth_table(torch_cuda, gs):
    cols = [np.array([r[k] for r in F.IF_TRUTH], np.uint32) for k in range(3)]
    pb = PlanBuilder()
    x = pb.extend(pb.table(0, 3), [P.IF(ENC_TV(col(0)), ENC_TV(col(1)), ENC_TV(col(2)))])
    plan = execute(torch_cuda, gs, pb.build(x, agg_columns=True), [cols])
    assert records(plan, 3) == [F.record(F.enc(r[3])) for r in F.IF_TRUTH]


@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_coalesce_truth_table(torch_cuda, gs, k):
    cases = [(ops, want) for ops, want in F.COALESCE_TRUTH if len(ops) == k]
    cols = [np.array([ops[q] for ops, _ in cases], np.uint32) for q in range(k)] + [np.array([w for _, w in cases], np.uint32),
                                                                                     np.arange(1, len(cases) + 1, dtype=np.uint32)]
    c = F.xcoalesce(*[F.xenc(q) for q in range(k)])
    # the value IS the expected one where there is one (`=` holds: no NaN among the values) and no term at all where there is none
    same = F.xeq(c, F.xenc(k))
    want = [same.fn(r) for r in zip(*[x.tolist() for x in cols])]
    assert want == [F.tv_bool(True) if w else F.NULL for _, w in cases]
    check_three_valued(torch_cuda, gs, same, cols, want, rid=k + 1)
    for test in (F.xis_iri, F.xis_blank, F.xis_literal, F.xis_numeric):
        x = test(c)
        check_three_valued(torch_cuda, gs, x, cols, [test(F.xenc(k)).fn(r) for r in zip(*[v.tolist() for v in cols])], rid=k + 1)


def test_coalesce_of_ids_truth_table(torch_cuda, gs):
    for k in sorted({len(ops) for ops, _ in F.COALESCE_ID_TRUTH}):
        cases = [(ops, want) for ops, want in F.COALESCE_ID_TRUTH if len(ops) == k]
        cols = [np.array([ops[q] for ops, _ in cases], np.uint32) for q in range(k)] + [np.array([w for _, w in cases], np.uint32),
                                                                                         np.arange(1, len(cases) + 1, dtype=np.uint32)]
        c = P.COALESCE(*[col(q) for q in range(k)])
        assert kept(torch_cuda, gs, P.ID_EQ(c, col(k)), cols, k + 1) == [i + 1 for i, (_, w) in enumerate(cases) if w]
        assert kept(torch_cuda, gs, P.NOT(P.BOUND(c)), cols, k + 1) == [i + 1 for i, (_, w) in enumerate(cases) if not w]


# ---------------------------------------------------------------------------------------------------
# 2. every op, alone and nested, in a FILTER: one lane, the wave edge, the workgroup-tile edge, a second sweep
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", F.ROW_COUNTS)
def test_ops_in_a_filter(torch_cuda, gs, reference, n):
    cols = F.id_columns(n)
    for name, x in F.filter_forms().items():
        try:
            check_three_valued(torch_cuda, gs, x, cols, reference[name][:n])
        except AssertionError as e:
            raise AssertionError(f"{name} over {n} rows") from e


def test_the_reference_separates_the_cases(reference):
    """every form is true somewhere, false somewhere and an error somewhere (IN of nothing: false everywhere)"""
    for name, want in reference.items():
        seen = {v if v[0] in (abi.TV_NULL, abi.TV_BOOLEAN) else "value" for v in want}
        if name == "in_0":
            assert seen == {F.tv_bool(False)}
        elif name == "lang_equals_fr":                                    # a tag no literal has: false, or an error
            assert seen == {F.tv_bool(False), F.NULL}
        elif name.endswith("_value"):
            assert "value" in seen, name
        else:
            assert {F.tv_bool(True), F.tv_bool(False), F.NULL} <= seen, (name, seen)


# ---------------------------------------------------------------------------------------------------
# 3. .. and wherever else a program runs
# ---------------------------------------------------------------------------------------------------
RIGHT = [np.array([1, 2, 1, 0], np.uint32), np.array([F.ID["integer7"], F.ID["str_en"], F.BEYOND, F.ID["iri2"]], np.uint32)]   # {key, w}


def join_tables(n):
    x, y, z, rid = F.id_columns(n)
    return [x, y, z, rid, (rid % 3).astype(np.uint32)], RIGHT            # the left key is 0 (null), 1 or 2


def pairs(forms, name, left, on_key):
    """[(rid, right row)] the reference lets through: forms over (left x, left y, right w)"""
    x = forms[name]
    out = []
    for l in zip(*[c.tolist() for c in left]):
        for q, r in enumerate(zip(*[c.tolist() for c in RIGHT])):
            if on_key and (l[4] == 0 or l[4] != r[0]):
                continue
            if x.fn(l + r) == F.tv_bool(True):
                out.append((l[3], q))
    return out


@pytest.mark.parametrize("kind,n", [(HASH, 1025), (NLJ, 257)])
def test_ops_in_join_filters(torch_cuda, gs, kind, n):
    left, right = join_tables(n)
    forms = F.filter_forms(0, 1, 6)                                       # x, y of the left; w of the right
    w_of = {int(w): q for q, w in enumerate(RIGHT[1])}
    for name, x in forms.items():
        want = pairs(forms, name, left, kind == HASH)
        for jt in (abi.JOIN_INNER, SEMI):
            pb = PlanBuilder()
            l, r = pb.table(0, 5), pb.table(1, 2)
            proj = [3, 6] if jt == abi.JOIN_INNER else [3]
            j = pb.hash_join(l, r, [(4, 0)], join_type=jt, filter=EBV(x.expr), projection=proj) if kind == HASH else \
                pb.nested_loop_join(l, r, jt, filter=EBV(x.expr), projection=proj)
            plan = execute(torch_cuda, gs, pb.build(j), [left, right])
            got = rows(plan)
            if jt == abi.JOIN_INNER:
                assert Counter((rid, w_of[w]) for rid, w in got) == Counter(want), (name, kind)
            else:
                assert sorted(r[0] for r in got) == sorted({rid for rid, _ in want}), (name, kind)


@pytest.mark.parametrize("n", [1, 1025, 4097])
def test_ops_in_computed_columns(torch_cuda, gs, reference, n):
    cols = F.id_columns(n)
    forms = F.value_forms()
    names = sorted(forms)
    for at in range(0, len(names), 8):                                    # (a ProjectionExec carries up to 8 expressions)
        part = names[at:at + 8]
        pb = PlanBuilder()
        x = pb.extend(pb.table(0, 4), [forms[k].expr for k in part], keep=[3])
        plan = execute(torch_cuda, gs, pb.build(x, agg_columns=True), [cols])
        assert rows(plan) and [r[0] for r in rows(plan)] == list(range(1, n + 1))
        for q, name in enumerate(part):
            assert records(plan, 1 + q) == [F.record(v) for v in reference[name][:n]], name


def test_sum_over_if_and_having_over_a_count(torch_cuda, gs, reference):
    n = 4097
    x, y, z, rid = F.id_columns(n)
    g = (rid % 7 + 1).astype(np.uint32)
    A = ENC_TV(col(0))
    one_if = P.COALESCE(P.IF(P.IS_NUMERIC(A), P.integer(1), P.integer(0)), P.integer(100))     # 1: numeric, 0: another term, 100: no term
    pb = PlanBuilder()
    a = pb.aggregate(pb.table(0, 5), [4], [(abi.AGG_SUM, one_if), (abi.AGG_COUNT_STAR, None), (abi.AGG_MIN, P.COALESCE(P.IF(P.IS_LITERAL(A), P.integer(3), P.integer(-3)), P.integer(-100)))])
    # HAVING: the COUNT read through ENC_TV, tested by IN, and chosen from by IF
    cnt = ENC_TV(col(2))
    counts = Counter(g.tolist())
    big = sorted(set(counts.values()))[-1]
    h = pb.sparql_having(a, EBV(P.IF(P.IN(cnt, [P.integer(big), P.integer(1)]), P.boolean(True), P.IS_IRI(cnt))))
    num = [v == F.tv_bool(True) for v in reference["is_numeric"][:n]]
    nul = [v == F.NULL for v in reference["is_numeric"][:n]]
    lit = [v for v in reference["is_literal"][:n]]
    want = {}
    for k in counts:
        members = [i for i in range(n) if g[i] == k]
        mn = [3 if lit[i] == F.tv_bool(True) else -3 if lit[i] == F.tv_bool(False) else -100 for i in members]
        want[k] = (sum(1 if num[i] else 100 if nul[i] else 0 for i in members), counts[k], min(mn))
    for node, groups in ((a, set(counts)), (h, {k for k, c in counts.items() if c == big})):
        plan = execute(torch_cuda, gs, pb.build(node, agg_columns=True), [[x, y, z, rid, g]])
        keys = [r[0] for r in rows(plan)]
        assert sorted(keys) == sorted(groups) and groups
        got = {k: (s[1], c[1], m[1]) for k, s, c, m in zip(keys, records(plan, 1), records(plan, 2), records(plan, 3))}
        assert got == {k: want[k] for k in groups}
        assert {s[0] for s in records(plan, 1)} == {abi.TV_INTEGER}


def test_a_refusal_in_the_branch_not_chosen_fails_the_execute(torch_cuda, gs):
    """Evaluation is eager: IF(true, 1, xsd:float("-nan")) computes the cast — a literal the device declines — and the execute fails, although
    the reference would answer 1; so does a plain CAST of a simple literal in a COALESCE operand that is never reached.  The plan is usable
    on the next table."""
    s = F.ID["str_minus_nan"]
    clean = [np.array([F.ID["integer7"], F.ID["f64"], 0], np.uint32), np.arange(1, 4, dtype=np.uint32)]
    dirty = [np.array([F.ID["integer7"], s, F.ID["f64"]], np.uint32), np.arange(1, 4, dtype=np.uint32)]
    A = ENC_TV(col(0))
    for e, text in ((P.IF(P.boolean(True), P.integer(1), P.CAST_LEX(A, abi.TV_FLOAT)), "CAST_LEX"),
                    (P.COALESCE(P.integer(1), P.CAST(A, abi.TV_DOUBLE)), "simple literal")):
        pb = PlanBuilder()
        desc = pb.build(pb.filter(pb.table(0, 2), EBV(P.EQ(e, P.integer(1))), projection=[1]))
        plan = gs.plan(desc)
        for cols in (dirty, clean, dirty, clean):
            k, p = table_on_device(torch_cuda, cols)
            plan.bind_table(0, p, 3)
            if cols is dirty:
                with pytest.raises(RdfGpuError) as err:
                    plan.execute()
                assert err.value.status == abi.ERR_UNSUPPORTED and text in str(err.value)
            else:
                assert sorted(r[0] for r in rows(plan.execute())) == [1, 2, 3]


PARENT_TYPED_FILTER_KERNELS = ["void rdfgpu::filter_kernel<2>"]      # what the parent commit reports for the plan below (measured there)


def test_a_typed_comparison_keeps_its_specialised_kernel(torch_cuda, gs):
    """EBV(GT(ENC_TV(col), lit)) reports what it reported before: the typed-comparison shape, not the VM; the same predicate beside a term
    test goes through the VM."""
    cols = F.id_columns(20_000)
    pb = PlanBuilder()
    t = pb.table(0, 4)
    gt = EBV(P.GT(ENC_TV(col(0)), P.integer(0)))
    plain = execute(torch_cuda, gs, pb.build(pb.filter(t, gt, projection=[3])), [cols], timing=True)
    names = [k[0] for k in plain.kernel_stats()]
    assert names == PARENT_TYPED_FILTER_KERNELS, names
    both = execute(torch_cuda, gs, pb.build(pb.filter(t, P.AND(gt, EBV(P.IS_NUMERIC(ENC_TV(col(0))))), projection=[3])), [cols], timing=True)
    assert [k[0] for k in both.kernel_stats()] == ["void rdfgpu::filter_kernel<0>"]      # (the VM's instantiations share one reported name)
    assert sorted(rows(both)) == sorted(rows(plain)) and rows(plain)


# ---------------------------------------------------------------------------------------------------
# 4. the LeftMark join
# ---------------------------------------------------------------------------------------------------
def mark_plan(kind, nl_cols, nr_cols, on, flt, proj=None, left=None):
    pb = PlanBuilder()
    l, r = pb.table(0, nl_cols), pb.table(1, nr_cols)
    if left is not None:
        l = left(pb, l)
    j = pb.hash_join(l, r, on, join_type=MARK, filter=flt, projection=proj) if kind == HASH else pb.nested_loop_join(l, r, MARK, filter=flt, projection=proj)
    return pb, j


def check_mark(torch, gs, kind, L, R, on, filt="none", options=None, expect_kernel=None, proj=None):
    """the join's rows are the left rows IN ORDER, each with its mark (entry 1 = false, 2 = true; never 0)"""
    flt, fn = F.mark_filters(len(L))[filt]
    pb, j = mark_plan(kind, len(L), len(R), on, flt, proj)
    plan = execute(torch, gs, pb.build(j, agg_columns=True), [L, R], options, timing=True)
    want = F.mark_join(L, R, on, fn)
    lrows = list(zip(*[c.tolist() for c in L]))
    full = [lrows[jx] + (2 if m else 1,) for jx, m in want]
    assert rows(plan) == [tuple(r[c] for c in (proj if proj is not None else range(len(L) + 1))) for r in full]
    mark_at = (proj if proj is not None else list(range(len(L) + 1))).index(len(L))
    assert plan.value_columns() == [mark_at]
    assert plan.column_values(mark_at) == [m for _, m in want]
    assert plan.result_values(mark_at)[1] == 2
    names = [k[0] for k in plan.kernel_stats()]
    if expect_kernel is not None:
        assert any(expect_kernel in k for k in names), (expect_kernel, names)
        assert not any("semi_join_kernel" in k or "semi_nested_kernel" in k for k in names), names
    return plan, want


LDS_DEFAULT, LDS_MAX = 1024, 8192     # the largest right input whose set is built in LDS: by default (RDFGPU_OPT_LDS_MAX_BUILD), at most (kSemiLdsMaxBuild)
HASH_FORMS = {   # name: (options, right rows, kernel)
    "empty": ({}, 0, None), "one": ({}, 1, "mark_join_kernel<0"),
    "lds_limit": ({}, LDS_DEFAULT, "mark_join_kernel<0"), "above_lds_limit": ({}, LDS_DEFAULT + 1, "mark_join_kernel<1"),
    "lds_hard_limit": ({"LDS_MAX_BUILD": 1 << 20}, LDS_MAX, "mark_join_kernel<0"), "above_lds_hard_limit": ({"LDS_MAX_BUILD": 1 << 20}, LDS_MAX + 1, "mark_join_kernel<1"),
    "hbm_forced": ({"NO_SEMI_LDS": 1}, 700, "mark_join_kernel<1"),
}


def keyed_tables(rng, nl, nr, n_ids=F.N_IDS + 4):
    """{key, a, b} x {key, w}: a few right rows per key (duplicates on both sides, nulls among them), the other columns ids of the typed table"""
    kd = max(8, nr // 4 + 2)
    L = F.rand_cols(rng, nl, 1, kd) + F.rand_cols(rng, nl, 2, n_ids)
    R = F.rand_cols(rng, nr, 1, kd, null_frac=0.05) + F.rand_cols(rng, nr, 1, n_ids)
    return L, R


@pytest.mark.parametrize("form", list(HASH_FORMS))
@pytest.mark.parametrize("filt", ["none", "id_pair", "vm"])
def test_mark_hash_forms(torch_cuda, gs, form, filt):
    options, nr, kernel = HASH_FORMS[form]
    rng = np.random.default_rng(len(form) * 7 + len(filt))
    for nl in (1, 1023, 1024, 1025, 2049):                               # kSemiTile = 1024
        L, R = keyed_tables(rng, nl, nr)
        _, want = check_mark(torch_cuda, gs, HASH, L, R, [(0, 0)], filt, options, kernel)
        assert nl == 1 or nr < 2 or {m for _, m in want} == {True, False}
    check_mark(torch_cuda, gs, HASH, L, R, [(0, 0)], filt, options, kernel, proj=[3, 1])


@pytest.mark.parametrize("n_keys", [1, 2, 4])
def test_mark_keys_and_null_keys(torch_cuda, gs, n_keys):
    rng = np.random.default_rng(n_keys)
    L, R = F.rand_cols(rng, 1025, 4, 6, null_frac=0.2), F.rand_cols(rng, 300, 4, 6, null_frac=0.2)      # null keys on both sides
    on = [(k, (k + 1) % 4) for k in range(n_keys)]
    for options, kernel in (({}, "mark_join_kernel<0"), ({"NO_SEMI_LDS": 1}, "mark_join_kernel<1")):
        for filt in ("none", "id_pair"):
            _, want = check_mark(torch_cuda, gs, HASH, L, R, on, filt, options, kernel)
            assert {m for _, m in want} == {True, False}


def test_mark_all_equal_right_keys(torch_cuda, gs):
    """3000 right rows of one key: without a filter the build keeps one entry per key (DEDUPE); with one every row is an entry"""
    rng = np.random.default_rng(3)
    L = F.rand_cols(rng, 1025, 3, 5)
    R = [np.full(3000, 2, np.uint32), rng.integers(1, 4, 3000).astype(np.uint32)]
    for options, kernel in (({"LDS_MAX_BUILD": 8192}, "mark_join_kernel<0"), ({"NO_SEMI_LDS": 1}, "mark_join_kernel<1")):
        for filt in ("none", "id_pair"):
            check_mark(torch_cuda, gs, HASH, L, R, [(0, 0)], filt, options, kernel)


@pytest.mark.parametrize("filt", ["id_pair", "vm"])
def test_mark_nested_form(torch_cuda, gs, filt):
    rng = np.random.default_rng(11 + len(filt))
    n_ids = F.N_IDS + 4
    sizes = [(nl, nr) for nr in (255, 256, 257) for nl in (255, 256, 257, 513)]      # kNljTile = 256, the workgroup's 256 left rows
    for nl, nr in sizes if filt == "id_pair" else [(257, 257), (513, 255), (255, 256)]:
        L, R = F.rand_cols(rng, nl, 3, n_ids), F.rand_cols(rng, nr, 2, n_ids)
        R[1][: nr - 3] = 0                                               # only the last right rows can pass: every tile is walked
        _, want = check_mark(torch_cuda, gs, NLJ, L, R, [], filt, None, "mark_nested_kernel")
        assert {m for _, m in want} == {True, False}
    # a filter no pair passes: every lane walks every tile of right rows
    pb, j = mark_plan(NLJ, 3, 2, [], P.AND(P.ID_EQ(col(0), col(3)), P.NOT(P.BOUND(col(0)))))
    plan = execute(torch_cuda, gs, pb.build(j, agg_columns=True), [L, R])
    assert plan.column_values(3) == [False] * len(L[0])


def test_mark_shortcuts_without_a_join_kernel(torch_cuda, gs):
    rng = np.random.default_rng(4)
    L, R = F.rand_cols(rng, 1025, 3, 9), F.rand_cols(rng, 40, 2, 9)
    Z = [c[:0] for c in R]
    for kind, on in ((HASH, [(0, 0)]), (NLJ, [])):
        plan, want = check_mark(torch_cuda, gs, kind, L, Z, on, "id_pair")                     # an empty right input: all false
        assert not any(m for _, m in want) and not any("mark_" in k[0] for k in plan.kernel_stats())
        check_mark(torch_cuda, gs, kind, L, Z, on, "none", proj=[3, 0])
        check_mark(torch_cuda, gs, kind, [c[:0] for c in L], R, on, "none")                    # an empty left input: no rows
    plan, want = check_mark(torch_cuda, gs, NLJ, L, R, [], "none")                             # no keys, no filter, a right row: all true
    assert all(m for _, m in want) and not any("mark_" in k[0] for k in plan.kernel_stats())
    # .. but a right input counted on the device decides there
    for pred, mark in ((P.BOUND(col(0)), True), (P.AND(P.BOUND(col(0)), P.NOT(P.BOUND(col(0)))), False)):
        pb = PlanBuilder()
        j = pb.nested_loop_join(pb.table(0, 3), pb.filter(pb.table(1, 2), pred), MARK)
        plan = execute(torch_cuda, gs, pb.build(j, agg_columns=True), [L, [np.maximum(c, 1) for c in R]], timing=True)
        assert plan.column_values(3) == [mark] * 1025 and any("mark_nested_kernel" in k[0] for k in plan.kernel_stats())


def test_mark_left_input_counted_on_the_device(torch_cuda, gs):
    """the left input is a FilterExec: its count stays on the device, its columns have garbage beyond the live rows"""
    rng = np.random.default_rng(6)
    L, R = F.rand_cols(rng, 2049, 3, 40, null_frac=0.3), F.rand_cols(rng, 500, 2, 40)
    live = [c[L[1] != 0] for c in L]
    for kind, on, filt in ((HASH, [(0, 0)], "none"), (HASH, [(0, 0)], "vm"), (NLJ, [], "id_pair")):
        flt, fn = F.mark_filters(3)[filt]
        pb, j = mark_plan(kind, 3, 2, on, flt, left=lambda pb, l: pb.filter(l, P.BOUND(col(1))))
        plan = execute(torch_cuda, gs, pb.build(j, agg_columns=True), [L, R])
        want = F.mark_join(live, R, on, fn)
        assert len(want) == len(live[0]) < 2049
        got = rows(plan)
        assert Counter(got) == Counter(tuple(c[jx] for c in [x.tolist() for x in live]) + (2 if m else 1,) for jx, m in want)
        assert plan.metrics().output_rows == len(want)


def test_mark_read_by_the_operators_above(torch_cuda, gs):
    rng = np.random.default_rng(8)
    L, R = F.rand_cols(rng, 2049, 3, F.N_IDS + 4), F.rand_cols(rng, 300, 2, F.N_IDS + 4)
    L.append(np.arange(1, 2050, dtype=np.uint32))
    want = F.mark_join(L, R, [(0, 0)])
    marks = [m for _, m in want]
    tables = [L, R]

    def base(pb):
        return pb.sparql_exists_value(pb.table(0, 4, ["k", "a", "b", "rid"]), pb.table(1, 2, ["k", "w"]))
    # FILTER(?a is numeric || EXISTS {..}): the union of the semi join's rows and the other disjunct's
    other = F.xis_numeric(F.xenc(1))
    pb = PlanBuilder()
    f = pb.filter(base(pb), P.OR(EBV(other.expr), EBV(ENC_TV(col(4)))), projection=[3])
    got = sorted(r[0] for r in rows(execute(torch_cuda, gs, pb.build(f, agg_columns=True), tables)))
    pb2 = PlanBuilder()
    semi = pb2.sparql_exists(pb2.table(0, 4, ["k", "a", "b", "rid"]), pb2.table(1, 2, ["k", "w"]))
    semi_rids = {r[3] for r in rows(execute(torch_cuda, gs, pb2.build(semi), tables))}
    assert semi_rids == {L[3][jx] for jx, m in want if m}
    lrows = list(zip(*[c.tolist() for c in L]))
    other_rids = {r[3] for r in lrows if other.fn(r) == F.tv_bool(True)}
    assert got == sorted(semi_rids | other_rids) and semi_rids - other_rids and other_rids - semi_rids
    # NOT EXISTS as an operand
    pb = PlanBuilder()
    f = pb.filter(base(pb), P.NOT(EBV(ENC_TV(col(4)))), projection=[3])
    assert sorted(r[0] for r in rows(execute(torch_cuda, gs, pb.build(f, agg_columns=True), tables))) == sorted(set(L[3].tolist()) - semi_rids)
    # BIND(IF(EXISTS {..}, 1, -1))
    pb = PlanBuilder()
    x = pb.extend(base(pb), [P.IF(ENC_TV(col(4)), P.integer(1), P.integer(-1))], keep=[3, 4])
    plan = execute(torch_cuda, gs, pb.build(x, agg_columns=True), tables)
    assert [r[0] for r in rows(plan)] == L[3].tolist() and plan.column_values(1) == marks and plan.column_values(2) == [1 if m else -1 for m in marks]
    # SUM / COUNT / AVG grouped by a left column
    pb = PlanBuilder()
    true_ones = P.IF(ENC_TV(col(4)), P.integer(1), P.integer(0))
    a = pb.aggregate(base(pb), [1], [(abi.AGG_SUM, true_ones), (abi.AGG_COUNT, 4), (abi.AGG_COUNT_STAR, None), (abi.AGG_AVG, true_ones), (abi.AGG_SUM, 4)])
    plan = execute(torch_cuda, gs, pb.build(a, agg_columns=True), tables)
    per = {}
    for r, m in zip(lrows, marks):
        s = per.setdefault(r[1], [0, 0])
        s[0] += int(m); s[1] += 1
    from fractions import Fraction
    got = {k: (s, c, n, v) for (k,), s, c, n, v in zip([r[:1] for r in rows(plan)], *[plan.column_values(q) for q in (1, 2, 3, 4)])}
    assert {k: v[:3] for k, v in got.items()} == {k: (s, n, n) for k, (s, n) in per.items()}      # COUNT(mark) counts every row: a mark is never unbound
    for k, (s, n) in per.items():                                                   # (an xsd:decimal of 18 fraction digits, cut off)
        assert isinstance(got[k][3], Fraction) and 0 <= Fraction(s, n) - got[k][3] < Fraction(1, 10 ** 17), k
    assert len(set(plan.column_values(5))) == 1                                     # (SUM of the booleans themselves: no number among them, in any group)
    # grouped BY the mark (value keys), and sorted by it
    pb = PlanBuilder()
    a = pb.aggregate(base(pb), [4], [(abi.AGG_COUNT_STAR, None)])
    plan = execute(torch_cuda, gs, pb.build(a, agg_columns=True, value_keys=True), tables)
    assert sorted(zip(plan.column_values(0), plan.column_values(1))) == sorted(Counter(marks).items())
    pb = PlanBuilder()
    s = pb.sparql_order_by(base(pb), [(4, True), (3, False)])             # ORDER BY DESC(mark), rid
    plan = execute(torch_cuda, gs, pb.build(s, agg_columns=True), tables)
    assert [(r[3]) for r in rows(plan)] == [rid for m, rid in sorted(((not m), rid) for m, rid in zip(marks, L[3].tolist()))]
    assert plan.column_values(4) == sorted(marks, reverse=True)
    # the mark is no term
    pb = PlanBuilder()
    plan = execute(torch_cuda, gs, pb.build(base(pb), agg_columns=True), tables)
    with pytest.raises(RdfGpuError) as err:
        plan.decode_terms(4)
    assert err.value.status == abi.ERR_UNSUPPORTED and "mark" in str(err.value)


def test_one_mark_plan_over_tables_of_other_sizes(torch_cuda, gs):
    rng = np.random.default_rng(12)
    flt, fn = F.mark_filters(3)["id_pair"]
    pb, j = mark_plan(HASH, 3, 2, [(0, 0)], flt)
    plan = gs.plan(pb.build(j, agg_columns=True))
    for nl, nr in ((1025, 300), (10, 20_000), (3000, 1), (0, 5), (700, 0), (1025, 300)):
        L, R = F.rand_cols(rng, nl, 3, 50), F.rand_cols(rng, nr, 2, 50)
        kl, pl = table_on_device(torch_cuda, L)
        kr, pr = table_on_device(torch_cuda, R)
        plan.bind_table(0, pl, nl); plan.bind_table(1, pr, nr)
        plan.execute()
        want = F.mark_join(L, R, [(0, 0)], fn)
        assert rows(plan) == [tuple(c[jx] for c in [x.tolist() for x in L]) + (2 if m else 1,) for jx, m in want]
        assert plan.column_values(3) == [m for _, m in want]


# what the semi / anti joins of the inputs below report on the parent commit (its tests/test_gpu_negation.py helper `kernels`)
PARENT_SEMI_KERNELS = {
    ("lds", SEMI): ["void rdfgpu::semi_join_kernel<0, false"], ("lds", ANTI): ["void rdfgpu::semi_join_kernel<0, true"],
    ("hbm", SEMI): ["void rdfgpu::semi_build_kernel", "void rdfgpu::semi_join_kernel<1, false"],
    ("hbm", ANTI): ["void rdfgpu::semi_build_kernel", "void rdfgpu::semi_join_kernel<1, true"],
    ("nested", SEMI): ["void rdfgpu::semi_nested_kernel<false"], ("nested", ANTI): ["void rdfgpu::semi_nested_kernel<true"],
}
MARK_KERNELS = {"lds": ["void rdfgpu::mark_join_kernel<0"], "hbm": ["void rdfgpu::semi_build_kernel", "void rdfgpu::mark_join_kernel<1"],
                "nested": ["void rdfgpu::mark_nested_kernel"]}


def test_kernel_names_of_mark_semi_and_anti_nodes(torch_cuda, gs):
    rng = np.random.default_rng(2)
    L, R = F.rand_cols(rng, 8000, 3, 200), F.rand_cols(rng, 700, 2, 200, null_frac=0.05)
    for form, kind, options in (("lds", HASH, {}), ("hbm", HASH, {"NO_SEMI_LDS": 1}), ("nested", NLJ, {})):
        on = [(0, 0)] if kind == HASH else []
        flt = P.ID_NEQ(col(1), col(4))
        for jt in (SEMI, ANTI, MARK):
            pb = PlanBuilder()
            l, r = pb.table(0, 3), pb.table(1, 2)
            j = pb.hash_join(l, r, on, join_type=jt, filter=flt) if kind == HASH else pb.nested_loop_join(l, r, jt, filter=flt)
            plan = execute(torch_cuda, gs, pb.build(j, agg_columns=jt == MARK), [L, R], options, timing=True)
            names = [k[0] for k in plan.kernel_stats()]
            assert names == (MARK_KERNELS[form] if jt == MARK else PARENT_SEMI_KERNELS[(form, jt)]), (form, jt, names)


def test_mark_random_differential(torch_cuda, gs):
    rng = np.random.default_rng(20261021)
    options = [{}, {"NO_SEMI_LDS": 1}, {"LDS_MAX_BUILD": 64}, {"FORCE_GENERIC_VM": 1}]
    for case in range(200):
        n_ids = int(rng.integers(3, F.N_IDS + 8))
        nl, nr = int(rng.integers(0, 301)), int(rng.choice([0, 1, 5, 64, 65, 300]))
        L, R = F.rand_cols(rng, nl, 3, n_ids, rng.random() * 0.3), F.rand_cols(rng, nr, 2, n_ids, rng.random() * 0.3)
        kind = HASH if rng.random() < 0.7 else NLJ
        on = [[(0, 0)], [(0, 0), (1, 1)], [(2, 1), (0, 0)]][int(rng.integers(0, 3))] if kind == HASH else []
        filt = ["none", "id_pair", "vm"][int(rng.integers(0, 3))]
        proj = None if rng.random() < 0.5 else [int(c) for c in rng.permutation(4)[:int(rng.integers(1, 5))]]
        if proj is not None and 3 not in proj:
            proj.append(3)
        opts = options[int(rng.integers(0, len(options)))]
        try:
            check_mark(torch_cuda, gs, kind, L, R, on, filt, opts, proj=proj)
        except AssertionError as e:
            raise AssertionError(f"case {case}: kind={kind} nl={nl} nr={nr} on={on} filt={filt} proj={proj} opts={opts}") from e
