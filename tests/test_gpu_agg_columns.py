"""Aggregate values as columns (abi.PLAN_AGG_COLUMNS) on the MI355X: HAVING, joins of aggregates, a cross join with a global aggregate,
aggregates over aggregates, semi / anti joins, error values, every value kind, a shared aggregate, re-execution and the result export —
each against the Python reference of aggcol_cases.py — and what stays refused."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rdf_fusion_amd import abi
from rdf_fusion_amd.engine import RdfGpuError, AGG_DTYPE, agg_value
from rdf_fusion_amd.plan import (PlanBuilder, quad_pattern, col, lit_id, integer, decimal, EBV, GT, GEQ, LT, MUL, ADD, AND, NOT, BOUND,
                                 ENC_TV, ID_EQ, ID_NEQ, IS_COMPATIBLE, STR, STRLEN)
from test_gpu_parity import both_stores, table_on_device
import agg_cases as ac
import aggcol_cases as cc
from aggcol_cases import STAR, COUNT, DISTINCT, SUM, AVG, UNBOUND, E18, compare, tv

EMPTY = (np.zeros(0, np.uint32),) * 4
INNER, LEFT, SEMI, ANTI = abi.JOIN_INNER, abi.JOIN_LEFT, abi.JOIN_LEFT_SEMI, abi.JOIN_LEFT_ANTI
INTEGER, DEC = abi.TV_INTEGER, abi.TV_DECIMAL


@pytest.fixture(scope="module")
def gs(torch_cuda):
    return both_stores(EMPTY, typed=ac.TV, decimals=ac.DECIMALS)[0]


def run(torch, gs, tables, root_of, option=None, timing=False, agg_columns=True):
    """the plan `root_of(pb, [table nodes])` over bound tables, executed"""
    pb = PlanBuilder()
    nodes = [pb.table(slot, len(cols)) for slot, cols in enumerate(tables)]
    plan = gs.plan(pb.build(root_of(pb, nodes), agg_columns=agg_columns))
    if option:
        plan.set_option(option)
    if timing:
        plan.enable_kernel_timing(True)
    bind(torch, plan, tables)
    return plan.execute()


def bind(torch, plan, tables):
    plan._keep_cols = []
    for slot, cols in enumerate(tables):
        keep, ptrs = table_on_device(torch, cols)
        plan._keep_cols.append(keep)
        plan.bind_table(slot, ptrs, len(cols[0]))


def kernels(plan):
    return [s[0] for s in plan.kernel_stats()]


# ---------------------------------------------------------------------------------------------------
# HAVING
# ---------------------------------------------------------------------------------------------------
PRODUCT = lambda r: cc.mul(tv(r[1]), tv(r[2]))          # the reference's SUM(x * y) input
HAVING = {
    "count": (lambda: EBV(GT(ENC_TV(col(1)), integer(3))), lambda r: compare("gt", r[1], (INTEGER, 3))),
    "sum": (lambda: EBV(GEQ(ENC_TV(col(2)), decimal(1500 * E18))), lambda r: compare("geq", r[2], (DEC, 1500 * E18))),
    "both": (lambda: AND(EBV(GT(ENC_TV(col(1)), integer(1))), EBV(GEQ(ENC_TV(col(2)), decimal(700 * E18)))),
             lambda r: compare("gt", r[1], (INTEGER, 1)) and compare("geq", r[2], (DEC, 700 * E18))),
}


@pytest.mark.parametrize("which", list(HAVING))
def test_having_count_and_sum_of_products(torch_cuda, gs, which):
    """1. `COUNT(*) > k` and `SUM(x * y) >= d` over groups (BI Q3:17): the predicate runs in the generic VM"""
    expr, pred = HAVING[which]
    cols = cc.sized_groups(700)
    aggs = [(STAR, None), (SUM, MUL(ENC_TV(col(1)), ENC_TV(col(2))))]
    plan = run(torch_cuda, gs, [cols], lambda pb, t: pb.sparql_having(pb.aggregate(t[0], [0], aggs), expr()), timing=True)
    exp = cc.having(cc.aggregate(cc.rows_of(cols), [0], [(STAR, None), (SUM, PRODUCT)]), pred)
    assert 0 < len(exp) < 700
    cc.check_rows(exp, plan, [1, 2])
    names = kernels(plan)
    assert any(n.startswith("void rdfgpu::filter_kernel<0>") for n in names), names
    assert not any(n.startswith("void rdfgpu::filter_kernel<2>") or "filter_bits" in n for n in names), names


@pytest.mark.parametrize("groups", [1, 255, 256, 257])
def test_having_at_the_final_pass_block_edge(torch_cuda, gs, groups):
    """2. group counts around agg_final_kernel's 256-lane block: every group's entry and value, then the filter over them"""
    cols = cc.sized_groups(groups)
    aggs = [(STAR, None), (SUM, 1), (AVG, 2)]
    whole = run(torch_cuda, gs, [cols], lambda pb, t: pb.aggregate(t[0], [0], aggs))
    ref = cc.aggregate(cc.rows_of(cols), [0], aggs)
    cc.check_rows(ref, whole, [1, 2, 3])
    assert sorted(whole.fetch()[1].tolist()) == list(range(1, groups + 1))     # row g carries g + 1
    plan = run(torch_cuda, gs, [cols], lambda pb, t: pb.sparql_having(pb.aggregate(t[0], [0], aggs), EBV(GT(ENC_TV(col(1)), integer(2))), projection=[0, 3]))
    cc.check_rows(cc.having(ref, lambda r: compare("gt", r[1], (INTEGER, 2)), [0, 3]), plan, [1])


@pytest.mark.parametrize("option", [None, "NO_AGG_LDS"])
@pytest.mark.parametrize("edge", range(len(ac.form_edges())))
def test_having_across_the_lds_hbm_switch(torch_cuda, gs, edge, option):
    """3. the group counts on either side of the LDS / HBM switch of the accumulate pass, with and without NO_AGG_LDS"""
    aggs, fit, over = ac.form_edges()[edge]
    for groups in (fit, over):
        cols = ac.form_table(groups)
        whole = cc.aggregate(cc.rows_of(cols), [0], aggs)
        # the threshold is the reference's own median of the first aggregate (COUNT(*) = 3 everywhere, or a SUM over the limb set)
        mid = sorted(cc.exact(r[1]) for r in whole)[len(whole) // 2]
        plan = run(torch_cuda, gs, [cols], lambda pb, t: pb.sparql_having(pb.aggregate(t[0], [0], aggs), EBV(GEQ(ENC_TV(col(1)), decimal(int(mid * E18))))), option, timing=True)
        ref = cc.having(whole, lambda r: compare("geq", r[1], (DEC, int(mid * E18))))
        assert len(ref) == len(whole) if aggs[0][0] == STAR else len(whole) // 3 < len(ref) < len(whole)
        cc.check_rows(ref, plan, list(range(1, 1 + len(aggs))))
        lds = option is None and groups == fit
        assert any(n.startswith(f"void rdfgpu::agg_accum_kernel<{'true' if lds else 'false'}>") for n in kernels(plan)), kernels(plan)


# ---------------------------------------------------------------------------------------------------
# joins of aggregates (Q3 / Q4 / Q8), cross join with a global aggregate (Q6)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("join_type", [INNER, LEFT])
@pytest.mark.parametrize("kind", ["hash", "nested"])
def test_two_aggregates_joined_on_their_key(torch_cuda, gs, join_type, kind):
    """4. SUM per key of one table against COUNT / AVG per key of another, the filter comparing the two sides' values; LEFT: a left group
    without a partner, or whose partner fails the filter, reads unbound on the right"""
    a = cc.sized_groups(400, seed=1)[:2]
    b = [c[: len(c) // 2] for c in cc.sized_groups(520, seed=2)[:2]]
    aggs_a, aggs_b = [(SUM, 1)], [(STAR, None), (AVG, 1)]
    filt = lambda: EBV(GT(ENC_TV(col(1)), MUL(ENC_TV(col(4)), ENC_TV(col(3)))))          # sum_a > avg_b * count_b
    pred = lambda r: compare("gt", r[1], cc.mul(tv(r[4]), tv(r[3])))

    def root(pb, t):
        l, r = pb.aggregate(t[0], [0], aggs_a), pb.aggregate(t[1], [0], aggs_b)
        if kind == "hash":
            return pb.hash_join(l, r, [(0, 0)], join_type=join_type, filter=filt(), projection=[0, 1, 3, 4])
        return pb.nested_loop_join(l, r, join_type=join_type, filter=AND(ID_EQ(col(0), col(2)), filt()), projection=[0, 1, 3, 4])
    plan = run(torch_cuda, gs, [a, b], root)
    la, rb = cc.aggregate(cc.rows_of(a), [0], aggs_a), cc.aggregate(cc.rows_of(b), [0], aggs_b)
    exp = cc.join(la, rb, [(0, 0)], join_type, pred, right_width=3)
    assert any(r[2] == 0 for r in exp) == (join_type == LEFT) and any(r[2] != 0 for r in exp)
    cc.check_rows([tuple(r[c] for c in (0, 1, 3, 4)) for r in exp], plan, [1, 2, 3])


Q6 = {
    # ..Business Intelligence - Q6 (Execution Plan).snap:6
    "avg > avg * 1.5": (lambda: EBV(GT(ENC_TV(col(1)), MUL(ENC_TV(col(2)), decimal(15 * E18 // 10)))),
                        lambda r: compare("gt", r[1], cc.mul(r[2], (DEC, 15 * E18 // 10)))),
    # the product on the per-reviewer side: an average with 18 fraction digits times 1.5 is the error value (Decimal::checked_mul), as
    # numeric_ref.binary says, and such a reviewer is dropped
    "avg * 1.5 < avg": (lambda: EBV(LT(MUL(ENC_TV(col(1)), decimal(15 * E18 // 10)), ENC_TV(col(2)))),
                        lambda r: compare("lt", cc.mul(r[1], (DEC, 15 * E18 // 10)), r[2])),
}


@pytest.mark.parametrize("which", list(Q6))
def test_cross_join_with_a_global_aggregate(torch_cuda, gs, which):
    """5. BI Q6: AVG per reviewer x the AVG over all (256 bound ratings: a terminating decimal), then the FilterExec over both.  Ratings
    hold unbound ids: such a reviewer's AVG is the error value, an unbound entry."""
    expr, pred = Q6[which]
    cols = cc.review_table()
    clean = [c[cols[1] != 0][:256] for c in cols]

    def root(pb, t):
        per, all_ = pb.aggregate(t[0], [0], [(AVG, 1)]), pb.aggregate(t[1], [], [(AVG, 1)])
        return pb.sparql_having(pb.cross_join(per, all_), expr())
    plan = run(torch_cuda, gs, [cols, clean], root)
    per, all_ = cc.aggregate(cc.rows_of(cols), [0], [(AVG, 1)]), cc.aggregate(cc.rows_of(clean), [], [(AVG, 1)])
    assert any(r[1] == UNBOUND for r in per) and all_[0][0][0] == DEC
    crossed = cc.join(per, all_, [])
    assert any(pred(r) is None and r[1] != UNBOUND for r in crossed) == (which == "avg * 1.5 < avg")
    exp = cc.having(crossed, pred)
    assert 0 < len(exp) < len(per) // 2
    cc.check_rows(exp, plan, [1, 2])


# ---------------------------------------------------------------------------------------------------
# aggregates over aggregates (Q5)
# ---------------------------------------------------------------------------------------------------
def test_aggregate_over_aggregate(torch_cuda, gs):
    """6. gby=[country] over gby=[country, product]: SUM of the per-pair COUNTs is COUNT(*) of the input, AVG of the decimal AVGs, COUNT
    of a value column, and an input expression over one; then the same with zero keys"""
    cols = cc.two_level_table()
    inner = [(STAR, None), (AVG, 2)]
    outer = [(SUM, 2), (AVG, 3), (COUNT, 3), (SUM, ADD(ENC_TV(col(2)), integer(1)))]
    ref_outer = [(SUM, 2), (AVG, 3), (COUNT, 3), (SUM, lambda r: (INTEGER, r[2][1] + 1))]
    ref_inner = cc.aggregate(cc.rows_of(cols), [0, 1], inner)
    for keys in ([0], []):
        plan = run(torch_cuda, gs, [cols], lambda pb, t: pb.aggregate(pb.aggregate(t[0], [0, 1], inner), keys, outer), timing=True)
        exp = cc.aggregate(ref_inner, keys, ref_outer)
        cc.check_rows(exp, plan, list(range(len(keys), len(keys) + 4)))
        assert any(n.startswith("void rdfgpu::agg_accum_expr_kernel") for n in kernels(plan)), kernels(plan)
        counts = dict(zip(*np.unique(cols[0], return_counts=True))) if keys else {(): len(cols[0])}
        for r in exp:                                                                  # the reference itself: SUM of COUNTs = COUNT(*)
            assert r[len(keys)] == (INTEGER, counts[r[0] if keys else ()])


# ---------------------------------------------------------------------------------------------------
# semi / anti joins
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("join_type", [SEMI, ANTI])
@pytest.mark.parametrize("kind", ["hash", "nested"])
def test_semi_and_anti_join_filter_reads_the_right_sides_value(torch_cuda, gs, join_type, kind):
    """7. left rows (key, threshold) kept / dropped by whether the key's SUM on the right exceeds the row's threshold"""
    rng = np.random.default_rng(17)
    right = cc.sized_groups(300, seed=4)[:2]
    left = [(rng.integers(0, 330, 900) * 3 + 1).astype(np.uint32), rng.integers(1, 120, 900).astype(np.uint32)]
    left[0][::50] = 0                                                             # null keys never match
    filt = lambda: EBV(GT(ENC_TV(col(3)), ENC_TV(col(1))))

    def root(pb, t):
        r = pb.aggregate(t[1], [0], [(SUM, 1)])
        if kind == "hash":
            return pb.hash_join(t[0], r, [(0, 0)], join_type=join_type, filter=filt())
        return pb.nested_loop_join(t[0], r, join_type=join_type, filter=AND(ID_EQ(col(0), col(2)), filt()))
    plan = run(torch_cuda, gs, [left, right], root)
    exp = cc.join(cc.rows_of(left), cc.aggregate(cc.rows_of(right), [0], [(SUM, 1)]), [(0, 0)], join_type, lambda r: compare("gt", r[3], tv(r[1])))
    assert 0 < len(exp) < 900
    cc.check_rows(exp, plan, [])


# ---------------------------------------------------------------------------------------------------
# error values, value kinds
# ---------------------------------------------------------------------------------------------------
def test_an_error_aggregate_is_an_unbound_binding(torch_cuda, gs):
    """8. a group whose integer SUM overflows i64: dropped by a comparison, BOUND is false, not counted by COUNT, makes an AVG above it
    the error value, exported as a null"""
    cols = cc.overflow_table()
    ref = cc.aggregate(cc.rows_of(cols), [0], [(SUM, 1)])
    bad = [r for r in ref if r[1] == UNBOUND]
    assert len(bad) == 8
    agg = lambda pb, t: pb.aggregate(t[0], [0], [(SUM, 1)])
    plan = run(torch_cuda, gs, [cols], lambda pb, t: pb.sparql_having(agg(pb, t), EBV(GT(ENC_TV(col(1)), integer(0)))))
    cc.check_rows([r for r in ref if r[1] != UNBOUND], plan, [1])
    plan = run(torch_cuda, gs, [cols], lambda pb, t: pb.filter(agg(pb, t), NOT(BOUND(col(1)))))
    cc.check_rows(bad, plan, [1])
    plan = run(torch_cuda, gs, [cols], lambda pb, t: pb.aggregate(agg(pb, t), [], [(COUNT, 1), (AVG, 1), (SUM, 1), (STAR, None)]))
    cc.check_rows(cc.aggregate(ref, [], [(COUNT, 1), (AVG, 1), (SUM, 1), (STAR, None)]), plan, [0, 1, 2, 3])
    assert plan.column_values(0) == [32] and plan.column_values(1) == [None] and plan.column_values(3) == [40]
    plan = run(torch_cuda, gs, [cols], agg)                                          # at the root: entry 0, the null value, an Arrow null
    keys, entries = plan.fetch()
    assert sorted(keys[entries == 0].tolist()) == sorted(r[0] for r in bad)
    batch = next(iter(plan.batches()))
    assert batch.field(1).null_count == 8 and batch.field(0).null_count == 0
    assert [v is None for v in plan.column_values(1)] == (entries == 0).tolist()


def test_every_value_kind_carried_to_the_root(torch_cuda, gs):
    """9. integer; decimal with a negative high word; float; double; the error value — through a filter and a projection"""
    cols = cc.kinds_table()
    aggs = [(SUM, 1), (AVG, 1)]
    plan = run(torch_cuda, gs, [cols], lambda pb, t: pb.filter(pb.aggregate(t[0], [0], aggs), NOT(ID_EQ(col(0), lit_id(45))), projection=[2, 0, 1]))
    ref = cc.having(cc.aggregate(cc.rows_of(cols), [0], aggs), lambda r: r[0] != 45, [2, 0, 1])
    assert {r[2][0] for r in ref} == {abi.TV_INTEGER, abi.TV_DECIMAL, abi.TV_FLOAT, abi.TV_DOUBLE, abi.TV_NULL}
    cc.check_rows(ref, plan, [0, 2])
    got = dict(zip(plan.fetch()[1].tolist(), plan.fetch_column_values(2)))
    assert got[17]["tag"] == abi.TV_DECIMAL and got[17]["hi"] < 0                     # SUM(-10^-18, -1.0, -1): a negative high word
    neg = dict(zip(plan.fetch()[1].tolist(), plan.column_values(0)))
    assert neg[10] > 0 and plan.column_values(2)[plan.fetch()[1].tolist().index(38)] is None


# ---------------------------------------------------------------------------------------------------
# a shared node, re-execution
# ---------------------------------------------------------------------------------------------------
def test_an_aggregate_consumed_by_two_parents(torch_cuda, gs):
    """10. the groups with a large count joined with the groups with a large sum — both filters read the same AggregateExec"""
    cols = cc.sized_groups(500, seed=9)

    def root(pb, t):
        a = pb.aggregate(t[0], [0], [(STAR, None), (SUM, 1)])
        return pb.hash_join(pb.filter(a, EBV(GT(ENC_TV(col(1)), integer(2)))), pb.filter(a, EBV(GT(ENC_TV(col(2)), integer(60)))), [(0, 0)],
                            filter=EBV(LT(ENC_TV(col(1)), ENC_TV(col(5)))), projection=[0, 1, 5])
    plan = run(torch_cuda, gs, [cols], root)
    a = cc.aggregate(cc.rows_of(cols), [0], [(STAR, None), (SUM, 1)])
    exp = cc.join(cc.having(a, lambda r: compare("gt", r[1], (INTEGER, 2))), cc.having(a, lambda r: compare("gt", r[2], (INTEGER, 60))), [(0, 0)],
                  pred=lambda r: compare("lt", r[1], r[5]))
    assert 0 < len(exp) < 500
    cc.check_rows([(r[0], r[1], r[5]) for r in exp], plan, [1, 2])


def test_reexecution_over_other_tables_and_after_a_mutation(torch_cuda):
    """11. one plan, executed over bound tables of other sizes (the value arrays move and change length) and over a store pattern before
    and after the store grows: a program that kept an earlier execution's array would read stale or foreign values"""
    gs = both_stores(EMPTY, typed=ac.TV, decimals=ac.DECIMALS)[0]
    aggs = [(STAR, None), (SUM, 1)]
    pred = lambda r: compare("gt", r[2], (INTEGER, 40))
    pb = PlanBuilder()
    plan = gs.plan(pb.build(pb.sparql_having(pb.aggregate(pb.table(0, 3), [0], aggs), EBV(GT(ENC_TV(col(2)), integer(40)))), agg_columns=True))
    for groups in (900, 3, 257, 2000, 40):
        cols = cc.sized_groups(groups, seed=groups)
        bind(torch_cuda, plan, [cols])
        plan.execute()
        cc.check_rows(cc.having(cc.aggregate(cc.rows_of(cols), [0], aggs), pred), plan, [1, 2])
    pb = PlanBuilder()
    src = pb.data_source(quad_pattern("s", 1500, "o"))
    plan = gs.plan(pb.build(pb.sparql_having(pb.aggregate(src, [0], [(STAR, None), (SUM, 1)]), EBV(GT(ENC_TV(col(2)), integer(40)))), agg_columns=True))
    quads = None
    for groups in (300, 450):
        s, o, _ = cc.sized_groups(groups, seed=77)
        s = s + 2000
        batch = (np.zeros(len(s), np.uint32), s.astype(np.uint32), np.full(len(s), 1500, np.uint32), o)
        quads = batch if quads is None else tuple(np.concatenate(p) for p in zip(quads, batch))
        gs.extend(*batch)
        plan.execute()
        uniq = sorted(set(zip(quads[1].tolist(), quads[3].tolist())))                  # the store is a set of quads
        cc.check_rows(cc.having(cc.aggregate(uniq, [0], aggs), pred), plan, [1, 2])


# ---------------------------------------------------------------------------------------------------
# result export
# ---------------------------------------------------------------------------------------------------
def device_array(gs, ptr, n):
    """`n` rdfgpu_agg_value at device address `ptr`, read by the library itself: the array bound as a one-column table of 6 n u32 words
    (a plan whose root is the bound table fetches it as it is)"""
    pb = PlanBuilder()
    reader = gs.plan(pb.build(pb.table(0, 1)))
    reader.bind_table(0, [ptr], 6 * n)
    return reader.execute().fetch()[0].view(AGG_DTYPE)


def test_column_values_result_values_and_arrow_agree(torch_cuda, gs):
    """12. at the root, after a filter: the device array indexed by the column's entries, the host gather, the Python values and the
    Arrow batches are one set of values; an id column has no array"""
    cols = cc.overflow_table(groups=700)
    aggs = [(AVG, 1), (SUM, 1)]
    plan = run(torch_cuda, gs, [cols], lambda pb, t: pb.filter(pb.aggregate(t[0], [0], aggs), NOT(ID_EQ(col(0), lit_id(51)))))
    n, c = plan.result_info()
    assert (n, c) == (699, 3) and plan.agg_count() == 0 and plan.value_columns() == [1, 2]
    assert plan.result_values(0) == (0, 0)
    ids = plan.fetch()
    arrow = [b for b in plan.batches()]
    assert sum(len(b) for b in arrow) == n
    for q in (1, 2):
        ptr, length = plan.result_values(q)
        assert ptr != 0 and length == 700                                              # the AggregateExec's groups, not the filter's rows
        arr = device_array(gs, ptr, length)
        host = plan.fetch_column_values(q)
        e = ids[q].astype(np.int64)
        assert e.max() <= length
        for f in ("tag", "lo", "hi"):
            assert np.array_equal(host[f], np.where(e == 0, 0, arr[f][np.maximum(e, 1) - 1]))
        assert plan.column_values(q) == [agg_value(int(v["tag"]), int(v["lo"]), int(v["hi"])) for v in host]
        tags = np.concatenate([b.field(q).field("tag").to_numpy(zero_copy_only=False) for b in arrow])
        los = np.concatenate([b.field(q).field("lo").to_numpy(zero_copy_only=False) for b in arrow])
        valid = np.concatenate([np.asarray(b.field(q).is_valid()) for b in arrow])
        assert np.array_equal(valid, e != 0) and np.array_equal(tags[valid], host["tag"][valid]) and np.array_equal(los[valid], host["lo"][valid])
    assert (ids[2] == 0).sum() == 140 and (ids[1] != 0).all()
    with pytest.raises(RdfGpuError) as err:
        plan.fetch_column_values(0)
    assert err.value.status == abi.ERR_INVALID


# ---------------------------------------------------------------------------------------------------
# opt-in, refusals
# ---------------------------------------------------------------------------------------------------
def compile_status(gs, root_of, agg_columns=True, tables=((0, 3), (1, 3))):
    pb = PlanBuilder()
    t = [pb.table(slot, w) for slot, w in tables]
    try:
        gs.plan(pb.build(root_of(pb, t), agg_columns=agg_columns))
    except RdfGpuError as e:
        return e.status, str(e)
    return abi.OK, ""


AGG = lambda pb, t, k=0: pb.aggregate(t[k], [0], [(STAR, None), (SUM, 1)])           # columns: key, COUNT(*), SUM


def test_without_the_flag_the_same_description_is_refused_as_today(torch_cuda, gs):
    """13. filter over, join over and an aggregate that is not the root: RDFGPU_ERR_UNSUPPORTED with today's texts"""
    for root in (lambda pb, t: pb.sparql_having(AGG(pb, t), EBV(GT(ENC_TV(col(1)), integer(3)))),
                 lambda pb, t: pb.hash_join(AGG(pb, t), t[1], [(0, 0)]),
                 lambda pb, t: pb.aggregate(AGG(pb, t), [0], [(SUM, 1)])):
        assert compile_status(gs, root)[0] == abi.OK
        status, text = compile_status(gs, root, agg_columns=False)
        assert status == abi.ERR_UNSUPPORTED and "must be the plan's root" in text, text
    assert compile_status(gs, lambda pb, t: AGG(pb, t), agg_columns=False)[0] == abi.OK   # the root form itself is untouched


REFUSALS = {
    "left join key": (lambda pb, t: pb.hash_join(AGG(pb, t), t[1], [(1, 0)]), "node 3", "column 1"),
    "right join key": (lambda pb, t: pb.hash_join(t[1], AGG(pb, t), [(0, 2)]), "node 3", "column 2"),
    "semi join key": (lambda pb, t: pb.hash_join(t[1], AGG(pb, t), [(0, 1)], join_type=SEMI), "node 3", "column 1"),
    "group key": (lambda pb, t: pb.aggregate(AGG(pb, t), [0, 2], [(STAR, None)]), "node 3", "column 2"),
    "group key of a distinct": (lambda pb, t: pb.aggregate(AGG(pb, t), [1]), "node 3", "column 1"),
    "count distinct input": (lambda pb, t: pb.aggregate(AGG(pb, t), [0], [(DISTINCT, 2)]), "node 3", "column 2"),
    "topk key": (lambda pb, t: pb.topk(AGG(pb, t), [(1, abi.SORT_BY_ID)], 5, projection=[0], tie_break=True), "node 3", "column 1"),
    "topk key by double": (lambda pb, t: pb.topk(AGG(pb, t), [(2, abi.SORT_BY_DOUBLE), (0, abi.SORT_BY_ID)], 5, projection=[0], tie_break=False), "node 3", "column 2"),
    "topk output": (lambda pb, t: pb.topk(AGG(pb, t), [(0, abi.SORT_BY_ID)], 5, projection=[0, 1], tie_break=False), "node 3", "column 1"),
    "topk group": (lambda pb, t: pb.topk(AGG(pb, t), [(0, abi.SORT_BY_ID)], 5, group=2, projection=[0], tie_break=False), "node 3", "column 2"),
    "closure input": (lambda pb, t: pb.closure(AGG(pb, t)), "node 3", "column 1"),
    "union left": (lambda pb, t: pb.union(AGG(pb, t), t[1]), "node 3", "column 1"),
    "union right": (lambda pb, t: pb.union(t[1], AGG(pb, t)), "node 3", "column 1"),
    "through a projection and a filter": (lambda pb, t: pb.hash_join(pb.filter(pb.projection(AGG(pb, t), [2, 0]), BOUND(col(0))), t[1], [(0, 0)]), "node 5", "column 0"),
    "through a join": (lambda pb, t: pb.aggregate(pb.hash_join(t[1], AGG(pb, t), [(0, 0)]), [5], [(STAR, None)]), "node 4", "column 5"),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals_under_the_flag(torch_cuda, gs, what):
    """14. whatever would compare a value column's entries as ids: RDFGPU_ERR_UNSUPPORTED, the text names node and column"""
    root, node, column = REFUSALS[what]
    status, text = compile_status(gs, root)
    assert status == abi.ERR_UNSUPPORTED and node + ":" in text and column in text and "value column" in text, text


KIND_ERRORS = {
    "ID_EQ": lambda: ID_EQ(col(1), lit_id(3)), "ID_NEQ": lambda: ID_NEQ(col(0), col(2)), "IS_COMPATIBLE": lambda: IS_COMPATIBLE(col(1), col(0)),
    "STR": lambda: EBV(GT(STRLEN(STR(col(2))), integer(1))),
}


@pytest.mark.parametrize("op", list(KIND_ERRORS))
def test_a_value_column_under_an_id_op_is_a_kind_error(torch_cuda, gs, op):
    if op == "STR":                                     # string functions want the store's lexical forms before anything is typed
        import rdf_fusion_amd as rf
        gs = rf.GpuQuadStore()
        gs.set_typed_values(ac.TV, ac.DECIMALS)
        gs.set_strings(np.zeros(len(ac.TV) + 1, np.uint64), b"")
    status, text = compile_status(gs, lambda pb, t: pb.filter(AGG(pb, t), KIND_ERRORS[op]()))
    assert status == abi.ERR_INVALID and "value column" in text, text
    status, _ = compile_status(gs, lambda pb, t: pb.filter(AGG(pb, t), ID_EQ(col(0), lit_id(3))))     # the key column is an id column
    assert status == abi.OK


def test_decode_terms_of_a_value_column_is_refused(torch_cuda, gs):
    cols = cc.kinds_table()
    plan = run(torch_cuda, gs, [cols], lambda pb, t: pb.aggregate(t[0], [0], [(SUM, 1)]))
    with pytest.raises(RdfGpuError) as err:
        plan.decode_terms(1)
    assert err.value.status == abi.ERR_UNSUPPORTED and "column 1" in str(err.value) and "node 1" in str(err.value)
