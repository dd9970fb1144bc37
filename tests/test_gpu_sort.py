"""SortExec (abi.NODE_SORT) on the MI355X: the tile / run / pass edges of its three kernels, the fetch, the edge values of the sortable
encoding ascending and descending, the key forms, the plan shapes around the node, re-execution over tables of other sizes, the value
columns of its output and which kernels ran — the device's row sequence against sort_cases.reference, exactly.

Every table carries a last column r = input row + 1: the output's r column IS the permutation."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rdf_fusion_amd import abi
from rdf_fusion_amd.engine import RdfGpuError
from rdf_fusion_amd.plan import PlanBuilder, col, integer, EBV, GT, ENC_TV, MUL
from test_gpu_parity import both_stores, table_on_device
import extend_cases as ec
import numeric_ref as nr
import sort_cases as sc
from sort_cases import T, IDS, BY_ID, BY_TERM, BY_DOUBLE, BY_VALUE

EMPTY = (np.zeros(0, np.uint32),) * 4


@pytest.fixture(scope="module")
def gs(torch_cuda):
    return both_stores(EMPTY, typed=sc.TV, decimals=sc.DECIMALS)[0]


def bind(torch, plan, tables):
    plan._keep_cols = []
    for slot, cols in enumerate(tables):
        keep, ptrs = table_on_device(torch, cols)
        plan._keep_cols.append(keep)
        plan.bind_table(slot, ptrs, len(cols[0]))


def compiled(gs, n_cols, root_of):
    pb = PlanBuilder()
    nodes = [pb.table(slot, w) for slot, w in enumerate(n_cols)]
    return gs.plan(pb.build(root_of(pb, nodes), agg_columns=True))


def numbered(cols):
    """the columns and r = row + 1"""
    return list(cols) + [np.arange(1, len(cols[0]) + 1, dtype=np.uint32)]


def check_sequence(plan, cols, order):
    """the result is the rows `order` of `cols` (which end in r), in that order, column by column"""
    got = plan.fetch()
    assert plan.result_info()[0] == len(order)
    r = len(cols) - 1
    perm = (got[r].astype(np.int64) - 1).tolist()
    assert perm == order, [(i, g, w) for i, (g, w) in enumerate(zip(perm, order)) if g != w][:5]
    for c in range(r):
        assert np.array_equal(got[c], cols[c][np.asarray(order, np.int64)]), c


def sorted_values(pb, t, keys, value_cols, fetch=None):
    """SORT over `t` with ENC_TV of `value_cols` appended as value columns; a BY_VALUE key names the id column its value column is of"""
    e, at = sc.value_plan(pb, t, value_cols)
    return pb.sort(e, [(at[c] if how == BY_VALUE else c, how, desc) for c, how, desc in keys], fetch=fetch)


def run_sorted(torch, gs, cols, keys, fetch=None, timing=False):
    value_cols = sorted({c for c, how, _ in keys if how == BY_VALUE})
    root = (lambda pb, t: sorted_values(pb, t[0], keys, value_cols, fetch)) if value_cols else (lambda pb, t: pb.sort(t[0], keys, fetch=fetch))
    plan = compiled(gs, [len(cols)], root)
    if timing:
        plan.enable_kernel_timing(True)
    bind(torch, plan, [cols])
    return plan.execute()


WIDEST = [(0, BY_VALUE, True), (1, BY_ID, False), (2, BY_DOUBLE, True), (3, BY_TERM, False)]     # 4 + 1 + 1 + 1 words and the row: sc.MAX_WORDS


# ---------------------------------------------------------------------------------------------------
# sizes, fetch
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sc.SIZES)
def test_sizes_with_a_one_word_key(torch_cuda, gs, n):
    """n rows by one id key with few distinct values: the padded last tile, one run, an odd run count in a pass, a short final run;
    equal keys come out in input order"""
    cols = numbered(sc.id_table(n))
    plan = run_sorted(torch_cuda, gs, cols, [(0, BY_ID, False)])
    assert plan.result_info() == (n, 4)
    check_sequence(plan, cols, sc.reference(sc.rows_of(cols), [(0, BY_ID, False)]))


@pytest.mark.parametrize("n", sc.WIDE_SIZES)
def test_sizes_with_the_widest_record(torch_cuda, gs, n):
    """(value DESC, id ASC, BY_DOUBLE DESC, BY_TERM ASC): a record of 8 words, 64 KB of LDS per tile"""
    cols = numbered(sc.mixed_table(n))
    plan = run_sorted(torch_cuda, gs, cols, WIDEST)
    assert plan.result_info() == (n, 6) and plan.value_columns() == [5]
    check_sequence(plan, cols, sc.reference(sc.rows_of(cols), WIDEST))


@pytest.mark.parametrize("k", sc.FETCHES)
def test_fetch(torch_cuda, gs, k):
    """TopK(fetch=k) over 3T + 5 rows: every run is cut to k rows after the tile sort and after each pass"""
    cols = numbered(sc.id_table(sc.FETCH_N))
    keys = [(0, BY_ID, True), (1, BY_ID, False)]
    plan = run_sorted(torch_cuda, gs, cols, keys, fetch=k)
    assert plan.result_info()[0] == min(k, sc.FETCH_N)
    check_sequence(plan, cols, sc.reference(sc.rows_of(cols), keys, fetch=k))


# ---------------------------------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("desc", [False, True])
def test_value_edges(torch_cuda, gs, desc):
    """-0 / +0 / +-inf / NaN; 2 as INT, INTEGER, FLOAT, DOUBLE and DECIMAL; 2^53 and 2^53 + 1; negative integers; booleans before numerics;
    unbound first ascending and last descending — every value twice, so equal keys meet"""
    cols = numbered([sc.edge_ids()])
    plan = run_sorted(torch_cuda, gs, cols, [(0, BY_VALUE, desc)])
    order = sc.reference(sc.rows_of(cols), [(0, BY_VALUE, desc)])
    check_sequence(plan, cols, order)
    unbound = [i for i, x in enumerate(cols[0].tolist()) if x == 0]
    assert (order[:2] == unbound) if not desc else (order[-2:] == unbound)
    # the value column's entries still index the values: row + 1 of the EXTEND below, 0 for the unbound ones
    entries = plan.fetch()[2].tolist()
    assert entries == [0 if cols[0][r] == 0 else r + 1 for r in order]
    got = [nr.device_bits(int(v["tag"]), int(v["lo"]), int(v["hi"])) for v in plan.fetch_column_values(2)]
    assert got == [nr.bits(sc.val(int(cols[0][r]))) for r in order]


def test_all_equal_values_keep_input_order(torch_cuda, gs):
    n = T + 5
    cols = numbered([np.full(n, IDS["g1.5"], np.uint32)])
    for desc in (False, True):
        check_sequence(run_sorted(torch_cuda, gs, cols, [(0, BY_VALUE, desc)]), cols, list(range(n)))


# ---------------------------------------------------------------------------------------------------
# keys
# ---------------------------------------------------------------------------------------------------
KEYS = {
    "value DESC, id ASC": [(0, BY_VALUE, True), (1, BY_ID, False)],
    "id DESC": [(1, BY_ID, True)],
    "double DESC, term ASC": [(2, BY_DOUBLE, True), (3, BY_TERM, False)],
    "four keys": [(3, BY_TERM, True), (1, BY_ID, False), (2, BY_DOUBLE, False), (0, BY_ID, True)],
    "a column twice": [(1, BY_ID, False), (1, BY_ID, True), (0, BY_VALUE, False)],
}


@pytest.mark.parametrize("name", list(KEYS))
def test_keys(torch_cuda, gs, name):
    cols = numbered(sc.mixed_table(2 * T + 1))
    plan = run_sorted(torch_cuda, gs, cols, KEYS[name])
    check_sequence(plan, cols, sc.reference(sc.rows_of(cols), KEYS[name]))


def test_by_term_over_mixed_kinds_fails_the_execute(torch_cuda, gs):
    """a BY_TERM column that holds a number: refused like TopK's, and the plan stays usable"""
    plan = compiled(gs, [2], lambda pb, t: pb.sort(t[0], [(0, BY_TERM, False)]))
    bad = numbered([np.asarray([IDS["sB"], IDS["i1"], IDS["sA"]], np.uint32)])
    bind(torch_cuda, plan, [bad])
    with pytest.raises(RdfGpuError) as err:
        plan.execute()
    assert err.value.status == abi.ERR_UNSUPPORTED and "SORT_BY_TERM" in str(err.value), err.value
    good = numbered([np.asarray([IDS["sB"], IDS["iriA"], IDS["sA"]], np.uint32)])
    bind(torch_cuda, plan, [good])
    check_sequence(plan.execute(), good, [1, 2, 0])


# ---------------------------------------------------------------------------------------------------
# plan shapes
# ---------------------------------------------------------------------------------------------------
def test_q3_top_10_by_ratio(torch_cuda, gs):
    """BI Q3: the ratio of two counts, then SortExec: TopK(fetch=10), expr=[ratio DESC, product ASC]"""
    now, before = ec.q3_tables(300)
    plan = compiled(gs, [2, 2], lambda pb, t: pb.sparql_order_by(ec.q3_plan(pb, t[0], t[1]), [(3, True), (0, False)], limit=10))
    bind(torch_cuda, plan, [now, before])
    plan.execute()
    ref = ec.q3_reference(now, before)
    want = sorted(ref, key=lambda r: (sc.Desc(sc.sort_key(ec.raw(r[3]))), r[0]))[:10]
    assert plan.result_info() == (10, 4) and plan.value_columns() == [1, 2, 3]
    assert plan.fetch()[0].tolist() == [r[0] for r in want]
    got = [nr.device_bits(int(v["tag"]), int(v["lo"]), int(v["hi"])) for v in plan.fetch_column_values(3)]
    assert got == [nr.bits(ec.raw(r[3])) for r in want] and all(g[0] == abi.TV_FLOAT for g in got)      # the unbound ratios are last under DESC
    assert plan.column_values(1) == [r[1][1] for r in want]                                             # the counts came along


def test_sort_above_a_filter_counts_its_rows_on_the_device(torch_cuda, gs):
    """the FilterExec's row count is not read back: the sort's launches are sized by the capacity, its kernels stop at the live rows.
    r is the last key: the order does not depend on the order the filter leaves"""
    cols = numbered(sc.id_table(2 * T + 1))
    keys = [(0, BY_ID, True), (3, BY_ID, False)]
    plan = compiled(gs, [4], lambda pb, t: pb.sort(pb.filter(t[0], EBV(GT(ENC_TV(col(0)), integer(15)))), keys))
    bind(torch_cuda, plan, [cols])
    plan.execute()
    kept = [r for r in range(len(cols[0])) if cols[0][r] > 15]
    assert T < len(kept) < 2 * T and plan.metrics().exact_reruns == 0
    order = [kept[i] for i in sc.reference([sc.rows_of(cols)[r] for r in kept], keys)]
    check_sequence(plan, cols, order)
    few = compiled(gs, [4], lambda pb, t: pb.sort(pb.filter(t[0], EBV(GT(ENC_TV(col(0)), integer(39)))), keys, fetch=T + 1))   # fewer rows than the fetch
    bind(torch_cuda, few, [cols])
    kept = [r for r in range(len(cols[0])) if cols[0][r] > 39]
    assert 0 < len(kept) < T
    check_sequence(few.execute(), cols, [kept[i] for i in sc.reference([sc.rows_of(cols)[r] for r in kept], keys)])


def test_order_holds_under_extend_and_projection(torch_cuda, gs):
    cols = numbered(sc.id_table(T + 1))
    keys = [(1, BY_ID, False), (0, BY_ID, True)]

    def root(pb, t):
        e = pb.extend(pb.sort(t[0], keys), [MUL(ENC_TV(col(0)), ENC_TV(col(1)))])
        return pb.projection(e, [4, 3, 0])
    plan = compiled(gs, [4], root)
    bind(torch_cuda, plan, [cols])
    plan.execute()
    order = sc.reference(sc.rows_of(cols), keys)
    got = plan.fetch()
    assert (got[1].astype(np.int64) - 1).tolist() == order and got[2].tolist() == cols[0][order].tolist()
    assert got[0].tolist() == list(range(1, T + 2))                                                     # the EXTEND numbers the sorted rows
    assert plan.column_values(0) == [int(cols[0][r]) * int(cols[1][r]) for r in order]


def test_one_plan_over_tables_of_other_sizes(torch_cuda, gs):
    """compiled once, executed over tables that grow and shrink across a tile: nothing of an earlier execution shows"""
    keys = [(0, BY_ID, False), (1, BY_ID, True)]
    plan = compiled(gs, [4], lambda pb, t: pb.sort(t[0], keys, fetch=T + 2))
    for n in (T - 1, 2 * T + 1, 5, T + 1, 3 * T + 5, T):
        cols = numbered(sc.id_table(n, seed=11))
        bind(torch_cuda, plan, [cols])
        check_sequence(plan.execute(), cols, sc.reference(sc.rows_of(cols), keys, fetch=T + 2))


def test_value_columns_leave_through_fetch_and_the_arrow_stream(torch_cuda, gs):
    """a sorted value column through fetch_column_values and rdfgpu_plan_next: the struct child in its place, null where unbound"""
    cols = numbered(sc.mixed_table(T + 3))
    keys = [(0, BY_VALUE, False), (1, BY_ID, True)]
    plan = run_sorted(torch_cuda, gs, cols, keys, fetch=100)
    order = sc.reference(sc.rows_of(cols), keys, fetch=100)
    check_sequence(plan, cols, order)
    want = [nr.bits(sc.val(int(cols[0][r]))) for r in order]
    assert [nr.device_bits(int(v["tag"]), int(v["lo"]), int(v["hi"])) for v in plan.fetch_column_values(5)] == want
    ptr, length = plan.result_values(5)
    assert ptr != 0 and length == T + 3                                                                 # the values stayed where they were: the EXTEND's array
    arrow = list(plan.batches())
    assert sum(len(b) for b in arrow) == 100 and all(b.type.num_fields == 6 for b in arrow)
    child = [b.field(5) for b in arrow]
    valid = np.concatenate([np.asarray(c.is_valid()) for c in child])
    tags = np.concatenate([c.field("tag").to_numpy(zero_copy_only=False) for c in child])
    assert valid.tolist() == [w[0] != abi.TV_NULL for w in want] and not valid[0] and valid[-1]          # unbound first, ascending
    assert [int(t_) for t_ in tags[valid]] == [w[0] for w in want if w[0] != abi.TV_NULL]
    assert (np.concatenate([b.field(4).to_numpy(zero_copy_only=False) for b in arrow]).astype(np.int64) - 1).tolist() == order


def test_which_kernels_ran(torch_cuda, gs):
    """one launch each of the record, tile and gather kernels; no merge pass up to T rows, one at T + 1, three over six tiles"""
    for n, passes in ((T, 0), (T + 1, 1), (5 * T + 3, 3)):
        cols = numbered(sc.id_table(n))
        plan = run_sorted(torch_cuda, gs, cols, [(0, BY_ID, False)], timing=True)
        stats = {s[0]: s[1] for s in plan.kernel_stats() if s[0].startswith("rdfgpu::sort_")}
        want = {"rdfgpu::sort_keys_kernel": 1, "rdfgpu::sort_tile_kernel": 1, "rdfgpu::sort_gather_kernel": 1}
        if passes:
            want["rdfgpu::sort_merge_kernel"] = passes
        assert stats == want, (n, stats)
        assert plan.metrics().host_syncs == 1, plan.metrics().host_syncs                                 # the execute's own: none inside the node
