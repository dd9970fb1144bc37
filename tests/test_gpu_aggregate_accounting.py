"""What AggregateExec reports to kernel_stats on the MI355X: the launches, rows and compulsory bytes of each of its kernel classes, against
the formula written above exec_aggregate and in DESIGN §6 — not against the code.  With N = input rows and G = groups:

    agg_groups_kernel          1 launch, N rows, 4 * n_keys * N bytes (no launch with zero keys or an empty input)
    every agg_accum_* kernel   1 launch, N rows, N * (0 per COUNT(*), 4 per COUNT / COUNT DISTINCT, 20 per SUM / AVG / MIN / MAX)
    agg_minmax_refine_kernel   1 launch, N rows, 20 * N per MIN / MAX
    agg_final_kernel           1 launch, G * (4 * n_keys + 24 * n_aggs) bytes
    agg_value_cols_kernel      1 launch, G * 4 * n_aggs bytes

The accumulate classes are summed over every name that contains `agg_accum`, so which form (LDS / HBM) ran does not matter."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rdf_fusion_amd import abi
from rdf_fusion_amd.plan import PlanBuilder, col, integer, EBV, GT, DIV, ENC_TV
from test_gpu_parity import both_stores, table_on_device
import minmax_cases as mc

EMPTY = (np.zeros(0, np.uint32),) * 4
ROWS, GROUPS = 1000, 7
AGGS = [(abi.AGG_COUNT_STAR, None), (abi.AGG_COUNT, 2), (abi.AGG_COUNT_DISTINCT, 2), (abi.AGG_SUM, 2), (abi.AGG_AVG, 3), (abi.AGG_MAX, 2),
        (abi.AGG_MIN, DIV(ENC_TV(col(2)), ENC_TV(col(3))))]
ROW_BYTES = {abi.AGG_COUNT_STAR: 0, abi.AGG_COUNT: 4, abi.AGG_COUNT_DISTINCT: 4, abi.AGG_SUM: 20, abi.AGG_AVG: 20, abi.AGG_MAX: 20, abi.AGG_MIN: 20}


@pytest.fixture(scope="module")
def gs(torch_cuda):
    return both_stores(EMPTY, typed=mc.TV, decimals=mc.DECIMALS)[0]


def table():
    """(key a, key b, value, divisor): 1000 rows over 7 distinct key pairs; ids 1 .. 1000 are the xsd:integer of the same value"""
    rng = np.random.default_rng(18)
    pairs = np.asarray([(1, 1), (1, 2), (2, 1), (2, 2), (3, 1), (3, 3), (4, 9)], np.uint32)
    g = rng.integers(0, GROUPS, ROWS)
    g[:GROUPS] = np.arange(GROUPS)
    cols = [pairs[g, 0], pairs[g, 1], rng.integers(1, 1001, ROWS).astype(np.uint32), rng.integers(1, 50, ROWS).astype(np.uint32)]
    cols[2][::41] = 0                                                  # (unbound ids: COUNT skips them, nothing of the accounting does)
    return cols


def executed(torch, gs, root_of, cols, n_rows=None):
    pb = PlanBuilder()
    plan = gs.plan(pb.build(root_of(pb, pb.table(0, len(cols))), agg_columns=True))
    plan.enable_kernel_timing(True)
    plan._keep_cols, ptrs = table_on_device(torch, cols)
    plan.bind_table(0, ptrs, len(cols[0]) if n_rows is None else n_rows)
    return plan.execute()


def reported(plan):
    """{class: (launches, rows, bytes)} of the aggregate's kernels; the accumulate classes as one"""
    out = {}
    for name, launches, _, nbytes, rows in plan.kernel_stats():
        if "agg_" not in name:
            continue
        key = "accum" if "agg_accum" in name else name.split("rdfgpu::")[1].split("<")[0]
        had = out.get(key, (0, 0, 0))
        out[key] = (had[0] + launches, had[1] + rows, had[2] + nbytes)
    return out


def formula(n, g, n_keys, aggs, group_pass=True, row_passes=True):
    per_row = sum(ROW_BYTES[fn] for fn, _ in aggs)
    refine = sum(20 for fn, _ in aggs if fn in (abi.AGG_MIN, abi.AGG_MAX))
    want = {"agg_final_kernel": (1, 0, g * (4 * n_keys + 24 * len(aggs))), "agg_value_cols_kernel": (1, 0, g * 4 * len(aggs))}
    if group_pass:
        want["agg_groups_kernel"] = (1, n, 4 * n_keys * n)
    if row_passes:
        want["accum"] = (1, n, n * per_row)
        want["agg_minmax_refine_kernel"] = (1, n, n * refine)
    return want


def check(plan, want, groups):
    got = reported(plan)
    assert plan.result_info()[0] == groups
    assert got == want


def test_two_keys(torch_cuda, gs):
    cols = table()
    plan = executed(torch_cuda, gs, lambda pb, t: pb.aggregate(t, [0, 1], AGGS), cols)
    check(plan, formula(ROWS, GROUPS, 2, AGGS), GROUPS)


def test_zero_keys(torch_cuda, gs):
    cols = table()
    plan = executed(torch_cuda, gs, lambda pb, t: pb.aggregate(t, [], AGGS), cols)
    check(plan, formula(ROWS, 1, 0, AGGS, group_pass=False), 1)


def test_zero_keys_over_an_empty_table(torch_cuda, gs):
    cols = table()
    plan = executed(torch_cuda, gs, lambda pb, t: pb.aggregate(t, [], AGGS), cols, n_rows=0)
    check(plan, formula(0, 1, 0, AGGS, group_pass=False, row_passes=False), 1)


def test_above_a_filter_the_rows_are_the_rows_it_kept(torch_cuda, gs):
    cols = table()
    kept = int((cols[2] > 500).sum())                                  # (id 0, an unbound value, fails the comparison)
    assert 400 < kept < 600 and kept % 64 != 0
    live = [c[cols[2] > 500] for c in cols]
    groups = len({(a, b) for a, b in zip(live[0].tolist(), live[1].tolist())})
    assert groups == GROUPS
    plan = executed(torch_cuda, gs, lambda pb, t: pb.aggregate(pb.filter(t, EBV(GT(ENC_TV(col(2)), integer(500)))), [0, 1], AGGS), cols)
    check(plan, formula(kept, GROUPS, 2, AGGS), GROUPS)
