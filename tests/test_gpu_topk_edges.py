"""TopK on the device at its output order and its group-size edges (topk_cases.py): groups of 1, 2, 63, 64, 65, 127, 128, 129 and 1000 rows
on sparse group ids from 0 to 70000, limits from 1 to 1024 on either side of the wave width, duplicates, nulls in every key position,
four keys, every numeric kind under SORT_BY_DOUBLE, every projection form.  The device's rows, as a sequence, must be the rows of
topk_cases.reference (sorted(set(..))[:k] per group in Python; test_topk_order_cpu.py holds the oracle to the same).  Then TopK over an
input whose row count lives on the device, one plan re-executed over tables of other sizes, and the bounds exec_topk and the compile step
set: group ids below 2^24, limits 1 .. 1024."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi
import topk_cases as tc


@pytest.fixture(scope="module")
def store(torch_cuda):
    gs = rf.GpuQuadStore()
    gs.set_typed_values(tc.TV, tc.DECIMALS)
    return gs


def on_device(torch, cols):
    ts = [torch.from_numpy(np.ascontiguousarray(c, dtype=np.uint32).view(np.int32)).cuda() for c in cols]
    return ts, [t.data_ptr() for t in ts]


def check(plan, want, width, what):
    """one execution: the fetched rows, in their order, are `want`"""
    cols = plan.execute().fetch()
    n = plan.result_info()[0]
    assert len(cols) == width, (what, len(cols), width)
    got = np.stack(cols, 1)[:n] if width else np.zeros((n, 0), np.uint32)
    assert n == len(want), (what, n, len(want))
    np.testing.assert_array_equal(got, tc.as_matrix(want, width), err_msg=what)


@pytest.mark.parametrize("c", tc.CASES, ids=tc.CASE_IDS)
def test_device_rows_equal_reference_in_order(torch_cuda, store, c):
    keep, ptrs = on_device(torch_cuda, c.cols)
    plan = store.plan(tc.topk_plan(c))
    plan.bind_table(0, ptrs, len(c.cols[0]))
    for rep in range(2):                                             # the second execution reuses the first one's scratch
        check(plan, tc.expected(c), tc.out_width(c), f"{c.name} rep {rep}")
    plan.close()
    del keep


@pytest.mark.parametrize("name", ["ladder-k5-grouped", "ladder-k64-one-group", "nulls-under-double"])
def test_row_count_known_on_the_device_only(torch_cuda, store, name):
    """TopK above a FilterExec: the table TopK reads has the capacity of the filter's input and a live row count on the device.  The filter
    keeps nothing (capacity > 0, no live row: no row out), then about one row in ten (the reference over the surviving rows)."""
    c = tc.case_named(name)
    table = tc.with_flag_column(c)
    keep, ptrs = on_device(torch_cuda, table)
    for flag_id in (tc.NEVER_ID, tc.KEEP_ID):
        live = tc.surviving(table, flag_id)
        want = tc.reference(live, c.keys, c.limit, c.group, c.projection, tc.TV, tc.DECIMALS)
        assert (len(live[0]) == 0) == (flag_id == tc.NEVER_ID) and (len(want) == 0) == (flag_id == tc.NEVER_ID)
        plan = store.plan(tc.filtered_topk_plan(c, flag_id))
        plan.bind_table(0, ptrs, len(table[0]))
        for rep in range(2):
            check(plan, want, tc.out_width(c), f"{name} flag {flag_id} rep {rep}")
        plan.close()
    del keep


def test_one_plan_over_tables_of_other_sizes(torch_cuda, store):
    """A small table (40 rows, groups 0 .. 3), then a larger one with more groups and a larger maximum group id (the ladder: 1586 rows,
    groups up to 70000), then the small one again: the scratch, the per-group counts and the output offsets of an earlier execution
    must not show in a later one."""
    big = tc.case_named("ladder-k5-grouped")
    small = tc.small_table()
    want_small = tc.reference(small, big.keys, big.limit, big.group, big.projection, tc.TV, tc.DECIMALS)
    assert 0 < len(want_small) < len(tc.expected(big)) and max(small[0]) < max(big.cols[0])
    keep_s, ptrs_s = on_device(torch_cuda, small)
    keep_b, ptrs_b = on_device(torch_cuda, big.cols)
    plan = store.plan(tc.topk_plan(big))
    for step, (ptrs, cols, want) in enumerate([(ptrs_s, small, want_small), (ptrs_b, big.cols, tc.expected(big)), (ptrs_s, small, want_small),
                                               (ptrs_b, big.cols, tc.expected(big))]):
        plan.bind_table(0, ptrs, len(cols[0]))
        check(plan, want, 3, f"step {step}")
    plan.close()
    del keep_s, keep_b


def test_group_id_bound(torch_cuda, store):
    """Group ids up to 2^24 - 1 run (three rows in groups 0, 5 and 2^24 - 1, limit 1); a group id of 2^24 fails the execute with
    ERR_UNSUPPORTED, and the same plan still answers for the table before."""
    pb_case = tc.Case("bound", tc.group_bound_table(tc.GROUP_ID_LIMIT - 1), tc.TERM_KEYS, 1, 0, None)
    want = tc.reference(pb_case.cols, pb_case.keys, 1, 0, None, tc.TV, tc.DECIMALS)
    assert [r[0] for r in want] == [0, 5, tc.GROUP_ID_LIMIT - 1]
    keep, ptrs = on_device(torch_cuda, pb_case.cols)
    plan = store.plan(tc.topk_plan(pb_case))
    plan.bind_table(0, ptrs, 3)
    check(plan, want, 3, "largest group id 2^24 - 1")
    over = tc.group_bound_table(tc.GROUP_ID_LIMIT)
    keep2, ptrs2 = on_device(torch_cuda, over)
    plan.bind_table(0, ptrs2, 3)
    with pytest.raises(rf.RdfGpuError) as e:
        plan.execute()
    assert e.value.status == abi.ERR_UNSUPPORTED, e.value
    plan.bind_table(0, ptrs, 3)
    check(plan, want, 3, "largest group id 2^24 - 1, after the refusal")
    plan.close()
    del keep, keep2


@pytest.mark.parametrize("limit", [0, tc.MAX_LIMIT + 1])
def test_limit_bounds_refused_at_compile(torch_cuda, store, limit):
    c = tc.case_named("duplicates-k5")
    with pytest.raises(rf.RdfGpuError) as e:
        store.plan(tc.topk_plan(c, limit=limit))
    assert e.value.status == abi.ERR_UNSUPPORTED, e.value
