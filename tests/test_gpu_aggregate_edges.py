"""SUM / AVG on the device at the edges of their accumulators (agg_cases.py): totals on and one step past I64_MAX / I64_MIN / I128_MAX /
I128_MIN, limb sums far past 2^32, all-negative decimals, totals that fit only because the integer and the decimal part cancel; runs of
1 .. 257 equal neighbours starting at every lane; the group counts on either side of the LDS / HBM switch; the group pass with every
row a group of its own; a workgroup's second tile and second sweep; an input whose row count lives on the device.  Every expectation is
the restatement of test_aggregate_cpu.py (test_aggregate_edges_cpu.py holds the hand-written totals to it) or numpy; integer and decimal
results are compared exactly, tag included, float results against the bound include/rdfgpu.h states."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi
import agg_cases as ac
from test_aggregate_cpu import same

ENGINE_TOGGLED = any(k.startswith(("RDFGPU_NO_", "RDFGPU_FORCE_")) for k in os.environ)   # a debugging toggle is set for the whole run
FORMS = [None, "NO_AGG_LDS"]
STAR, SUM, AVG = ac.STAR, ac.SUM, ac.AVG


@pytest.fixture(scope="module")
def store(torch_cuda):
    gs = rf.GpuQuadStore()
    gs.set_typed_values(ac.TV, ac.DECIMALS)
    return gs


def execute(torch, store, cols, desc, form):
    ts = [torch.from_numpy(np.ascontiguousarray(c, dtype=np.uint32).view(np.int32)).cuda() for c in cols]
    plan = store.plan(desc)
    if form:
        plan.set_option(form)
    plan.enable_kernel_timing(True)
    plan.bind_table(0, [t.data_ptr() for t in ts], len(cols[0]))
    plan.execute()
    plan._keep_cols = ts
    return plan


def device_groups(plan, n_aggs):
    n, nk = plan.result_info()
    keys = [k.tolist() for k in plan.fetch()]
    vals = [plan.fetch_aggregate(a) for a in range(n_aggs)]
    assert plan.agg_count() == n_aggs
    cells = [list(zip(v["tag"].tolist(), v["lo"].tolist(), v["hi"].tolist())) for v in vals]
    out = {}
    for r in range(n):
        key = tuple(keys[q][r] for q in range(nk))
        assert key not in out, f"group {key} appears twice"
        out[key] = [c[r] for c in cells]
    return out


def check_groups(exp, got, what):
    assert len(got) == len(exp) and set(got) == set(exp), (what, len(exp), len(got))
    for key, e in exp.items():
        for a, (ev, gv) in enumerate(zip(e, got[key])):
            assert same(ev, gv), (what, key, a, ev if not hasattr(ev[1], "terms") else (ev[0], ev[1].exact()), gv)


def accum_kernels(plan):
    return [s[0] for s in plan.kernel_stats() if "agg_accum" in s[0]]


def ran(plan, kernel, lds):
    return any(k.startswith("void rdfgpu::%s<%s>" % (kernel, "true" if lds else "false")) for k in accum_kernels(plan))


# ---------------------------------------------------------------------------------------------------
# 1. totals
# ---------------------------------------------------------------------------------------------------
TOTAL_AGGS = [(SUM, 1), (AVG, 1), (STAR, None)]


@functools.lru_cache(maxsize=None)
def totals_expected():
    """one group per total case, by the restatement; the same for every order of the rows"""
    return ac.expected(ac.totals_table("sorted"), [0], TOTAL_AGGS)


def check_totals(plan, what):
    got = device_groups(plan, 3)
    check_groups(totals_expected(), got, what)
    for g, c in enumerate(ac.TOTAL_CASES):                          # and the results as worked by hand, where they are exact
        for a, lit in enumerate((c.sum, c.avg)):
            if ac.literal_result(lit) is not None:
                assert same(ac.literal_result(lit), got[(g,)][a]), (what, c.name, a, lit, got[(g,)][a])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("order", ["sorted", "shuffled", "filtered"])
def test_totals(torch_cuda, store, order, form):
    """filtered: the aggregate reads a FilterExec's output - the capacity of the filter's input, a live row count on the device that is
    no multiple of 64, dropped rows among and after the live ones"""
    cols = ac.totals_table(order)
    plan = execute(torch_cuda, store, cols, ac.aggregate_plan(len(cols), [0], TOTAL_AGGS, filtered=order == "filtered"), form)
    check_totals(plan, f"{order} {form}")
    assert ran(plan, "agg_accum_kernel", lds=not form) or ENGINE_TOGGLED, accum_kernels(plan)


@pytest.mark.parametrize("form", FORMS)
def test_totals_through_an_expression(torch_cuda, store, form):
    """SUM / AVG over ADD(ENC_TV(value), 0): the same values out of the expression VM, the same results"""
    cols = ac.totals_table("shuffled")
    e = ac.expression_input(1)
    plan = execute(torch_cuda, store, cols, ac.aggregate_plan(2, [0], [(SUM, e), (AVG, e), (STAR, None)]), form)
    check_totals(plan, f"expression {form}")
    assert any("agg_accum_expr_kernel" in k for k in accum_kernels(plan)), accum_kernels(plan)
    assert ran(plan, "agg_accum_expr_kernel", lds=not form) or ENGINE_TOGGLED, accum_kernels(plan)


# ---------------------------------------------------------------------------------------------------
# 2. runs
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def run_case():
    cols = ac.run_table()
    return cols, ac.expected(cols, [0], ac.RUN_AGGS)


@pytest.mark.parametrize("form", FORMS)
def test_runs(torch_cuda, store, form):
    cols, exp = run_case()
    plan = execute(torch_cuda, store, cols, ac.aggregate_plan(4, [0], ac.RUN_AGGS), form)
    check_groups(exp, device_groups(plan, len(ac.RUN_AGGS)), f"runs {form}")


# ---------------------------------------------------------------------------------------------------
# 3. the LDS / HBM switch
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge", range(3), ids=["count", "count-sum", "sum-avg"])
def test_form_switch(torch_cuda, store, edge):
    aggs, fits, over = ac.form_edges()[edge]
    for groups in (fits, over):
        cols = ac.form_table(groups)
        plan = execute(torch_cuda, store, cols, ac.aggregate_plan(2, [0], aggs), None)
        check_groups(ac.expected(cols, [0], aggs), device_groups(plan, len(aggs)), f"{groups} groups")
        if not ENGINE_TOGGLED:
            assert ran(plan, "agg_accum_kernel", lds=groups == fits) and not ran(plan, "agg_accum_kernel", lds=groups != fits), (groups, accum_kernels(plan))


# ---------------------------------------------------------------------------------------------------
# 4. the group pass
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_keys", ac.GROUP_KEYS)
@pytest.mark.parametrize("rows", ac.GROUP_ROWS)
def test_every_row_a_group(torch_cuda, store, rows, n_keys):
    cols = ac.distinct_tuples(rows, n_keys)
    keys, aggs = list(range(n_keys)), [(STAR, None), (SUM, n_keys)]
    plan = execute(torch_cuda, store, cols, ac.aggregate_plan(n_keys + 1, keys, aggs), None)
    got = device_groups(plan, 2)                                     # (no key twice)
    assert len(got) == rows
    check_groups(ac.expected(cols, keys, aggs), got, f"{rows} rows, {n_keys} keys")


# ---------------------------------------------------------------------------------------------------
# 5. strides
# ---------------------------------------------------------------------------------------------------
BIG_AGGS = [(STAR, None), (SUM, 1)]


@functools.lru_cache(maxsize=None)
def big_case(groups):
    key, value = ac.big_table(groups)
    uk, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    sums = np.bincount(inv, weights=value.astype(np.float64)).astype(np.int64)      # below 2^53: exact
    return key, value, uk, cnt, sums


@pytest.mark.parametrize("groups,form", [(ac.BIG_GROUPS, None), (ac.BIG_GROUPS, "NO_AGG_LDS"), (ac.BIG_GROUPS_LDS, None)])
def test_second_tile_and_later_sweeps(torch_cuda, store, groups, form):
    """2^24 + 1500 rows: workgroup 0 of the group pass takes tile 16384, a partial one, on its second trip, and the accumulate pass's
    sweeps after the first end in a partial one.  The words of 1000 groups are past LDS, so the default form is the HBM form there, as
    it is with NO_AGG_LDS; 600 groups run the same rows through the LDS form."""
    key, value, uk, cnt, sums = big_case(groups)
    assert len(uk) == groups and cnt.sum() == ac.BIG_ROWS
    plan = execute(torch_cuda, store, [key, value], ac.aggregate_plan(2, [0], BIG_AGGS), form)
    assert plan.result_info() == (len(uk), 1)
    gk = plan.fetch()[0]
    order = np.argsort(gk)
    assert np.array_equal(gk[order], uk)
    star, s = (plan.fetch_aggregate(a)[order] for a in range(2))
    assert (star["tag"] == abi.TV_INTEGER).all() and np.array_equal(star["lo"], cnt)
    assert (s["tag"] == abi.TV_INTEGER).all() and np.array_equal(s["lo"], sums)
    lds = not form and ac.n_words(BIG_AGGS) * groups * 8 <= ac.LDS_BYTES
    assert lds == (groups == ac.BIG_GROUPS_LDS)
    assert ran(plan, "agg_accum_kernel", lds=lds) or ENGINE_TOGGLED, accum_kernels(plan)


def test_second_sweep_of_the_lds_form(torch_cuda, store):
    """512 x 256 + 257 rows: the LDS form's workgroups 0 and 1 sweep a second time, the last of them over one row"""
    cols = ac.sweep_table()
    aggs = [(STAR, None), (SUM, 1), (AVG, 1)]
    plan = execute(torch_cuda, store, cols, ac.aggregate_plan(2, [0], aggs), None)
    check_groups(ac.expected(cols, [0], aggs), device_groups(plan, 3), "second sweep")
    assert ran(plan, "agg_accum_kernel", lds=True) or ENGINE_TOGGLED, accum_kernels(plan)
