"""FilterExec on the device at the tile and run edges of its streamed and run-copy forms (filter_cases.py): the six comparison operators
against literals of every numeric kind through each of the three places that spell the comparison out (filter_pred_value, stream_pred,
the nibble table of filter_bits_kernel<2>); the run copy over runs of 1 to 5 rows, absent ids, every output phase, chunk boundaries, no
survivor, one id, two ids per lane of its scan; both route thresholds at equality and one past it; verdict words of ids far apart; the
streamed form over bound tables at every start phase, output width, tile edge and survivor pattern, and over a FilterExec's output; the
single pass at 2^20 rows and more.  The device's rows are the rows of filter_cases.expected, in input order wherever the streamed or the
run-copy form ran (they promise it), as a multiset after a single pass.  Every case names the kernels that must have run."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import rdf_fusion_amd as rf
from rdf_fusion_amd.plan import PlanBuilder, col, lit_id, ENC_TV, EBV, BOUND, ID_EQ, ID_NEQ, REGEX, CONTAINS
from oracle import oracle as orc
import kat_util as ku
import filter_cases as fc

ENGINE_TOGGLED = any(k.startswith(("RDFGPU_NO_", "RDFGPU_FORCE_")) for k in os.environ)   # a debugging toggle is set for the whole run
BIG = fc.ROWS + 4097


def on_device(torch, cols):
    ts = [torch.from_numpy(np.ascontiguousarray(c, dtype=np.uint32).view(np.int32)).cuda() for c in cols]
    return ts, [t.data_ptr() for t in ts]


def assert_route(plan, must=(), must_not=()):
    """the kernels of the last execution: a route that is silently not taken fails the test"""
    if ENGINE_TOGGLED:
        return
    names = [st[0] for st in plan.kernel_stats()]
    for k in must:
        assert any(k in x for x in names), (k, names)
    for k in must_not:
        assert not any(k in x for x in names), (k, names)


def assert_rows(plan, exp, n_exp, width, what, ordered=True):
    got = plan.fetch()
    assert plan.result_info() == (n_exp, width), (what, plan.result_info(), n_exp, width)
    assert len(got) == len(exp) == width, what
    if ordered:
        for g, e in zip(got, exp):
            np.testing.assert_array_equal(g, e, err_msg=what)
    else:
        np.testing.assert_array_equal(ku.multiset(got, n_exp), ku.multiset(exp, n_exp), err_msg=what)


@pytest.fixture(scope="module")
def store(torch_cuda):
    """the typed table and no quads: the bound-table cases"""
    gs = rf.GpuQuadStore()
    gs.set_typed_values(fc.TV, fc.DECIMALS)
    yield gs
    gs.close()


def table_plan(gs, n_cols, predicate, projection):
    pb = PlanBuilder()
    return gs.plan(pb.build(pb.filter(pb.table(0, n_cols), predicate, projection=projection))).enable_kernel_timing(True)


# ---------------------------------------------------------------------------------------------------
# 1. operators, single pass
# ---------------------------------------------------------------------------------------------------
def test_operators_single_pass(torch_cuda, store):
    """filter_pred_value<2>: every id of the table (the null id and an id beyond it among them) in 4097 rows, six operators, every literal"""
    cols = fc.every_id_table(4097)
    keep, ptrs = on_device(torch_cuda, cols)
    for lit in fc.LITERALS:
        for op in fc.OPS:
            plan = table_plan(store, 2, fc.predicate(0, op, lit), [1])
            plan.bind_table(0, ptrs, len(cols[0]))
            plan.execute()
            exp, n_exp = fc.expected(cols, 0, op, lit, [1])
            assert_rows(plan, exp, n_exp, 1, f"{op} {lit.name}", ordered=False)
            assert_route(plan, must=["filter_kernel<2>"])
            plan.close()
    del keep


# ---------------------------------------------------------------------------------------------------
# store slices
# ---------------------------------------------------------------------------------------------------
class SliceStore:
    """one layout in a store of its own, and its rows in index order as the test computes them"""

    def __init__(self, layout):
        self.layout = layout
        self.gs = rf.GpuQuadStore()
        g, s, p, o = fc.store_quads(layout)
        assert self.gs.extend(g, s, p, o) == len(g)
        self.gs.set_typed_values(fc.TV, fc.DECIMALS)
        self.rows = fc.slice_rows(layout)

    def close(self):
        self.gs.close()


RUN_COPY = ["run_scan_kernel", "run_copy_kernel"]
STREAMED_KERNELS = ["filter_bits_kernel", "filter_write_kernel"]
ROUTES = {
    # name: (plan option, drop the slice's tables first, kernels that must run, kernels that must not)
    "searched": (None, True, ["value_runs_kernel"] + RUN_COPY, STREAMED_KERNELS),
    "cached": (None, False, RUN_COPY, ["value_runs_kernel"] + STREAMED_KERNELS),
    "no_table_cache": ("NO_TABLE_CACHE", False, ["value_runs_kernel"] + RUN_COPY, STREAMED_KERNELS),
    "verdict_bits": ("NO_RUN_COPY", False, ["value_verdict_kernel", "filter_bits_kernel<4>", "filter_write_kernel"], RUN_COPY + ["filter_bits_kernel<2>"]),
    "typed_bits": ("NO_VALUE_VERDICTS", False, ["filter_bits_kernel<2>", "filter_write_kernel"], RUN_COPY + ["value_verdict_kernel", "filter_bits_kernel<4>"]),
}


def run_slice(st, op, lit, projection, routes):
    """one filter over the slice by each of `routes`: the same rows in the same order"""
    exp, n_exp = fc.expected(st.rows, 1, op, lit, projection)
    desc = fc.slice_plan(op, lit, projection)
    for route in routes:
        option, drop, must, must_not = ROUTES[route]
        if route == "cached":                        # the plan that searched the runs, or any plan before it on this slice, left them
            plan = st.gs.plan(desc).enable_kernel_timing(True)
            plan.execute()
        else:
            if drop:
                st.gs.drop_tables()
            plan = st.gs.plan(desc).enable_kernel_timing(True)
            if option:
                plan.set_option(option)
        plan.execute()
        assert_rows(plan, exp, n_exp, len(projection), f"{st.layout.name} head {st.layout.head} {op} {lit.name} {projection} {route}")
        assert_route(plan, must, must_not)
        plan.close()
    return n_exp


@pytest.fixture(scope="module")
def store_a(torch_cuda):
    st = SliceStore(fc.long_runs(1))
    yield st
    st.close()


# ---------------------------------------------------------------------------------------------------
# 2. operators, every slice route
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lit_name", fc.A_KIND_LITERALS)
def test_operators_every_slice_route(store_a, lit_name):
    """layout A: six operators against one literal of each numeric kind, each equal to an id of the slice, three projections; the runs
    searched (value_runs_kernel), taken from the slice's table (the comparison inside run_scan_kernel), searched without a table, then the
    verdict bits and the typed bits: five routes, the same rows in the same order"""
    for op in fc.OPS:
        for projection in ([0], [0, 1], [1]):
            run_slice(store_a, op, fc.LIT[lit_name], projection, list(ROUTES))


def test_operators_integer_ends_and_no_or_every_survivor(store_a):
    """the integer literals at the ends of i64 and at 2^53 (waves of xsd:integer ids alone take the i64 path of filter_bits_kernel<2>, waves
    of other kinds leave every row undecided), then the literals that keep no row and every row"""
    for name in fc.A_MORE_INTEGERS:
        for op in fc.OPS:
            run_slice(store_a, op, fc.LIT[name], [0, 1], ["typed_bits", "cached", "verdict_bits"])
    kept = [run_slice(store_a, op, fc.LIT[name], [1, 0], list(ROUTES)) for op, name in fc.A_ENDS]
    assert kept == [0, fc.ROWS, 0]


# ---------------------------------------------------------------------------------------------------
# 3. run copy edges
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", fc.HEADS)
@pytest.mark.parametrize("name", ["short_runs", "span_1025", "one_run"])
def test_run_copy_edges(torch_cuda, name, head):
    """layouts B, C and F at every start phase of the slice: runs of 1 to 5 rows, absent ids, output runs that start at each phase of a
    16-byte group, end on a 4096-row chunk and cross one, no survivor, every survivor, one id, two ids per lane of the scan"""
    st = SliceStore(fc.LAYOUTS[name](head))
    try:
        for op, ln in fc.CASES[name]:
            for projection in ([1], [1, 0], [0, 1]):   # the sorted column alone: one id per run; then either output slot
                run_slice(st, op, fc.LIT[ln], projection, ["searched", "cached"])
        if name == "short_runs":                       # the same short runs, absent ids and NaNs through the verdict bits
            for op, ln in fc.CASES[name]:
                run_slice(st, op, fc.LIT[ln], [0, 1], ["verdict_bits", "typed_bits"])
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------------
# 4. thresholds: span * 1024 <= rows (run copy), span * 4 <= rows (verdict bits), at equality and one id past it
# ---------------------------------------------------------------------------------------------------
NOT_STREAMED_TYPED = ["filter_bits_kernel<2>"]
THRESHOLDS = {
    "span_1025": ("span_1025", False, RUN_COPY, STREAMED_KERNELS),
    "span_1025+1": ("span_1025", True, ["value_verdict_kernel", "filter_bits_kernel<4>", "filter_write_kernel"], RUN_COPY + NOT_STREAMED_TYPED),
    "wide_span": ("wide_span", False, ["value_verdict_kernel", "filter_bits_kernel<4>", "filter_write_kernel"], RUN_COPY + NOT_STREAMED_TYPED),
    "wide_span+1": ("wide_span", True, ["filter_bits_kernel<2>", "filter_write_kernel"], RUN_COPY + ["value_verdict_kernel", "filter_bits_kernel<4>"]),
}


@pytest.mark.parametrize("which", list(THRESHOLDS))
def test_route_thresholds(torch_cuda, which):
    """span * 1024 == rows: the run copy; one more id: the verdict bits.  span * 4 == rows: the verdict bits; one more id: the typed bits"""
    name, one_more, must, must_not = THRESHOLDS[which]
    layout = fc.LAYOUTS[name](2)
    st = SliceStore(fc.with_one_more_id(layout) if one_more else layout)
    try:
        for k, (op, ln) in enumerate(fc.CASES[name]):
            projection = ([0], [1, 0], [1])[k % 3]
            exp, n_exp = fc.expected(st.rows, 1, op, fc.LIT[ln], projection)
            plan = st.gs.plan(fc.slice_plan(op, fc.LIT[ln], projection)).enable_kernel_timing(True)
            for rep in range(2):
                plan.execute()
                assert_rows(plan, exp, n_exp, len(projection), f"{which} {op} {ln} {projection} rep {rep}")
                assert_route(plan, must, must_not)
            plan.close()
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------------
# 5. verdict words: ids of one 16-byte group in three or more words, a last ballot of 48 ids
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", fc.HEADS)
def test_verdict_words(torch_cuda, head):
    """layout D under NO_RUN_COPY: filter_bits_kernel<4> loads a verdict word of its own for an id between the ends of a 16-byte group;
    value_verdict_kernel's last ballot holds 48 ids and the last of them is kept under LT / LEQ"""
    st = SliceStore(fc.sparse_singles(head))
    try:
        for op, ln in fc.CASES["sparse_singles"]:
            for projection in ([0], [1, 0]):
                run_slice(st, op, fc.LIT[ln], projection, ["verdict_bits"])
    finally:
        st.close()


# ---------------------------------------------------------------------------------------------------
# 6. streamed over bound tables (unsorted ids)
# ---------------------------------------------------------------------------------------------------
STREAMED_NOT_SINGLE = ["filter_kernel<"]
SHAPE2_PAIRS = [("GT", "integer 5"), ("LT", "double 0.5"), ("GEQ", "integer 0"), ("LEQ", "decimal 1.0"), ("EQ", "float 0.75"), ("NEQ", "int 7")]
PROJECTIONS = ([], [1], [2, 1], [0])                  # count only (filter_write_kernel<0>), one column, two columns, the predicate column


def id_expected(cols, is_eq, lit, projection):
    v = cols[0]
    mask = (v != 0) & (lit != 0) & ((v == lit) == is_eq)             # the null id on either side: dropped
    return [cols[c][mask] for c in projection], int(mask.sum())


@pytest.mark.parametrize("n", [fc.ROWS, fc.ROWS + 1, fc.ROWS + 4095, fc.ROWS + 4097])
def test_streamed_over_bound_tables(torch_cuda, store, n):
    """shapes 1 and 2 streamed (filter_bits_kernel<1|2>, the scan, filter_write_kernel<0|1|2>) over n rows that start 0 to 3 words into a
    16-byte group: n a multiple of the 4096-row tile, one row more, one row short of a further tile, one row into it.  Then the survivor
    patterns: no row, every row, the first row alone, the last row alone, one whole tile between tiles that keep nothing."""
    table = fc.unsorted_table(n + 3)
    keep, ptrs = on_device(torch_cuda, table)
    for skip in (0, 1, 2, 3):                        # the columns start `skip` words into a 16-byte group, all of them alike
        cols = [c[skip:skip + n] for c in table]
        bound = [p + 4 * skip for p in ptrs]
        pattern = np.zeros(n + 3, np.uint32)
        pattern[skip:skip + n] = fc.pattern_column(n, skip)
        keep_p, ptr_p = on_device(torch_cuda, [pattern])
        pcols = [pattern[skip:skip + n], cols[1], cols[2]]
        pbound = [ptr_p[0] + 4 * skip, bound[1], bound[2]]
        runs = []
        for is_eq, lit in ((True, 7), (False, 7), (True, 0), (False, 0)):                      # shape 1; a null literal keeps nothing
            runs.append((cols, bound, (ID_EQ if is_eq else ID_NEQ)(col(0), lit_id(lit)), lambda p, e=is_eq, l=lit: id_expected(cols, e, l, p), "filter_bits_kernel<1>", None))
        for op, ln in SHAPE2_PAIRS:                                                             # shape 2
            runs.append((cols, bound, fc.predicate(0, op, fc.LIT[ln]), lambda p, o=op, l=ln: fc.expected(cols, 0, o, fc.LIT[l], p), "filter_bits_kernel<2>", None))
        P = fc.PATTERN_IDS                                                                      # survivor patterns
        for is_eq, lit, want in ((True, P["nowhere"], 0), (False, P["nowhere"], n), (True, P["first"], 1), (True, P["last"], 1), (True, P["tile"], fc.RUN_CHUNK)):
            runs.append((pcols, pbound, (ID_EQ if is_eq else ID_NEQ)(col(0), lit_id(lit)), lambda p, e=is_eq, l=lit: id_expected(pcols, e, l, p), "filter_bits_kernel<1>", want))
        for j, (_, ptrs_, pred, expect, kernel, want) in enumerate(runs):
            # two of the four output forms per case and start phase: over the four phases every case meets every form twice
            for projection in (PROJECTIONS[(j + skip) % 4], PROJECTIONS[(j + skip + 2) % 4]):
                plan = table_plan(store, 3, pred, projection)
                plan.bind_table(0, ptrs_, n)
                plan.execute()
                exp, n_exp = expect(projection)
                assert want is None or n_exp == want
                assert_rows(plan, exp, n_exp, len(projection), f"n {n} skip {skip} {kernel} case {j} {projection}")
                assert_route(plan, [kernel, "filter_write_kernel"], STREAMED_NOT_SINGLE)
                plan.close()
        # the one whole tile: its rows are the rows of tile 129 and no other
        exp, n_exp = id_expected(pcols, True, P["tile"], [1])
        first = 129 * fc.RUN_CHUNK - skip
        np.testing.assert_array_equal(exp[0], pcols[1][first:first + fc.RUN_CHUNK])
        del keep_p
    del keep


def test_streamed_string_verdicts(torch_cuda):
    """shape 3 streamed (filter_bits_kernel<3>): CONTAINS and REGEX per distinct term against Python's `in` / `re`, an id beyond the verdict
    table, and a row whose string needs the Unicode tables under \\d: a loud error, after which the plan still answers"""
    strings = ["", "a", "ab", "abc", "a.c", "xabcx", "cab", "b", "12", "x1", "no", "K", "abab", "zzz", "a c", "a\nc", "7", "abc 12", "café 12"]
    unicode_id = len(strings)
    tv, offsets, heap = ku.string_dictionary(strings)
    gs, os_ = rf.GpuQuadStore(), orc.OracleStore()
    for s_ in (gs, os_):
        s_.set_typed_values(tv)
        s_.set_strings(offsets, heap)
    n = BIG
    rng = np.random.default_rng(21)
    pool = np.array([i for i in range(len(tv) + 2) if i != unicode_id], np.uint32)          # the null id, the integers, two ids beyond the table
    table = [pool[rng.integers(0, len(pool), n + 3)], np.arange(1, n + 4, dtype=np.uint32), rng.integers(1, 1 << 30, n + 3).astype(np.uint32)]
    keep, ptrs = on_device(torch_cuda, table)
    with_unicode = [c.copy() for c in table]
    with_unicode[0][fc.ROWS + 5] = unicode_id
    keep_u, ptrs_u = on_device(torch_cuda, with_unicode)
    is_str = lambda i: 1 <= i <= len(strings)
    answers = [
        (EBV(CONTAINS(ENC_TV(col(0)), "ab")), lambda i: is_str(i) and "ab" in strings[i - 1]),
        (EBV(REGEX(ENC_TV(col(0)), "a.c", "")), lambda i: is_str(i) and re.search("a.c", strings[i - 1]) is not None),
        (EBV(REGEX(ENC_TV(col(0)), "\\d+", "")), lambda i: is_str(i) and re.search("\\d+", strings[i - 1], re.ASCII) is not None),
    ]
    try:
        for k, (pred, answer) in enumerate(answers):
            per_id = np.array([bool(answer(i)) for i in range(len(tv) + 2)])
            ids = np.asarray(pool)
            np.testing.assert_array_equal(os_.eval_bool(pred, [ids]) == 1, per_id[ids])     # Python's answer is the oracle's, per distinct id
            for skip in (0, 2):
                cols = [c[skip:skip + n] for c in table]
                mask = per_id[cols[0]]
                assert 0 < mask.sum() < n
                for projection in ([1], [2, 1], []):
                    plan = table_plan(gs, 3, pred, projection)
                    plan.bind_table(0, [p + 4 * skip for p in ptrs], n)
                    plan.execute()
                    assert_rows(plan, [cols[c][mask] for c in projection], int(mask.sum()), len(projection), f"strings {k} skip {skip} {projection}")
                    assert_route(plan, ["filter_bits_kernel<3>", "filter_write_kernel"], STREAMED_NOT_SINGLE)
                    if k == 2 and projection == [1]:
                        plan.bind_table(0, [p + 4 * skip for p in ptrs_u], n)
                        with pytest.raises(rf.RdfGpuError, match="Unicode"):
                            plan.execute()
                        plan.bind_table(0, [p + 4 * skip for p in ptrs], n)                # the plan stays usable after the refusal
                        plan.execute()
                        assert_rows(plan, [cols[1][mask]], int(mask.sum()), 1, f"strings after the refusal, skip {skip}")
                    plan.close()
    finally:
        gs.close()
    del keep, keep_u


# ---------------------------------------------------------------------------------------------------
# 7. streamed over a FilterExec: the row count on the device, garbage beyond the live rows
# ---------------------------------------------------------------------------------------------------
def test_streamed_over_a_filter(torch_cuda, store):
    """filter(filter(table, BOUND(flag)), typed comparison) over 2^20 + 4097 rows of which about half are live: the outer filter streams over
    a table whose row count is on the device and whose rows beyond it are whatever the scratch held; no exact rerun"""
    n = BIG
    ids, payload, _ = fc.unsorted_table(n)
    flag = (np.random.default_rng(8).integers(0, 2, n) * 9).astype(np.uint32)               # bound in about half of the rows
    cols = [ids, payload, flag]
    keep, ptrs = on_device(torch_cuda, cols)
    live = [c[flag != 0] for c in cols]
    assert 0.45 * n < len(live[0]) < 0.55 * n
    for op, ln in SHAPE2_PAIRS:
        for projection in ([1], [1, 0]):
            pb = PlanBuilder()
            inner = pb.filter(pb.table(0, 3), BOUND(col(2)))
            plan = store.plan(pb.build(pb.filter(inner, fc.predicate(0, op, fc.LIT[ln]), projection=projection))).enable_kernel_timing(True)
            plan.bind_table(0, ptrs, n)
            for rep in range(2):
                plan.execute()
                exp, n_exp = fc.expected(live, 0, op, fc.LIT[ln], projection)
                # (the inner filter is a single pass: its rows come in no promised order, so neither do these)
                assert_rows(plan, exp, n_exp, len(projection), f"over a filter {op} {ln} {projection} rep {rep}", ordered=False)
                assert_route(plan, ["filter_kernel<0>", "filter_bits_kernel<2>", "filter_write_kernel"], ["filter_kernel<2>"])
                assert plan.metrics().exact_reruns == 0
            plan.close()
    del keep


# ---------------------------------------------------------------------------------------------------
# 8. single pass at 2^20 rows and more: three output columns, or an output column in another phase than the predicate column
# ---------------------------------------------------------------------------------------------------
def assert_rows_by_row_number(plan, cols, mask, projection, what):
    """the rows of a single pass over a big table, in whatever order: column 1 of the input numbers its rows, so it says which input row
    an output row is; every surviving row once and no other is the multiset of filter_cases.expected (without sorting 10^6 rows)"""
    got = plan.fetch()
    n_exp = int(mask.sum())
    assert plan.result_info() == (n_exp, len(projection)), (what, plan.result_info(), n_exp)
    r = got[projection.index(1)].astype(np.int64) - int(cols[1][0])
    assert len(r) == n_exp and (n_exp == 0 or (r.min() >= 0 and r.max() < len(mask))), what
    assert mask[r].all() and (n_exp == 0 or np.bincount(r, minlength=len(mask)).max() == 1), what
    for g, c in zip(got, projection):
        np.testing.assert_array_equal(g, cols[c][r], err_msg=what)


def test_single_pass_over_a_big_table(torch_cuda, store):
    n = BIG
    table = fc.unsorted_table(n + 3)
    keep, ptrs = on_device(torch_cuda, table)
    phases = ((0, 1), (2, 0), (3, 2), (1, 3), (0, 2), (3, 0))         # (words the id column starts into its 16-byte group, the other columns)
    for (op, ln), (id_skip, pay_skip) in zip(SHAPE2_PAIRS, phases):
        cols = [c[:n] for c in table]
        plan = table_plan(store, 3, fc.predicate(0, op, fc.LIT[ln]), [1, 2, 0])
        plan.bind_table(0, ptrs, n)
        plan.execute()
        assert_rows_by_row_number(plan, cols, fc.keep_mask(cols[0], op, fc.LIT[ln]), [1, 2, 0], f"three columns {op} {ln}")
        assert_route(plan, ["filter_kernel<2>"], STREAMED_KERNELS)
        plan.close()
        cols = [table[0][id_skip:id_skip + n], table[1][pay_skip:pay_skip + n], table[2][pay_skip:pay_skip + n]]
        mask = fc.keep_mask(cols[0], op, fc.LIT[ln])
        assert 0 < mask.sum() < n
        for projection in ([1], [0, 1]):
            plan = table_plan(store, 3, fc.predicate(0, op, fc.LIT[ln]), projection)
            plan.bind_table(0, [ptrs[0] + 4 * id_skip, ptrs[1] + 4 * pay_skip, ptrs[2] + 4 * pay_skip], n)
            plan.execute()
            assert_rows_by_row_number(plan, cols, mask, projection, f"phases {id_skip} {pay_skip} {op} {ln} {projection}")
            assert_route(plan, ["filter_kernel<2>"], STREAMED_KERNELS)
            plan.close()
    del keep
