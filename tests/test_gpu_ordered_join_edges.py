"""The ordered slice join (ordered_join.hip) at its tile, chain and record edges (ordered_cases.py): slices of 1025 .. 3072 rows around the
1024-row tile, chains of 254 .. 300 table rows on one key at the rows where tiles and rounds begin and end, tiles without a match and with
one match at either end, tile totals around the 256 lanes, 0 .. 3 look-up stages, 1 .. 9 output columns with 0 .. 8 words of the packed
record.  The device's rows must be reference()'s - in the slice's order, each slice row repeated by its chain - on the ordered form, and
the same multiset without it (test_ordered_join_cpu.py holds the oracle to the same reference).

When the form runs (run_ordered_join, plan_join.cpp): on a re-execution of a plan whose previous output had at least slice rows / 8 rows,
with at most 8 output columns.  Runner keeps that previous row count and asserts the kernels exactly where the rule says they must run."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import rdf_fusion_amd as rf
import band_cases as bc
import ordered_cases as oc
import kat_util as ku

ENGINE_TOGGLED = any(k.startswith(("RDFGPU_NO_", "RDFGPU_FORCE_")) for k in os.environ)   # a debugging toggle is set for the whole run
OJ_KERNELS = ("oj_probe_kernel", "oj_count_kernel", "oj_write_kernel")
IN_PLACE = "OjInPlace"

_STORES, _REFS = {}, {}


def device_store(n):
    if n not in _STORES:
        _STORES[n] = rf.GpuQuadStore()
        _STORES[n].extend(*oc.quads(n))
    return _STORES[n]


def on_device(torch, cols):
    """(an empty table still gets columns to point at)"""
    ts = [torch.from_numpy(np.ascontiguousarray(c if len(c) else np.zeros(1), dtype=np.uint32).view(np.int32)).cuda() for c in cols]
    return ts, [t.data_ptr() for t in ts]


def ran_ordered(names):
    return all(any(k in name for name in names) for k in OJ_KERNELS)


def no_ordered(names):
    return not any("oj_" in name for name in names)


def reference(n, name, tab, n_stages, proj):
    """computed once per named table, shared and left unchanged"""
    key = (n, name, n_stages, proj)
    if key not in _REFS:
        _REFS[key] = oc.reference(n, tab, n_stages, proj)
    return _REFS[key]


class Runner:
    """One plan over the store with a link slice of n rows, executed over one table after another."""
    def __init__(self, torch, n, n_stages, proj, flagged=False, options=()):
        self.torch, self.n, self.n_stages, self.proj, self.options = torch, n, n_stages, tuple(proj), tuple(options)
        self.plan = device_store(n).plan(oc.ordered_plan(n_stages, self.proj, flagged)).enable_kernel_timing(True)
        for o in options:
            self.plan.set_option(o, 1)
        self.prev = None                                            # rows of the previous execution: what the plan's history holds
        self.what = f"{n} rows, {n_stages} stages, {'+'.join(self.proj)}{' ' + '+'.join(options) if options else ''}"

    def run(self, tab, name):
        """-> (kernel names, metrics, the ordered form ran).  The rows are the reference's: in the slice's order when the form ran."""
        what = f"{self.what}: {name}"
        keep, ptrs = on_device(self.torch, tab)
        self.plan.bind_table(0, ptrs, len(tab[0]))
        got = self.plan.execute().fetch()
        del keep
        want = reference(self.n, name, tab, self.n_stages, self.proj)
        assert self.plan.result_info()[0] == len(want), (what, self.plan.result_info()[0], len(want))
        names, m = {k[0] for k in self.plan.kernel_stats()}, self.plan.metrics()
        must = self.prev is not None and self.prev * 8 >= self.n and oc.eligible(self.proj) and len(tab[0]) > 0 and not self.options
        fits = self.prev is not None and len(want) <= max(1024, self.prev + self.prev // 4 + 256)   # (run_speculative: 25 % head room + 256)
        ordered = ran_ordered(names) and m.exact_reruns == 0
        (oc.assert_slice_order if ordered else oc.assert_multiset)(got, want, self.proj, what)
        if not ENGINE_TOGGLED:
            if must and fits:
                assert ordered, (what, self.prev, m.exact_reruns, sorted(names))
            if must and not fits:
                assert m.exact_reruns == 1, (what, self.prev, len(want))
            if self.options or not oc.eligible(self.proj) or (self.prev is not None and self.prev * 8 < self.n):
                assert no_ordered(names), (what, self.prev, sorted(names))
        if len(tab[0]):                                             # (an empty table leaves the join, and its history, untouched)
            self.prev = len(want)
        return names, m, ordered

    def close(self):
        self.plan.close()


@pytest.mark.parametrize("n_stages", range(4))
@pytest.mark.parametrize("n", oc.SLICE_ROWS)
def test_rows_in_slice_order(torch_cuda, n, n_stages):
    """Every table x every projection: after a warm-up table the ordered form runs (not for 9 columns) and emits the slice's rows in its
    order, each repeated by its chain; one more plan per projection under NO_ORDERED_JOIN gives the same multiset without the kernels.
    The projections have 1 .. 8 columns, so every oj_write_kernel<N> runs."""
    sl = oc.slice_of(n)
    warm = oc.t_warm(sl)
    seen = 0
    for pname in oc.PROJECTIONS:
        proj = oc.projection(pname, n_stages)
        r, off = Runner(torch_cuda, n, n_stages, proj), Runner(torch_cuda, n, n_stages, proj, options=("NO_ORDERED_JOIN",))
        for c in oc.cases_of(n):
            r.run(warm, "warm")
            names, m, ordered = r.run(c.table, c.name)
            seen += ordered
            off.run(c.table, c.name)
        r.close(); off.close()
    n_eligible = sum(oc.eligible(oc.projection(pname, n_stages)) for pname in oc.PROJECTIONS)
    assert ENGINE_TOGGLED or seen == n_eligible * (len(oc.cases_of(n)) - 1)   # (every projection of up to 8 columns, every table but the empty one)


@pytest.mark.parametrize("pname", ["tag_o_s", "5_words"])
@pytest.mark.parametrize("n", oc.SLICE_ROWS)
def test_chain_cap(torch_cuda, n, pname):
    """254, 255, 256 and 300 table rows on LA (slice rows 0, 256, 1024) and on HA (255, 1023): the count pass caps a row's count at 255 and
    the write pass walks such a chain again.  One word of the packed record and five (two uint4); 0 and 3 stages."""
    sl = oc.slice_of(n)
    for n_stages in (0, 3):
        proj = oc.projection(pname, n_stages)
        r = Runner(torch_cuda, n, n_stages, proj)
        for length in oc.CHAINS:
            tab = oc.t_chain(sl, length)
            r.run(oc.t_warm(sl), "warm")
            names, m, ordered = r.run(tab, f"chain{length}")
            assert ordered or ENGINE_TOGGLED
            got = r.plan.fetch()
            s, o = got[proj.index("s")], got[proj.index("o")]
            for i in oc.CHAIN_ROWS:
                assert int(((s == sl.s[i]) & (o == sl.o[i])).sum()) == length, (r.what, length, i)
            assert len(s) == length * len(oc.CHAIN_ROWS)
        r.close()


@pytest.mark.parametrize("n_stages", [0, 2])
def test_route_boundary(torch_cuda, n_stages):
    """The 2048-row slice: after an execution with 256 rows (x 8 = the slice) the next one takes the ordered form, after one with 255 rows
    it does not; the rows are the reference's either way."""
    sl = oc.slice_of(2048)
    mixed = next(c.table for c in oc.cases_of(2048) if c.name == "mixed")
    r = Runner(torch_cuda, 2048, n_stages, oc.projection("tag_o_s", n_stages))
    r.run(oc.t_rows(sl, 256), "rows256")
    assert r.prev == 256
    names, m, ordered = r.run(mixed, "mixed")
    assert (ordered and m.exact_reruns == 0) or ENGINE_TOGGLED, sorted(names)
    r.run(oc.t_rows(sl, 255), "rows255")
    assert r.prev == 255
    names, m, ordered = r.run(mixed, "mixed")
    assert (no_ordered(names) and not ordered) or ENGINE_TOGGLED, sorted(names)
    r.close()


@pytest.mark.parametrize("n_stages", [0, 3])
@pytest.mark.parametrize("n", [2048, 3072])
def test_overflow_reruns_exactly(torch_cuda, n, n_stages):
    """A previous output of slice rows / 8 leaves room for 1024 rows; the 300-row chains emit 1500: the write pass drops what does not fit,
    the count stays exact, the plan runs again exactly - and the execution after that takes the ordered form with room for all."""
    sl = oc.slice_of(n)
    r = Runner(torch_cuda, n, n_stages, oc.projection("5_words", n_stages))
    r.run(oc.t_rows(sl, n // 8), "warm_eighth")
    r.run(oc.t_rows(sl, n // 8), "warm_eighth")
    assert r.prev == n // 8
    tab = oc.t_chain(sl, 300)
    names, m, ordered = r.run(tab, "chain300")
    assert m.exact_reruns == 1 or ENGINE_TOGGLED, m.exact_reruns
    names, m, ordered = r.run(tab, "chain300")
    assert (ordered and m.exact_reruns == 0) or ENGINE_TOGGLED, (m.exact_reruns, sorted(names))
    r.close()


@pytest.mark.parametrize("n_stages", range(4))
@pytest.mark.parametrize("n", [2047, 2048, 3072])
def test_one_plan_many_tables(torch_cuda, n, n_stages):
    """1500, 3, 0 and 1500 rows, a table in which nothing joins, 1500 rows again (and twice more, so that the large table also follows a
    large one): the scratch head / next / record arrays are sized and cleared for each"""
    sl = oc.slice_of(n)
    big, three, nothing = oc.t_sized(sl, 1500), oc.t_sized(sl, 3), oc.t_nothing(sl)
    r = Runner(torch_cuda, n, n_stages, oc.projection("stage_values", n_stages))
    seen = 0
    for name, tab in (("big", big), ("three", three), ("empty", oc.table([])), ("big", big), ("nothing", nothing), ("big", big), ("big", big), ("three", three), ("big", big)):
        seen += r.run(tab, name)[2]
    assert seen >= 3 or ENGINE_TOGGLED
    r.close()


@pytest.mark.parametrize("n", [2048, 3072])
def test_row_count_on_the_device_only(torch_cuda, n):
    """The table comes out of a FilterExec: 1500 rows of capacity, one in ten alive (or none), the count in device memory only"""
    sl = oc.slice_of(n)
    warm = oc.t_warm(sl)
    warm = warm + [np.full(len(warm[0]), oc.KEEP, np.uint32)]
    tenth = oc.t_sized(sl, 1500, [oc.KEEP if i % 10 == 0 else oc.DROP for i in range(1500)])
    none = oc.t_sized(sl, 1500, [oc.DROP] * 1500)
    r = Runner(torch_cuda, n, 2, oc.projection("stage_values", 2), flagged=True)
    for name, tab in (("tenth", tenth), ("none", none)):           # each after two executions over the warm-up table
        r.run(warm, "warm_flagged")
        r.run(warm, "warm_flagged")
        names, m, ordered = r.run(tab, name)
        assert ordered or ENGINE_TOGGLED, (name, sorted(names))
    assert r.prev == 0
    r.run(tenth, "tenth")
    r.close()


@pytest.mark.parametrize("n_stages", [0, 2])
def test_no_speculation(torch_cuda, n_stages):
    sl = oc.slice_of(2048)
    r = Runner(torch_cuda, 2048, n_stages, oc.projection("tag_o_s", n_stages), options=("NO_SPECULATION",))
    for c in oc.cases_of(2048):
        r.run(oc.t_warm(sl), "warm")
        names, m, ordered = r.run(c.table, c.name)
        assert not ordered
    r.close()


@pytest.mark.parametrize("extra_row", [False, True], ids=["2048", "2049"])
def test_band_join_over_counted_matches(torch_cuda, extra_row):
    """The band join that takes its row records from the ordered slice join below it, counted (one product of the batch twice, so not in
    place): oj_write_band_kernel also writes the key boundaries of the matches.  The pF slice has exactly two tiles (the closing call
    for a slice that ends with its last tile), the second of them first without a match and then with; then the same with 2049 rows."""
    st = oc.band_store(extra_row)
    gs = rf.GpuQuadStore()
    gs.extend(*st.quads)
    gs.set_typed_values(st.tv, st.decimals)
    windows = (oc.BAND_WINDOW, oc.BAND_WINDOW_2)
    plan = gs.plan(oc.band_over_ordered_plan(windows, True)).enable_kernel_timing(True)
    for second_tile in (False, True, False):
        params = oc.band_params(second_tile)
        want, unfiltered = bc.window_reference(st.quads, st.terms, oc.band_constants(st, params), windows, True)
        keep, ptrs = on_device(torch_cuda, params)
        plan.bind_table(0, ptrs, len(params[0]))
        for rep in range(6):
            got = plan.execute().fetch()
            assert plan.result_info()[0] == len(want), (second_tile, rep, plan.result_info()[0], len(want))
            np.testing.assert_array_equal(ku.multiset(got, len(want)), want, err_msg=f"second tile {second_tile} rep {rep}")
            names = {k[0] for k in plan.kernel_stats()}
        print(f"{st.n_build} rows, second tile {second_tile}: {len(want)} of {unfiltered} rows; {sorted(k for k in names if 'oj_' in k or 'band_' in k)}")
        if not ENGINE_TOGGLED:
            assert any("oj_write_band_kernel" in k for k in names) and any("oj_count_kernel" in k for k in names), sorted(names)
            assert not any(IN_PLACE in k for k in names), sorted(names)
        del keep
    plan.close()
