"""The band join of the batched Q5 reading the slice's own rows in place (ordered_join.hip, OjInPlace): once a plan has history and
no product of the batch appears twice, the ordered slice join below it neither counts nor compacts its matches.  Every check here
compares whole result multisets: with the oracle, and with the counted, compacted route (which NO_BAND_COMPACT keeps: the in-place
route needs the 16-byte records)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi, bsbm
from oracle import oracle as orc
import kat_util as ku

ENGINE_TOGGLED = any(k.startswith(("RDFGPU_NO_", "RDFGPU_FORCE_")) for k in os.environ)   # a debugging toggle is set for the whole run
IN_PLACE = "OjInPlace"          # the in-place form's kernel name carries its tag type
COUNTED = ("oj_count_kernel", "band_desc_kernel")


def stores(ds):
    gs, os_ = rf.GpuQuadStore(), orc.OracleStore()
    assert gs.extend(ds.g, ds.s, ds.p, ds.o) == os_.extend(ds.g, ds.s, ds.p, ds.o)
    gs.set_typed_values(ds.typed_values, ds.decimals)
    os_.set_typed_values(ds.typed_values, ds.decimals)
    return gs, os_


def on_device(torch, cols):
    ts = [torch.from_numpy(np.ascontiguousarray(c, dtype=np.uint32).view(np.int32)).cuda() for c in cols]
    return ts, [t.data_ptr() for t in ts]


def batch_of(ds, rng, n, repeat=0, foreign=0):
    """n instances of distinct products; `repeat` of them take the product of another instance, `foreign` an id that is no product"""
    xs = np.array([ds.product(int(i)) for i in rng.choice(ds.n_products, n, replace=False)], dtype=np.uint32)
    if repeat:
        xs[rng.choice(np.arange(1, n), repeat, replace=False)] = xs[0]
    if foreign:
        xs[rng.choice(n, foreign, replace=False)] = ds.feature_base + rng.integers(0, ds.n_features, foreign)
    return [np.arange(1, n + 1, dtype=np.uint32), xs]


class Runner:
    def __init__(self, torch, gs, os_, ds, option=None):
        self.torch, self.os_, self.desc = torch, os_, bsbm.q5_batch_plan(ds)
        self.plan = gs.plan(self.desc).enable_kernel_timing(True)
        if option:
            self.plan.set_option(option, 1)

    def run(self, params, check=True):
        keep, ptrs = on_device(self.torch, params)
        self.plan.bind_table(0, ptrs, len(params[0]))
        got = self.plan.execute().fetch()
        if check:
            exp, n_exp, _ = self.os_.execute(self.desc, [params])
            np.testing.assert_array_equal(ku.multiset(got), ku.multiset(exp, n_exp))
        ran = {k[0] for k in self.plan.kernel_stats()}
        return got, self.plan.metrics(), ran


def in_place(ran, steady=True):
    """the in-place route ran; steady: with the slice's block layout found cached (its first execution builds it: band_desc_kernel)"""
    skipped = ("oj_count_kernel",) + (("band_desc_kernel",) if steady else ())
    return any(IN_PLACE in k for k in ran) and not any(c in k for k in ran for c in skipped)


def counted(ran):
    return not any(IN_PLACE in k for k in ran) and all(any(c in k for k in ran) for c in COUNTED)


@pytest.fixture(scope="module")
def small(torch_cuda):
    ds = bsbm.generate(2000)
    gs, os_ = stores(ds)
    return ds, gs, os_


def test_in_place_against_compacted_and_oracle(small, torch_cuda):
    """First executions (exact, then the counted routes) keep today's forms; from the fifth on the in-place route runs (with one host sync
    and no table built: the first execution that could take it built the slice's block layout), and answers like the oracle and like the
    32-byte counted route on every batch, ids that are no product's included."""
    ds, gs, os_ = small
    rng = np.random.default_rng(5)
    a, b = Runner(torch_cuda, gs, os_, ds), Runner(torch_cuda, gs, os_, ds, "NO_BAND_COMPACT")
    forms = []
    for step in range(8):
        params = batch_of(ds, rng, 1500 - 20 * step, foreign=40 if step % 2 else 0)
        got, m, ran = a.run(params)
        got_b, _, ran_b = b.run(params, check=False)
        np.testing.assert_array_equal(ku.multiset(got), ku.multiset(got_b))
        assert not any(IN_PLACE in k for k in ran_b), sorted(ran_b)
        forms.append("in place" if in_place(ran, steady=False) else "counted" if counted(ran) else "other")
    if not ENGINE_TOGGLED:
        assert forms[0] != "in place" and "counted" in forms and forms[-4:] == ["in place"] * 4, forms
        assert in_place(ran) and m.host_syncs == 1 and m.tables_built == 0 and m.exact_reruns == 0, (m.host_syncs, m.tables_built, m.exact_reruns)
        assert counted(ran_b), sorted(ran_b)


def test_repeated_product_falls_back_exactly(small, torch_cuda):
    """A batch in which one product has two instances (a chain of two table rows): the in-place execution cannot hold both, so it is
    re-run exactly (the bindings stay the oracle's); the next executions count and compact until a batch without repeats is seen."""
    ds, gs, os_ = small
    rng = np.random.default_rng(6)
    r = Runner(torch_cuda, gs, os_, ds)
    for step in range(6):
        _, m, ran = r.run(batch_of(ds, rng, 1200 + step))
    if ENGINE_TOGGLED:
        return
    assert in_place(ran), sorted(ran)
    rep = batch_of(ds, rng, 1200, repeat=1)
    _, m, ran = r.run(rep)
    assert m.exact_reruns == 1, m.exact_reruns
    _, m, ran = r.run(rep)                                       # the history saw a row behind a chain head: counted route, no re-run
    assert m.exact_reruns == 0 and counted(ran), (m.exact_reruns, sorted(ran))
    _, m, ran = r.run(batch_of(ds, rng, 1210))                   # distinct products again: still counted (history of the repeats) ..
    assert m.exact_reruns == 0 and counted(ran), (m.exact_reruns, sorted(ran))
    _, m, ran = r.run(batch_of(ds, rng, 1190))                   # .. and in place once an execution measured no repeat
    assert m.exact_reruns == 0 and in_place(ran) and m.host_syncs == 1, (m.exact_reruns, m.host_syncs, sorted(ran))


def test_instances_without_a_numeric_stage_row(torch_cuda):
    """Instances whose product lost its productPropertyNumeric1 triple join nothing (their slice rows carry the record that passes
    nothing) and are no candidate of any other instance; slice rows of products outside the batch likewise."""
    ds = bsbm.generate(1500, seed=9)
    gs, os_ = stores(ds)
    rng = np.random.default_rng(9)
    num1 = ds.pred["bsbm:productPropertyNumeric1"]
    gone = [ds.product(int(i)) for i in rng.choice(ds.n_products, 60, replace=False)]
    sel = (ds.p == num1) & np.isin(ds.s, gone)
    q = [c[sel] for c in (ds.g, ds.s, ds.p, ds.o)]
    assert gs.remove(*q) == os_.remove(*q) == len(gone)
    r = Runner(torch_cuda, gs, os_, ds)
    ran = set()
    for step in range(7):
        params = batch_of(ds, rng, 900 + 10 * step)
        params[1][:30] = gone[:30]                               # a few instances of the products without the stage row
        _, m, ran = r.run(params)
    if not ENGINE_TOGGLED:
        assert in_place(ran) and m.exact_reruns == 0, (m.exact_reruns, sorted(ran))


def test_layout_rebuilt_after_drop_tables(small, torch_cuda):
    """rdfgpu_store_drop_tables: the next in-place execution builds the band entries and the slice's block layout inside the step (and
    counts them in tables_built); the one after that finds them cached again."""
    ds, gs, os_ = small
    rng = np.random.default_rng(8)
    r = Runner(torch_cuda, gs, os_, ds)
    for step in range(6):
        _, m, ran = r.run(batch_of(ds, rng, 1400 + step))
    if ENGINE_TOGGLED:
        return
    assert in_place(ran) and m.tables_built == 0, (m.tables_built, sorted(ran))
    gs.drop_tables()
    _, m, ran = r.run(batch_of(ds, rng, 1420))
    assert m.tables_built >= 5 and m.exact_reruns == 0, (m.tables_built, m.exact_reruns)
    assert in_place(ran, steady=False), sorted(ran)
    assert any("band_entries_kernel" in k for k in ran) and any("band_desc_kernel" in k for k in ran), sorted(ran)
    _, m, ran = r.run(batch_of(ds, rng, 1430))
    assert in_place(ran) and m.tables_built == 0 and m.host_syncs == 1, (m.tables_built, m.host_syncs, sorted(ran))


@pytest.mark.parametrize("batch", [200_000, 40_000])
def test_bsbm_100m_in_place_against_compacted(torch_cuda, batch):
    """BSBM-100M (285 000 products): a batch that covers most of the slice takes the in-place route, one that covers a seventh of it keeps
    the counted route (the in-place form would carry every slice row through the pair test).  Either way the whole result is the one of
    the 32-byte counted route, and the bindings of sampled instance tags are the oracle's per-query results."""
    ds = bsbm.generate(285_000)
    gs = rf.GpuQuadStore()
    gs.extend(ds.g, ds.s, ds.p, ds.o)
    gs.set_typed_values(ds.typed_values, ds.decimals)
    os_ = orc.OracleStore()
    for comp in (abi.GSPO, abi.GPOS, abi.GOSP):
        os_.adopt_sorted(comp, gs.read_index(comp))
    os_.set_typed_values(ds.typed_values, ds.decimals)
    rng = np.random.default_rng(101)
    params = batch_of(ds, rng, batch)
    tags = sorted({1, 2, batch // 2, batch - 1, batch} | set(int(t) for t in rng.integers(1, batch + 1, 4)))
    expected = []
    for t in tags:
        cols, n, _ = os_.execute(bsbm.q5_plan(ds, int(params[1][t - 1])))
        expected.append(np.stack([np.full(n, t, np.uint32), cols[0][:n], cols[1][:n]], axis=1))
    expected = ku.multiset(list(np.concatenate(expected).T))
    a, b = Runner(torch_cuda, gs, os_, ds), Runner(torch_cuda, gs, os_, ds, "NO_BAND_COMPACT")
    for _ in range(6):
        got, m, ran = a.run(params, check=False)
        sel = np.isin(got[0], tags)
        np.testing.assert_array_equal(ku.multiset([c[sel] for c in got]), expected)
    for _ in range(6):
        got_b, _, ran_b = b.run(params, check=False)
    np.testing.assert_array_equal(ku.multiset(got), ku.multiset(got_b))
    if not ENGINE_TOGGLED:
        assert (in_place(ran) if batch > ds.n_products // 2 else counted(ran)) and m.host_syncs == 1 and m.exact_reruns == 0, \
            (m.host_syncs, m.exact_reruns, sorted(ran))
        assert counted(ran_b), sorted(ran_b)
