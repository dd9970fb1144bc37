"""The front of a steady batched-Q5 step (ordered_join.hip, oj_probe_kernel(.., OjKeyValues)): when the band join reads the slice's rows in place
through their cached windows, the ordered slice join below it owes its probe pass, and the band join settles it with one pass that writes the
batch's values by key — no multimap, no stage rows, no packed records, no records pass.  A step that takes another form after all runs the full
probe in front of its count pass (host_logic.hpp, oj_probe_form).  Every step is compared, as a multiset, with the oracle; which passes ran is
read from the kernel classes of the step, and only when no RDFGPU_NO_* / RDFGPU_FORCE_* toggle is set for the run."""
import os

import numpy as np
import pytest

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi, bsbm
from oracle import oracle as orc
import kat_util as ku

pytestmark = pytest.mark.gpu

ENGINE_TOGGLED = any(k.startswith(("RDFGPU_NO_", "RDFGPU_FORCE_")) for k in os.environ)   # a debugging toggle is set for the whole run
LEAN = "OjKeyValues"            # the kernel names carry their tag types
IN_PLACE = "OjInPlace"
PF, NUM1 = "bsbm:productFeature", "bsbm:productPropertyNumeric1"


def stores(ds, keep=None):
    """the device store and the oracle's over the dataset's quads (`keep`: a mask of the quads that go in)"""
    cols = [c if keep is None else c[keep] for c in (ds.g, ds.s, ds.p, ds.o)]
    gs, os_ = rf.GpuQuadStore(), orc.OracleStore()
    assert gs.extend(*cols) == os_.extend(*cols)
    gs.set_typed_values(ds.typed_values, ds.decimals)
    os_.set_typed_values(ds.typed_values, ds.decimals)
    return gs, os_


def on_device(torch, cols):
    ts = [torch.from_numpy(np.ascontiguousarray(c, dtype=np.uint32).view(np.int32)).cuda() for c in cols]
    return ts, [t.data_ptr() for t in ts]


def batch_of(ds, rng, n, foreign=0, among=None, repeat=0):
    """n instances of distinct products (of `among`, indices of products, when given); `foreign` of them take an id that is no product,
    `repeat` of them the product of the first instance"""
    pool = ds.n_products if among is None else np.asarray(among)
    xs = np.array([ds.product(int(i)) for i in rng.choice(pool, n, replace=False)], dtype=np.uint32)
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

    def run(self, params, same_as=None):
        """one step, checked against the oracle (or, `same_as`, against bindings that were): (metrics, kernel classes that ran, the bindings)"""
        keep, ptrs = on_device(self.torch, params)
        self.plan.bind_table(0, ptrs, len(params[0]))
        got = self.plan.execute().fetch()
        if same_as is None:
            exp, n_exp, _ = self.os_.execute(self.desc, [params])
            np.testing.assert_array_equal(ku.multiset(got), ku.multiset(exp, n_exp))
        else:
            np.testing.assert_array_equal(ku.multiset(got), ku.multiset(same_as))
        return self.plan.metrics(), {k[0] for k in self.plan.kernel_stats()}, got


def ran_any(ran, part):
    return any(part in k for k in ran)


def full_probe(ran):
    """the untagged probe pass ran (its class name ends with the kernel's; the tagged one's goes on with its arguments)"""
    return any(k.endswith("oj_probe_kernel") for k in ran)


def lean(m, ran):
    """the steady step: the values-by-key pass in front of the in-place pass, no full probe and no records pass; nothing built, one wait"""
    return ran_any(ran, LEAN) and not full_probe(ran) and not ran_any(ran, "oj_band_records_kernel") and ran_any(ran, IN_PLACE) and \
        m.host_syncs == 1 and m.tables_built == 0 and m.exact_reruns == 0


def counted(ran):
    return full_probe(ran) and ran_any(ran, "oj_count_kernel") and not ran_any(ran, LEAN)


def say(m, ran):
    return (m.host_syncs, m.tables_built, m.exact_reruns, sorted(ran))


def until_steady(r, ds, rng, n=1400, steps=7, among=None):
    for step in range(steps):
        m, ran, _ = r.run(batch_of(ds, rng, n + step, among=among))
    if not ENGINE_TOGGLED:
        assert lean(m, ran), say(m, ran)
    return m, ran


@pytest.fixture(scope="module")
def small(torch_cuda):
    ds = bsbm.generate(2000)
    gs, os_ = stores(ds)
    return ds, gs, os_


def test_steady_steps(small, torch_cuda):
    """Eight batches of 1400 - 1500 distinct products, ids that are no product's on odd steps.  The last four steps run the values-by-key pass and
    the in-place pass, neither the full probe nor the records pass, wait once, build nothing, and launch one kernel less than the same step of a
    plan with NO_BAND_ROW_CACHE (probe, records, in place against values, in place)."""
    ds, gs, os_ = small
    rng = np.random.default_rng(31)
    a, b = Runner(torch_cuda, gs, os_, ds), Runner(torch_cuda, gs, os_, ds, "NO_BAND_ROW_CACHE")
    seen = []
    for step in range(8):
        params = batch_of(ds, rng, 1500 - 14 * step, foreign=40 if step % 2 else 0)
        first = a.run(params)
        seen.append((first, b.run(params, same_as=first[2])))
    if ENGINE_TOGGLED:
        return
    for (m, ran, _), (mb, ran_b, _) in seen[-4:]:
        assert lean(m, ran), say(m, ran)
        assert not ran_any(ran_b, LEAN) and full_probe(ran_b) and ran_any(ran_b, "oj_band_records_kernel") and ran_any(ran_b, IN_PLACE), sorted(ran_b)
        assert m.kernels_launched == mb.kernels_launched - 1, (m.kernels_launched, mb.kernels_launched)


def test_launch_edges(small, torch_cuda):
    """Three consecutive steady steps of 5 x 256 - 1, 5 x 256 and 5 x 256 + 1 instances: the last workgroup of the pass full but for one lane, full,
    and one lane of a sixth."""
    ds, gs, os_ = small
    rng = np.random.default_rng(32)
    r = Runner(torch_cuda, gs, os_, ds)
    until_steady(r, ds, rng)
    for n in (1279, 1280, 1281):
        m, ran, _ = r.run(batch_of(ds, rng, n))
        if not ENGINE_TOGGLED:
            assert lean(m, ran), (n,) + say(m, ran)


def test_stale_values(torch_cuda):
    """Two disjoint halves of the products on alternate steps: a key that carried a value in one step must say "no table row" again in the next,
    or its slice rows would emit the bindings of an instance that is gone.  The halves cover the same number of slice rows, so that each still
    covers half of the slice and the route stays."""
    ds = bsbm.generate(2000, seed=12)
    sel = ds.p == ds.pred[PF]
    pairs = np.unique(np.stack([ds.s[sel], ds.o[sel]], axis=1), axis=0)   # the slice as the store holds it: distinct (product, feature) pairs
    rows = np.bincount(pairs[:, 0] - ds.product_base, minlength=ds.n_products)
    rng = np.random.default_rng(33)
    order = rng.permutation(ds.n_products)
    half = [list(order[:1000]), list(order[1000:])]
    keep = None
    if rows.sum() % 2:                                             # an odd slice cannot be halved: one pair of a product with many stays out
        victim = int(np.argmax(rows))
        gone = pairs[pairs[:, 0] == ds.product(victim)][0]
        keep = ~(sel & (ds.s == gone[0]) & (ds.o == gone[1]))
        rows[victim] -= 1
    diff = int(rows[half[0]].sum() - rows[half[1]].sum())          # even; swapping i and j moves it by 2 (rows[j] - rows[i])
    while diff:
        step = max(-19, min(19, diff // 2))
        i, j = next((i, j) for i in range(1000) for j in range(1000) if rows[half[0][i]] - rows[half[1][j]] == step)
        half[0][i], half[1][j] = half[1][j], half[0][i]
        diff -= 2 * step
    assert rows[half[0]].sum() == rows[half[1]].sum() and not set(half[0]) & set(half[1])
    gs, os_ = stores(ds, keep)
    r = Runner(torch_cuda, gs, os_, ds)
    until_steady(r, ds, rng)
    seen = [r.run(batch_of(ds, rng, 1000, among=half[step % 2])) for step in range(6)]
    if not ENGINE_TOGGLED:
        for m, ran, _ in seen[1:]:                                 # (the first half-batch follows a larger one: any route)
            assert lean(m, ran), say(m, ran)


def test_product_without_a_stage_row(torch_cuda):
    """A store from which one product's productPropertyNumeric1 triple is left out: the instance of that product has no row in that stage, is not
    linked, emits nothing (the oracle's inner join drops it too) and leaves every other instance's bindings alone."""
    ds = bsbm.generate(2000, seed=13)
    odd = 1234
    gs, os_ = stores(ds, ~((ds.p == ds.pred[NUM1]) & (ds.s == ds.product(odd))))
    rng = np.random.default_rng(34)
    r = Runner(torch_cuda, gs, os_, ds)
    others = [i for i in range(ds.n_products) if i != odd]
    until_steady(r, ds, rng, among=others)
    for step in range(3):
        params = batch_of(ds, rng, 1410 + step, among=others)
        params[1][7 * step] = ds.product(odd)
        m, ran, got = r.run(params)
        assert not np.any(np.asarray(got[0], dtype=np.uint32) == params[0][7 * step])           # the instance of that product has no binding
        if not ENGINE_TOGGLED:
            assert lean(m, ran), say(m, ran)


def test_repeated_product(small, torch_cuda):
    """A product with two instances in a steady plan: the exchange by key meets the first one's value, the step re-runs exactly and answers like
    the oracle; the next steps count and compact (the full probe in its old place) until an execution measured no repeat, then the lean form is back."""
    ds, gs, os_ = small
    rng = np.random.default_rng(35)
    r = Runner(torch_cuda, gs, os_, ds)
    until_steady(r, ds, rng, n=1200)
    rep = batch_of(ds, rng, 1200, repeat=1)
    m, ran, _ = r.run(rep)
    if ENGINE_TOGGLED:
        return
    assert m.exact_reruns == 1, m.exact_reruns
    m, ran, _ = r.run(rep)                                         # the history saw the repeat: counted route, no re-run
    assert m.exact_reruns == 0 and counted(ran), say(m, ran)
    m, ran, _ = r.run(batch_of(ds, rng, 1210))                     # distinct products again: still counted (history of the repeats) ..
    assert m.exact_reruns == 0 and counted(ran), say(m, ran)
    m, ran, _ = r.run(batch_of(ds, rng, 1190))                     # .. and lean once an execution measured no repeat
    assert lean(m, ran), say(m, ran)


def test_instance_tag_that_is_the_fill_value(small, torch_cuda):
    """An instance whose tag is 0xFFFFFFFF, the value that says "no table row": the pass counts it as a slow row, the step is answered exactly (like
    the oracle: Runner.run), and with the bindings of a NO_BAND_ROW_CACHE plan on the same batch."""
    ds, gs, os_ = small
    rng = np.random.default_rng(36)
    a, b = Runner(torch_cuda, gs, os_, ds), Runner(torch_cuda, gs, os_, ds, "NO_BAND_ROW_CACHE")
    for step in range(7):
        params = batch_of(ds, rng, 1400 + step)
        m, ran, got = a.run(params)
        b.run(params, same_as=got)
    params = batch_of(ds, rng, 1390)
    params[0][5] = 0xFFFFFFFF
    if not ENGINE_TOGGLED:
        assert lean(m, ran), say(m, ran)
    m, ran, got = a.run(params)
    b.run(params, same_as=got)
    assert np.any(np.asarray(got[0], dtype=np.uint32) == 0xFFFFFFFF)                            # (the instance has bindings: the exact answer holds them)
    if not ENGINE_TOGGLED:
        assert m.exact_reruns == 1, say(m, ran)


def test_fallback_inside_one_execution(torch_cuda):
    """After steady steps the store is extended by a productPropertyNumeric1 of one product that is an xsd:double (the product had none: the slice's keys
    stay unique).  The plan's history still promises the lean form, so the ordered join owes its probe; the step finds the row cache declined, runs the
    full probe in front of the count pass, and answers like the oracle — as do the two steps after it, with that product in the batch."""
    ds = bsbm.generate(2000, seed=14)
    odd = 321
    gs, os_ = stores(ds, ~((ds.p == ds.pred[NUM1]) & (ds.s == ds.product(odd))))
    rng = np.random.default_rng(37)
    r = Runner(torch_cuda, gs, os_, ds)
    others = [i for i in range(ds.n_products) if i != odd]
    until_steady(r, ds, rng, among=others)
    double_id = int(np.flatnonzero(ds.typed_values["tag"] == abi.TV_DOUBLE)[5])
    new = [np.zeros(1, np.uint32), np.array([ds.product(odd)], np.uint32), np.array([ds.pred[NUM1]], np.uint32), np.array([double_id], np.uint32)]
    assert gs.extend(*new) == os_.extend(*new) == 1
    m, ran, _ = r.run(batch_of(ds, rng, 1410, among=others))
    if not ENGINE_TOGGLED:
        assert full_probe(ran) and ran_any(ran, "oj_count_kernel") and not ran_any(ran, LEAN), say(m, ran)
    for step in range(2):
        params = batch_of(ds, rng, 1420 + step, among=others)
        params[1][step] = ds.product(odd)
        r.run(params)


def test_drop_tables_between_two_steady_steps(torch_cuda):
    """rdfgpu_store_drop_tables between two steady steps: the next step builds the slice's tables inside the step (the rows' windows among them) and
    keeps the lean form — what it needs of the ordered join to build them are host fields — and the one after it is steady again."""
    ds = bsbm.generate(2000, seed=15)
    gs, os_ = stores(ds)
    rng = np.random.default_rng(38)
    r = Runner(torch_cuda, gs, os_, ds)
    until_steady(r, ds, rng)
    gs.drop_tables()
    m, ran, _ = r.run(batch_of(ds, rng, 1410))
    if not ENGINE_TOGGLED:
        assert m.tables_built >= 6 and m.exact_reruns == 0 and ran_any(ran, LEAN) and not full_probe(ran) and ran_any(ran, "band_row_win_rows_kernel"), say(m, ran)
    m, ran, _ = r.run(batch_of(ds, rng, 1420))
    if not ENGINE_TOGGLED:
        assert lean(m, ran), say(m, ran)
