"""The band join of the batched Q5 reading the slice's rows in place with the pair test's VERDICTS kept on the slice (band_join.hip,
band_pair_bits_kernel and band_mask_kernel's CACHED form; store.hpp, SliceTable::BandRowWindows::pair_bits): the entries, the block layout
and the rows' windows are all tables of the store version and the plan's literals, so the 64 words a block's pair test writes are too, up
to which of its rows have a table row in the batch.  A step streams the cached words, notes the valid rows of every block and counts.
Every check compares whole result multisets with the oracle; NO_BAND_PAIR_CACHE keeps the pair test, and which form a step took shows in
the bytes recorded for the band_mask_kernel class: 540 per block + 4 per slice row with the verdicts cached, 16 + 12 per slice row without."""
import os

import numpy as np
import pytest

import rdf_fusion_amd as rf
from rdf_fusion_amd import bsbm
from oracle import oracle as orc
import kat_util as ku

gpu = pytest.mark.gpu

ENGINE_TOGGLED = any(k.startswith(("RDFGPU_NO_", "RDFGPU_FORCE_")) for k in os.environ)   # a debugging toggle is set for the whole run
IN_PLACE = "OjInPlace"          # the in-place form's kernel name carries its tag type
MASK, BUILD = "band_mask_kernel", "band_pair_bits_kernel"
PF, NUM1 = "bsbm:productFeature", "bsbm:productPropertyNumeric1"


def stores(ds):
    gs, os_ = rf.GpuQuadStore(), orc.OracleStore()
    assert gs.extend(ds.g, ds.s, ds.p, ds.o) == os_.extend(ds.g, ds.s, ds.p, ds.o)
    gs.set_typed_values(ds.typed_values, ds.decimals)
    os_.set_typed_values(ds.typed_values, ds.decimals)
    return gs, os_


def on_device(torch, cols):
    ts = [torch.from_numpy(np.ascontiguousarray(c, dtype=np.uint32).view(np.int32)).cuda() for c in cols]
    return ts, [t.data_ptr() for t in ts]


def batch_of(ds, rng, n, foreign=0, among=None):
    """n instances of distinct products (of `among`, indices of products, when given); `foreign` of them take an id that is no product"""
    pool = ds.n_products if among is None else np.asarray(among)
    xs = np.array([ds.product(int(i)) for i in rng.choice(pool, n, replace=False)], dtype=np.uint32)
    if foreign:
        xs[rng.choice(n, foreign, replace=False)] = ds.feature_base + rng.integers(0, ds.n_features, foreign)
    return [np.arange(1, n + 1, dtype=np.uint32), xs]


def batch_with(ids):
    ids = np.asarray(ids, dtype=np.uint32)
    return [np.arange(1, len(ids) + 1, dtype=np.uint32), ids]


def quads(ds, s, p, o):
    s = np.asarray(s, dtype=np.uint32)
    return [np.zeros(len(s), np.uint32), s, np.full(len(s), p, np.uint32), np.asarray(o, dtype=np.uint32)]


def feature_pairs(ds):
    """the productFeature slice as the store holds it: distinct (product, feature) pairs"""
    sel = ds.p == ds.pred[PF]
    return np.unique(np.stack([ds.s[sel], ds.o[sel]], axis=1), axis=0)


def layout_of(pairs):
    """(rows of the slice, 64 x 64 blocks of its in-place layout): a feature group of E rows takes ceil(E / 64)^2 blocks"""
    sizes = np.unique(pairs[:, 1], return_counts=True)[1]
    chunks = (sizes + 63) // 64
    return len(pairs), int((chunks * chunks).sum())


class Step:
    def __init__(self, m, stats):
        self.m, self.ran = m, {k[0] for k in stats}
        per_row = [nbytes // rows for name, launches, ms, nbytes, rows in stats if IN_PLACE in name and rows]
        self.per_row = per_row[0] if per_row else None                                  # bytes per row of the in-place pass
        mask = [nbytes for name, launches, ms, nbytes, rows in stats if MASK in name]
        self.mask_bytes = mask[0] if mask else None
        self.built = any(BUILD in k for k in self.ran)

    def quiet(self):
        """the in-place route with the cached windows, nothing built or waited for inside the step"""
        return self.per_row == 12 and not self.built and not any("oj_count_kernel" in k or "band_desc_kernel" in k or "band_row_win" in k for k in self.ran) and \
            self.m.tables_built == 0 and self.m.host_syncs == 1 and self.m.exact_reruns == 0

    def cached(self, nb, n_blocks):
        return self.quiet() and self.mask_bytes == 540 * n_blocks + 4 * nb

    def pair_test(self, nb):
        return self.quiet() and self.mask_bytes == 16 * nb + 12 * nb

    def why(self):
        return (self.m.tables_built, self.m.host_syncs, self.m.exact_reruns, self.per_row, self.mask_bytes, sorted(self.ran))


class Runner:
    def __init__(self, torch, gs, os_, ds, options=None, **windows):
        self.torch, self.os_, self.desc = torch, os_, bsbm.q5_batch_plan(ds, **windows)
        self.plan = gs.plan(self.desc).enable_kernel_timing(True)
        for name, value in (options or {}).items():
            self.plan.set_option(name, value)

    def run(self, params):
        """one step, checked against the oracle"""
        keep, ptrs = on_device(self.torch, params)
        self.plan.bind_table(0, ptrs, len(params[0]))
        got = self.plan.execute().fetch()
        exp, n_exp, _ = self.os_.execute(self.desc, [params])
        np.testing.assert_array_equal(ku.multiset(got), ku.multiset(exp, n_exp))
        return Step(self.plan.metrics(), self.plan.kernel_stats())


def until_steady(r, ds, rng, n=1400, steps=8):
    return [r.run(batch_of(ds, rng, n + step)) for step in range(steps)]


@pytest.fixture(scope="module")
def small(torch_cuda):
    ds = bsbm.generate(2000)
    gs, os_ = stores(ds)
    return ds, gs, os_, layout_of(feature_pairs(ds))


@gpu
def test_against_the_uncached_form_and_the_oracle(small, torch_cuda):
    """Eight different batches (ids that are no product's on odd steps): with the verdicts kept and without them (NO_BAND_PAIR_CACHE) every
    step answers like the oracle.  The last four steps of the default plan stream the cached words, build nothing and wait once; the plan
    with the option never builds them and keeps the pair test over the cached windows."""
    ds, gs, os_, (nb, n_blocks) = small
    rng = np.random.default_rng(31)
    a, b = Runner(torch_cuda, gs, os_, ds), Runner(torch_cuda, gs, os_, ds, {"NO_BAND_PAIR_CACHE": 1})
    seen_a, seen_b = [], []
    for step in range(8):
        params = batch_of(ds, rng, 1500 - 20 * step, foreign=40 if step % 2 else 0)
        seen_a.append(a.run(params))
        seen_b.append(b.run(params))
    if ENGINE_TOGGLED:
        return
    for s in seen_a[-4:]:
        assert s.cached(nb, n_blocks), s.why()
    assert sum(s.built for s in seen_a) <= 1                        # (none at all when an earlier test's plan left the table on the store)
    assert not any(s.built for s in seen_b), [s.why() for s in seen_b if s.built]
    for s in seen_b[-4:]:
        assert s.pair_test(nb), s.why()


@gpu
def test_rows_entering_and_leaving(torch_cuda):
    """Two batches of 1 500 products that share 1 000 on alternate steps: a row valid in one step is not in the next.  Then a batch chosen
    from the slice's own order (feature, then product): one feature group's rows 0 .. 63 all without an instance (blocks that count
    nothing), another group's second chunk of rows with exactly one (blocks of one valid row).  A repeated product closes the in-place
    route for a step (the counted route answers); the batches after it come back to the cached words."""
    ds = bsbm.generate(2000, seed=12)
    pairs = feature_pairs(ds)
    nb, n_blocks = layout_of(pairs)
    gs, os_ = stores(ds)
    rng = np.random.default_rng(32)
    r = Runner(torch_cuda, gs, os_, ds)
    s = until_steady(r, ds, rng)[-1]
    if not ENGINE_TOGGLED:
        assert s.cached(nb, n_blocks), s.why()
    order = rng.permutation(ds.n_products)
    halves = [[ds.product(int(i)) for i in order[:1500]], [ds.product(int(i)) for i in order[500:]]]
    seen = [r.run(batch_with(halves[step % 2])) for step in range(6)]
    # the slice's order: rows sorted by feature, then product (np.unique sorted the pairs by product, then feature)
    rows = pairs[np.lexsort((pairs[:, 0], pairs[:, 1]))]
    sizes = np.bincount(rows[:, 1] - ds.feature_base, minlength=ds.n_features)
    first = np.concatenate([[0], np.cumsum(sizes)])
    big = [f for f in range(ds.n_features) if sizes[f] >= 70]
    f0, f1 = big[0], big[1]
    out0 = set(rows[first[f0]:first[f0] + 64, 0].tolist())                     # the products of group f0's rows 0 .. 63
    chunk1 = [int(p) for p in rows[first[f1] + 64:first[f1] + min(128, sizes[f1]), 0]]
    kept = next(p for p in chunk1 if p not in out0)
    out = out0 | (set(chunk1) - {kept})
    allowed = [ds.product(i) for i in range(ds.n_products) if ds.product(i) not in out and ds.product(i) != kept]
    ids = [kept] + [allowed[int(i)] for i in rng.choice(len(allowed), 1499, replace=False)]
    assert not set(ids) & out and kept in ids and len(set(ids)) == 1500
    seen.append(r.run(batch_with(ids)))
    if not ENGINE_TOGGLED:
        for s in seen:
            assert s.cached(nb, n_blocks), s.why()
    twice = list(halves[0])
    twice[7] = twice[900]
    s = r.run(batch_with(twice))                                                # (equal to the oracle, like every step)
    if not ENGINE_TOGGLED:
        assert s.m.exact_reruns >= 1 and not s.cached(nb, n_blocks), s.why()
    after = [r.run(batch_with(halves[step % 2])) for step in range(3)]
    if not ENGINE_TOGGLED:
        assert after[1].cached(nb, n_blocks) and after[2].cached(nb, n_blocks), (after[1].why(), after[2].why())


@gpu
def test_group_and_block_edges(torch_cuda):
    """Feature groups of exactly 65, 64, 63 rows and of one row (one block of 64 rows more or less, a block of one), beside the store's
    own groups of 127, 128 and 129 rows."""
    ds = bsbm.generate(2000)
    pairs = feature_pairs(ds)
    sizes = np.bincount(pairs[:, 1] - ds.feature_base, minlength=ds.n_features)
    assert sizes.min() > 65 and {127, 128, 129} <= set(sizes.tolist())
    plain = [f for f in range(ds.n_features) if sizes[f] not in (127, 128, 129)][:4]
    drop = np.zeros(len(pairs), bool)
    for f, keep in zip(plain, (65, 64, 63, 1)):
        drop[np.flatnonzero(pairs[:, 1] == ds.feature_base + f)[keep:]] = True
    left = np.bincount(pairs[~drop][:, 1] - ds.feature_base, minlength=ds.n_features)
    assert [int(left[f]) for f in plain] == [65, 64, 63, 1] and {128, 129} <= set(left.tolist())
    nb, n_blocks = layout_of(pairs[~drop])
    gs, os_ = stores(ds)
    q = quads(ds, pairs[drop][:, 0], ds.pred[PF], pairs[drop][:, 1])
    assert gs.remove(*q) == os_.remove(*q) == int(drop.sum())
    rng = np.random.default_rng(33)
    r = Runner(torch_cuda, gs, os_, ds)
    s = until_steady(r, ds, rng)[-1]
    if not ENGINE_TOGGLED:
        assert s.cached(nb, n_blocks), s.why()


@gpu
def test_two_literal_sets_on_one_store(small, torch_cuda):
    """The verdicts depend on the plan's literals: two plans with different widths keep two tables on the slice, each built once, and
    neither replaces the other's (a plan that lost its table would build it again)."""
    ds, gs, os_, (nb, n_blocks) = small
    rng = np.random.default_rng(34)
    a, b = Runner(torch_cuda, gs, os_, ds), Runner(torch_cuda, gs, os_, ds, w1=7, w2=900)
    seen = []
    for step in range(8):
        params = batch_of(ds, rng, 1300 + step)
        seen.append((a.run(params), b.run(params)))
    if not ENGINE_TOGGLED:
        for pair in seen[-3:]:
            for s in pair:
                assert s.cached(nb, n_blocks), s.why()
        assert sum(sa.built for sa, _ in seen) <= 1                 # (the defaults' table may be on the store from an earlier test)
        assert sum(sb.built for _, sb in seen) == 1                 # w1 = 7, w2 = 900 is this test's alone: its table was built here, once


@gpu
def test_mutation_and_drop_tables(torch_cuda):
    """A mutation of the operand slice (60 products lose numeric1, 60 others get a new value) drops the verdicts with the store version:
    the next executions answer like the oracle on the new store, where stale bits would not, and come back to the cached form;
    drop_tables makes the next step build the table inside the step, the one after finds it."""
    ds = bsbm.generate(2000, seed=15)
    nb, n_blocks = layout_of(feature_pairs(ds))
    gs, os_ = stores(ds)
    rng = np.random.default_rng(35)
    r = Runner(torch_cuda, gs, os_, ds)
    s = until_steady(r, ds, rng)[-1]
    if not ENGINE_TOGGLED:
        assert s.cached(nb, n_blocks), s.why()
    touched = [ds.product(int(i)) for i in rng.choice(ds.n_products, 120, replace=False)]
    sel = (ds.p == ds.pred[NUM1]) & np.isin(ds.s, touched)
    old = [c[sel] for c in (ds.g, ds.s, ds.p, ds.o)]
    assert gs.remove(*old) == os_.remove(*old) == 120
    moved = np.array(touched[60:], dtype=np.uint32)
    new = quads(ds, moved, ds.pred[NUM1], ds.int_base + rng.integers(0, 2000, 60))
    assert gs.extend(*new) == os_.extend(*new) == 60
    others = sorted(set(range(ds.n_products)) - {x - ds.product_base for x in touched})
    for step in range(6):
        params = batch_of(ds, rng, 1400 + step, among=others)      # (no product twice: a repeated one would close the in-place route)
        params[1][:40] = touched[:20] + touched[60:80]             # products without the stage row, and products whose windows moved
        s = r.run(params)
    if ENGINE_TOGGLED:
        return
    assert s.cached(nb, n_blocks), s.why()
    gs.drop_tables()
    s = r.run(batch_of(ds, rng, 1410))
    assert s.built and s.m.exact_reruns == 0, s.why()
    s = r.run(batch_of(ds, rng, 1420))
    assert s.cached(nb, n_blocks), s.why()


@gpu
def test_the_cap(torch_cuda):
    """BAND_PAIR_CACHE_BLOCKS one below the layout's blocks: no verdicts are built, the steps keep the pair test over the cached windows.
    At exactly the layout's blocks (the cap is inclusive) a plan on a fresh store builds and uses them."""
    ds = bsbm.generate(2000, seed=17)
    nb, n_blocks = layout_of(feature_pairs(ds))
    assert rf.band_pair_cache_eligible(n_blocks, cap_blocks=n_blocks) and not rf.band_pair_cache_eligible(n_blocks, cap_blocks=n_blocks - 1)
    rng = np.random.default_rng(36)
    gs, os_ = stores(ds)
    seen = until_steady(Runner(torch_cuda, gs, os_, ds, {"BAND_PAIR_CACHE_BLOCKS": n_blocks - 1}), ds, rng)
    if not ENGINE_TOGGLED:
        assert not any(s.built for s in seen) and seen[-1].pair_test(nb), seen[-1].why()
    gs, os_ = stores(ds)
    seen = until_steady(Runner(torch_cuda, gs, os_, ds, {"BAND_PAIR_CACHE_BLOCKS": n_blocks}), ds, rng)
    if not ENGINE_TOGGLED:
        assert sum(s.built for s in seen) == 1 and seen[-1].cached(nb, n_blocks), seen[-1].why()
