"""The band join of the batched Q5 emitting its rows from the slice's LIST of surviving pairs (band_join.hip, band_pair_list_*_kernel and
band_emit_kernel's list form; store.hpp, SliceTable::BandRowWindows::pair_list): the set bits of the cached verdicts, block by block, in the
order the emit pass writes the rows.  A step filters the list by "this row has a value in this execution" and compacts each round of 64.
Every step is compared with the oracle as a multiset; against the bits form (NO_BAND_PAIR_LIST) the fetched columns are compared element by
element.  Which form ran shows in the bytes recorded for the band_emit_kernel class: both forms record 16 bytes per slice row and 12 per output
row for this plan, the list form 2 bytes per survivor and 4 per block + 4 on top (band_list_cases restates the pair test to count them)."""
import numpy as np
import pytest

from rdf_fusion_amd import bsbm
import rdf_fusion_amd as rf
import kat_util as ku
import band_list_cases as bl
import test_gpu_band_pair_cache as pc

gpu = pytest.mark.gpu

ENGINE_TOGGLED = pc.ENGINE_TOGGLED
EMIT, BUILD_LIST = "band_emit_kernel", "band_pair_list_write_kernel"
NUM1 = bl.NUM1


class Step(pc.Step):
    def __init__(self, m, stats, cols):
        super().__init__(m, stats)
        emit = [nbytes for name, launches, ms, nbytes, rows in stats if EMIT in name]
        self.emit_bytes = emit[0] if emit else None
        self.cols, self.n_out = cols, len(cols[0])
        self.built_list = any(BUILD_LIST in k for k in self.ran)

    def extra(self, nb):
        """what the emit pass records beyond the slice's rows and the output rows"""
        return None if self.emit_bytes is None else self.emit_bytes - 16 * nb - 12 * self.n_out

    def listed(self, nb, n_blocks, per):
        return self.cached(nb, n_blocks) and self.extra(nb) == bl.list_bytes(per)

    def bits(self, nb, n_blocks):
        return self.cached(nb, n_blocks) and self.extra(nb) == 0

    def why(self):
        return super().why() + (self.emit_bytes, self.n_out)


class Runner(pc.Runner):
    def run(self, params):
        """one step, checked against the oracle"""
        keep, ptrs = pc.on_device(self.torch, params)
        self.plan.bind_table(0, ptrs, len(params[0]))
        got = self.plan.execute().fetch()
        exp, n_exp, _ = self.os_.execute(self.desc, [params])
        assert len(got[0]) == n_exp
        np.testing.assert_array_equal(ku.multiset(got), ku.multiset(exp, n_exp))
        return Step(self.plan.metrics(), self.plan.kernel_stats(), got)


def until_steady(r, ds, rng, n=1400, steps=8):
    return [r.run(pc.batch_of(ds, rng, n + step)) for step in range(steps)]


@pytest.fixture(scope="module")
def small(torch_cuda):
    ds = bsbm.generate(2000)
    gs, os_ = pc.stores(ds)
    pairs = bl.feature_pairs(ds)
    return ds, gs, os_, pc.layout_of(pairs), pairs


@gpu
def test_same_arrays_as_the_bits_form(small, torch_cuda):
    """Eight batches (ids that are no product's on odd steps) through a default plan and one with NO_BAND_PAIR_LIST on the same store: both
    answer like the oracle; in the steady steps their columns are equal element by element, order included.  The default plan's last steps
    record the list form; the other plan never builds a list nor uses the one the first left."""
    ds, gs, os_, (nb, n_blocks), pairs = small
    per = bl.block_survivors(ds, pairs, 120, 170)
    assert len(per) == n_blocks
    rng = np.random.default_rng(41)
    a, b = Runner(torch_cuda, gs, os_, ds), Runner(torch_cuda, gs, os_, ds, {"NO_BAND_PAIR_LIST": 1})
    seen_a, seen_b = [], []
    for step in range(8):
        params = pc.batch_of(ds, rng, 1500 - 20 * step, foreign=40 if step % 2 else 0)
        seen_a.append(a.run(params))
        seen_b.append(b.run(params))
    if ENGINE_TOGGLED:
        return
    for sa, sb in zip(seen_a[-4:], seen_b[-4:]):
        assert sa.listed(nb, n_blocks, per), sa.why()
        assert sb.bits(nb, n_blocks), sb.why()
        assert len(sa.cols) == len(sb.cols) == 3
        for ca, cb in zip(sa.cols, sb.cols):
            np.testing.assert_array_equal(ca, cb)
    assert sum(s.built_list for s in seen_a) <= 1                   # (none at all when an earlier test's plan left the list on the store)
    assert not any(s.built_list for s in seen_b), [s.why() for s in seen_b if s.built_list]


@gpu
def test_rows_entering_and_leaving(torch_cuda):
    """Two batches of 1 500 products that share 1 000 on alternate steps: a row valid in one step is not in the next.  Then a batch chosen from
    the slice's own order: one feature group's rows 0 .. 63 all without an instance (rounds in which no item counts), another group's second
    chunk of rows with exactly one.  A repeated product takes the exact re-run on the counted route; the batches after it are back on the list."""
    ds = bsbm.generate(2000, seed=12)
    pairs = bl.feature_pairs(ds)
    nb, n_blocks = pc.layout_of(pairs)
    per = bl.block_survivors(ds, pairs, 120, 170)
    gs, os_ = pc.stores(ds)
    rng = np.random.default_rng(42)
    r = Runner(torch_cuda, gs, os_, ds)
    s = until_steady(r, ds, rng)[-1]
    if not ENGINE_TOGGLED:
        assert s.listed(nb, n_blocks, per), s.why()
    order = rng.permutation(ds.n_products)
    halves = [[ds.product(int(i)) for i in order[:1500]], [ds.product(int(i)) for i in order[500:]]]
    seen = [r.run(pc.batch_with(halves[step % 2])) for step in range(6)]
    rows = pairs[np.lexsort((pairs[:, 0], pairs[:, 1]))]             # the slice's order: by feature, then product
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
    seen.append(r.run(pc.batch_with(ids)))
    if not ENGINE_TOGGLED:
        for s in seen:
            assert s.listed(nb, n_blocks, per), s.why()
    twice = list(halves[0])
    twice[7] = twice[900]
    s = r.run(pc.batch_with(twice))                                             # (equal to the oracle, like every step)
    if not ENGINE_TOGGLED:
        assert s.m.exact_reruns >= 1 and not s.cached(nb, n_blocks), s.why()
    after = [r.run(pc.batch_with(halves[step % 2])) for step in range(3)]
    if not ENGINE_TOGGLED:
        assert after[1].listed(nb, n_blocks, per) and after[2].listed(nb, n_blocks, per), (after[1].why(), after[2].why())


@gpu
def test_group_and_block_edges(torch_cuda):
    """Feature groups cut to 65, 64, 63 rows and to one row beside the store's own groups of 127, 128 and 129 rows."""
    ds = bsbm.generate(2000)
    pairs = bl.feature_pairs(ds)
    sizes = np.bincount(pairs[:, 1] - ds.feature_base, minlength=ds.n_features)
    assert sizes.min() > 65 and {127, 128, 129} <= set(sizes.tolist())
    plain = [f for f in range(ds.n_features) if sizes[f] not in (127, 128, 129)][:4]
    drop = np.zeros(len(pairs), bool)
    for f, keep in zip(plain, (65, 64, 63, 1)):
        drop[np.flatnonzero(pairs[:, 1] == ds.feature_base + f)[keep:]] = True
    nb, n_blocks = pc.layout_of(pairs[~drop])
    per = bl.block_survivors(ds, pairs[~drop], 120, 170)
    assert len(per) == n_blocks
    gs, os_ = pc.stores(ds)
    q = pc.quads(ds, pairs[drop][:, 0], ds.pred[bl.PF], pairs[drop][:, 1])
    assert gs.remove(*q) == os_.remove(*q) == int(drop.sum())
    rng = np.random.default_rng(43)
    r = Runner(torch_cuda, gs, os_, ds)
    seen = until_steady(r, ds, rng)
    if not ENGINE_TOGGLED:
        assert seen[-1].listed(nb, n_blocks, per) and seen[-2].listed(nb, n_blocks, per), seen[-1].why()


@gpu
def test_empty_blocks_and_short_lists(small, torch_cuda):
    """w1 = 7, w2 = 900 on the same store: 24 blocks without a survivor (equal offsets: the wave leaves before its second round trip), blocks of
    one and of 64 (band_list_cases; the CPU test asserts these facts), lists far shorter than a round on average."""
    ds, gs, os_, (nb, n_blocks), pairs = small
    per = bl.block_survivors(ds, pairs, 7, 900)
    assert int((per == 0).sum()) == 24 and {1, 64} <= set(per.tolist())
    rng = np.random.default_rng(47)
    seen = until_steady(Runner(torch_cuda, gs, os_, ds, w1=7, w2=900), ds, rng, steps=6)
    if not ENGINE_TOGGLED:
        assert seen[-1].listed(nb, n_blocks, per) and seen[-2].listed(nb, n_blocks, per), seen[-1].why()


@gpu
def test_output_capacity(small, torch_cuda):
    """A steady run of batches of about 1 100 instances, then one of 1 990: the output capacity is speculated as the last step's rows + 25 % + 256
    (Plan::run_speculative), and the big batch has more rows than that, so its first execution runs the list form out of room in the middle of
    a block and the plan re-runs.  The count stays exact (the fetched rows are the oracle's, no more and no fewer), and the rows are right — also
    those of the bits-form plan beside it and of the steps after it, whose buffers a write past the capacity would have hit."""
    ds, gs, os_, (nb, n_blocks), pairs = small
    per = bl.block_survivors(ds, pairs, 120, 170)
    rng = np.random.default_rng(44)
    a, b = Runner(torch_cuda, gs, os_, ds), Runner(torch_cuda, gs, os_, ds, {"NO_BAND_PAIR_LIST": 1})
    for step in range(6):
        params = pc.batch_of(ds, rng, 1100 + step)
        sa, sb = a.run(params), b.run(params)
    if not ENGINE_TOGGLED:
        assert sa.listed(nb, n_blocks, per) and sb.bits(nb, n_blocks), (sa.why(), sb.why())
    big = pc.batch_of(ds, rng, 1990)
    ba, bb = a.run(big), b.run(big)
    assert ba.n_out == bb.n_out and ba.n_out > sa.n_out + sa.n_out // 4 + 256       # more rows than the speculated capacity
    np.testing.assert_array_equal(ku.multiset(ba.cols), ku.multiset(bb.cols))
    if not ENGINE_TOGGLED:
        assert ba.m.exact_reruns >= 1 and bb.m.exact_reruns >= 1, (ba.why(), bb.why())
    for step in range(2):
        params = pc.batch_of(ds, rng, 1100 + step)
        sa, sb = a.run(params), b.run(params)
        for ca, cb in zip(sa.cols, sb.cols):
            np.testing.assert_array_equal(ca, cb)
    if not ENGINE_TOGGLED:
        assert sa.listed(nb, n_blocks, per), sa.why()


@gpu
def test_declined_by_the_condition(small, torch_cuda):
    """w1 = w2 = 900 passes 2 563 pairs per block on average: ten times what the bits cost.  No list is built: the plan counts the pairs once
    behind its verdicts (the list is sized by the condition's bound, so the count and write kernels run, and the write kernel stores nothing:
    `built_list` says "the build kernels ran", not "a list was published"), publishes none — its build step counts two tables, the windows
    and the verdicts — remembers that, and stays on the bits form with the cached mask pass as pinned; the default plan beside it keeps its list."""
    ds, gs, os_, (nb, n_blocks), pairs = small
    per, wide = bl.block_survivors(ds, pairs, 120, 170), bl.block_survivors(ds, pairs, 900, 900)
    assert rf.band_pair_list_eligible(int(per.sum()), n_blocks) and not rf.band_pair_list_eligible(int(wide.sum()), n_blocks)
    rng = np.random.default_rng(45)
    a, b = Runner(torch_cuda, gs, os_, ds), Runner(torch_cuda, gs, os_, ds, w1=900, w2=900)
    seen = []
    for step in range(6):
        params = pc.batch_of(ds, rng, 1300 + step)
        seen.append((a.run(params), b.run(params)))
    if ENGINE_TOGGLED:
        return
    for sa, sb in seen[-2:]:
        assert sa.listed(nb, n_blocks, per), sa.why()
        assert sb.bits(nb, n_blocks), sb.why()
    built = [sb for _, sb in seen if sb.built]
    assert len(built) == 1 and built[0].m.tables_built == 2, [s.why() for s in built]     # w1 = w2 = 900 is this test's alone
    assert sum(sb.built_list for _, sb in seen) == 1                                        # counted once, remembered as declined


@gpu
def test_mutation_and_drop_tables(torch_cuda):
    """A mutation of the operand slice (60 products lose numeric1, 60 others get a new value) drops the list with the verdicts: the next
    executions answer like the oracle on the new store, where a stale list would not, and come back to the list of the new store.
    drop_tables makes the next step build verdicts and list inside the step, without a re-run; the one after is steady on the list."""
    ds = bsbm.generate(2000, seed=15)
    pairs = bl.feature_pairs(ds)
    nb, n_blocks = pc.layout_of(pairs)
    per = bl.block_survivors(ds, pairs, 120, 170)
    gs, os_ = pc.stores(ds)
    rng = np.random.default_rng(46)
    r = Runner(torch_cuda, gs, os_, ds)
    s = until_steady(r, ds, rng)[-1]
    if not ENGINE_TOGGLED:
        assert s.listed(nb, n_blocks, per), s.why()
    touched = [ds.product(int(i)) for i in rng.choice(ds.n_products, 120, replace=False)]
    sel = (ds.p == ds.pred[NUM1]) & np.isin(ds.s, touched)
    old = [c[sel] for c in (ds.g, ds.s, ds.p, ds.o)]
    assert gs.remove(*old) == os_.remove(*old) == 120
    moved = np.array(touched[60:], dtype=np.uint32)
    new = pc.quads(ds, moved, ds.pred[NUM1], ds.int_base + rng.integers(0, 2000, 60))
    assert gs.extend(*new) == os_.extend(*new) == 60
    v1 = bl.numeric(ds, NUM1)
    v1[np.array(touched[:60]) - ds.product_base] = bl.NONE
    v1[moved.astype(np.int64) - ds.product_base] = new[3].astype(np.int64) - ds.int_base + 1
    per_new = bl.block_survivors(ds, pairs, 120, 170, v1=v1)
    assert per_new.sum() != per.sum()
    others = sorted(set(range(ds.n_products)) - {x - ds.product_base for x in touched})
    for step in range(6):
        params = pc.batch_of(ds, rng, 1400 + step, among=others)   # (no product twice: a repeated one would close the in-place route)
        params[1][:40] = touched[:20] + touched[60:80]             # products without the stage row, and products whose windows moved
        s = r.run(params)
    if ENGINE_TOGGLED:
        return
    assert s.listed(nb, n_blocks, per_new), s.why()
    gs.drop_tables()
    s = r.run(pc.batch_of(ds, rng, 1410))
    assert s.built and s.built_list and s.m.exact_reruns == 0, s.why()
    s = r.run(pc.batch_of(ds, rng, 1420))
    assert s.listed(nb, n_blocks, per_new), s.why()
