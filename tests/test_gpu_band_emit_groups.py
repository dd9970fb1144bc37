"""The grouped list form of the band join's emit pass (band_join.hip, band_emit_list): a wave owns kBandEmitGroup consecutive blocks of the
in-place layout, reads their lists as one contiguous range and writes their rows as one contiguous range from bofs[first block].  Every step
is compared with the oracle as a multiset; in the steady steps the fetched columns are compared element by element with a plan that keeps the
bits form (NO_BAND_PAIR_LIST) on the same store, and the default plan must record the list form.  What the stores and batches have — partial
last groups, groups that mix two keys' blocks, whole groups in which nothing counts, groups longer than the prefetch, the capacity running
out past a group's first block — is asserted without a device in test_band_emit_groups_cpu."""
import numpy as np
import pytest

from rdf_fusion_amd import bsbm
import rdf_fusion_amd as rf
import kat_util as ku
import band_list_cases as bl
import band_group_cases as bg
import test_gpu_band_pair_cache as pc
from test_gpu_band_pair_list import Runner, Step, until_steady          # noqa: F401  (Step: what Runner.run returns)

gpu = pytest.mark.gpu

ENGINE_TOGGLED = pc.ENGINE_TOGGLED
G, AHEAD = bg.constants()


def both(torch_cuda, gs, os_, ds, **windows):
    """the default plan and the bits-form plan on one store"""
    return Runner(torch_cuda, gs, os_, ds, **windows), Runner(torch_cuda, gs, os_, ds, {"NO_BAND_PAIR_LIST": 1}, **windows)


def run_both(a, b, params):
    sa, sb = a.run(params), b.run(params)
    return sa, sb


def same_arrays(sa, sb):
    assert len(sa.cols) == len(sb.cols) == 3
    for ca, cb in zip(sa.cols, sb.cols):
        np.testing.assert_array_equal(ca, cb)


def steady_pair(a, b, ds, rng, nb, n_blocks, per, n=1400, steps=7, check=2):
    """`steps` batches through both plans; the last `check` are steady: the list form on one side, the bits form on the other, equal arrays"""
    seen = [run_both(a, b, pc.batch_of(ds, rng, n + step)) for step in range(steps)]
    for sa, sb in seen[-check:]:
        if not ENGINE_TOGGLED:
            assert sa.listed(nb, n_blocks, per), sa.why()
            assert sb.bits(nb, n_blocks), sb.why()
            same_arrays(sa, sb)
    return seen


def cut_store(ds, pairs, drop):
    gs, os_ = pc.stores(ds)
    q = pc.quads(ds, pairs[drop][:, 0], ds.pred[bl.PF], pairs[drop][:, 1])
    assert gs.remove(*q) == os_.remove(*q) == int(drop.sum())
    return gs, os_


@pytest.fixture(scope="module")
def small(torch_cuda):
    ds = bsbm.generate(2000)
    gs, os_ = pc.stores(ds)
    pairs = bl.feature_pairs(ds)
    return ds, gs, os_, pc.layout_of(pairs), pairs


@gpu
def test_partial_last_group(torch_cuda):
    """1 389 blocks — odd, so the last group is partial for every candidate G — on a store with one feature group cut to a single block"""
    ds = bsbm.generate(2000)
    pairs = bl.feature_pairs(ds)
    drop = bg.odd_cut(ds, pairs)
    kept = pairs[~drop]
    nb, n_blocks = pc.layout_of(kept)
    assert n_blocks == 1389
    gs, os_ = cut_store(ds, pairs, drop)
    a, b = both(torch_cuda, gs, os_, ds)
    steady_pair(a, b, ds, np.random.default_rng(62), nb, n_blocks, bl.block_survivors(ds, kept, 120, 170))


@gpu
def test_block_count_a_multiple_of_every_group_size(small, torch_cuda):
    """the store as generated: 1 392 blocks, a multiple of 8 — no partial group for any candidate G"""
    ds, gs, os_, (nb, n_blocks), pairs = small
    assert n_blocks == 1392 and n_blocks % 8 == 0
    a, b = both(torch_cuda, gs, os_, ds)
    steady_pair(a, b, ds, np.random.default_rng(61), nb, n_blocks, bl.block_survivors(ds, pairs, 120, 170))


@gpu
def test_groups_straddling_keys(torch_cuda):
    """The first feature group cut to 64 rows, one block: the four-block keys behind it start one block off, so a group holds blocks of two
    keys with different entries, rows and counts of both.  A key of 129 rows (3 x 3 blocks) and one of a single row lie in such groups too."""
    ds = bsbm.generate(2000)
    pairs = bl.feature_pairs(ds)
    drop, first, one = bg.straddle_cut(ds, pairs)
    kept = pairs[~drop]
    nb, n_blocks = pc.layout_of(kept)
    assert n_blocks == 1386
    gs, os_ = cut_store(ds, pairs, drop)
    a, b = both(torch_cuda, gs, os_, ds)
    steady_pair(a, b, ds, np.random.default_rng(63), nb, n_blocks, bl.block_survivors(ds, kept, 120, 170))


@gpu
def test_nothing_counts_in_a_whole_group(small, torch_cuda):
    """Batches without any product of two adjacent feature groups: their lists are full, none of their items counts, whole groups of blocks
    emit nothing, and the groups behind them still start at the right offsets.  Then w1 = 7, w2 = 900 on the same store: empty lists
    inside groups that have items from their other blocks."""
    ds, gs, os_, (nb, n_blocks), pairs = small
    per = bl.block_survivors(ds, pairs, 120, 170)
    feats, prods, b0, nblk = bg.silent_features(ds, pairs, G)
    others = sorted(set(range(ds.n_products)) - {int(p) - ds.product_base for p in prods})
    rng = np.random.default_rng(64)
    a, b = both(torch_cuda, gs, os_, ds)
    seen = [run_both(a, b, pc.batch_of(ds, rng, 1400 + step, among=others)) for step in range(7)]
    for sa, sb in seen[-2:]:
        if not ENGINE_TOGGLED:
            assert sa.listed(nb, n_blocks, per) and sb.bits(nb, n_blocks), (sa.why(), sb.why())
            same_arrays(sa, sb)
    sa, sb = run_both(a, b, pc.batch_of(ds, rng, 1500))                          # and with their products back
    if not ENGINE_TOGGLED:
        assert sa.listed(nb, n_blocks, per), sa.why()
        same_arrays(sa, sb)
    narrow = bl.block_survivors(ds, pairs, 7, 900)
    assert int((narrow == 0).sum()) == 24
    a, b = both(torch_cuda, gs, os_, ds, w1=7, w2=900)
    steady_pair(a, b, ds, rng, nb, n_blocks, narrow)


@gpu
def test_a_group_longer_than_the_prefetch(small, torch_cuda):
    """Windows chosen on the CPU so that the list stays eligible and groups hold more than 64 * kBandEmitAhead items: their further rounds come
    from memory, a round trip at a time."""
    ds, gs, os_, (nb, n_blocks), pairs = small
    w1, w2, per = bg.long_group_windows(ds, pairs, G, AHEAD, rf.band_pair_list_eligible)
    assert np.add.reduceat(per, np.arange(0, len(per), G)).max() > 64 * AHEAD
    a, b = both(torch_cuda, gs, os_, ds, w1=w1, w2=w2)
    steady_pair(a, b, ds, np.random.default_rng(66), nb, n_blocks, per, n=1900)   # (nearly every product: nearly every item counts)


@gpu
def test_capacity_runs_out_inside_a_group(small, torch_cuda):
    """The recipe of test_gpu_band_pair_list.test_output_capacity with a seed for which the big batch crosses the speculated capacity in
    block 953 (test_band_emit_groups_cpu): not the first block of its group for any candidate G.  The count stays exact, the plan re-runs,
    the rows equal the bits-form plan's, and the steps after it are right too."""
    ds, gs, os_, (nb, n_blocks), pairs = small
    per = bl.block_survivors(ds, pairs, 120, 170)
    rng = np.random.default_rng(bg.CAPACITY_SEED)
    a, b = both(torch_cuda, gs, os_, ds)
    for step in range(6):
        sa, sb = run_both(a, b, pc.batch_of(ds, rng, 1100 + step))
    if not ENGINE_TOGGLED:
        assert sa.listed(nb, n_blocks, per) and sb.bits(nb, n_blocks), (sa.why(), sb.why())
        same_arrays(sa, sb)
    ba, bb = run_both(a, b, pc.batch_of(ds, rng, 1990))
    assert ba.n_out == bb.n_out and ba.n_out > sa.n_out + sa.n_out // 4 + 256       # more rows than the speculated capacity
    np.testing.assert_array_equal(ku.multiset(ba.cols), ku.multiset(bb.cols))
    if not ENGINE_TOGGLED:
        assert ba.m.exact_reruns >= 1 and bb.m.exact_reruns >= 1, (ba.why(), bb.why())
    for step in range(2):
        sa, sb = run_both(a, b, pc.batch_of(ds, rng, 1100 + step))
        same_arrays(sa, sb)
    if not ENGINE_TOGGLED:
        assert sa.listed(nb, n_blocks, per), sa.why()
