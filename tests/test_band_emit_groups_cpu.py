"""The grouped list form of the band join's emit pass (band_join.hip, band_emit_list: a wave owns kBandEmitGroup consecutive blocks): the
constants as the source states them, the facts of the small stores that test_gpu_band_emit_groups relies on, and the numpy restatement of
"group -> one contiguous list range -> compacted output from bofs[first block]" against the per-block restatement.  No device."""
import numpy as np
import pytest

import rdf_fusion_amd as rf
from rdf_fusion_amd import bsbm
import band_list_cases as bl
import band_group_cases as bg
import test_gpu_band_pair_cache as pc

G, AHEAD = bg.constants()


@pytest.fixture(scope="module")
def small():
    ds = bsbm.generate(2000)
    return ds, bl.feature_pairs(ds)


def test_constants_are_admissible():
    """G from {2, 4, 8}; LDS of the three-slot form (4 waves x 3 slots x G x 64 dwords) lets 8 workgroups share a CU's 160 KiB"""
    assert G in (2, 4, 8) and AHEAD >= 1
    assert 8 * (4 * 3 * G * 64 * 4) <= 160 * 1024


def test_block_counts_of_the_stores(small):
    ds, pairs = small
    assert pc.layout_of(pairs) == (len(pairs), 1392) and 1392 % 8 == 0          # the store as generated: a multiple of every candidate G
    odd = pairs[~bg.odd_cut(ds, pairs)]
    assert pc.layout_of(odd)[1] == 1389                                        # odd: the last group is partial for every G
    assert all(1389 % g for g in (2, 4, 8))
    drop, first, one = bg.straddle_cut(ds, pairs)
    assert pc.layout_of(pairs[~drop])[1] == 1386
    sizes = bg.sizes_of(ds, pairs[~drop])
    assert sizes[first] == 64 and sizes[one] == 1 and 129 in sizes.tolist()
    assert len(bl.block_survivors(ds, pairs[~drop], 120, 170)) == 1386


def test_groups_straddle_keys(small):
    """behind the one-block first key the four-block keys start one off a multiple of four: groups mix two keys' blocks (all of them, for
    G = 4, up to the first key that is not four blocks)"""
    ds, pairs = small
    drop, first, one = bg.straddle_cut(ds, pairs)
    keys = bg.block_keys(pairs[~drop])
    mixed = [len(set(keys[g0:g0 + G].tolist())) > 1 for g0 in range(0, len(keys), G)]
    assert sum(mixed) >= 10                                                    # (G = 2: every other group between the one-block key and the one-row key; G = 4: below)
    if G == 4:
        per_key = np.bincount(keys)
        plain = int(np.flatnonzero(per_key[1:] != 4)[0]) + 1                    # the first later key that is not four blocks
        assert plain >= 20 and all(mixed[:plain - 1])                          # (group j holds key j's last block and key j + 1's first three)
    # the 129-row key's nine blocks and the one-row key's single block both lie in groups that hold another key's blocks too
    per_key = np.bincount(keys)
    for k in (int(np.flatnonzero(per_key == 9)[0]), int(np.flatnonzero(per_key == 1)[1])):
        blocks = np.flatnonzero(keys == k)
        assert any(len(set(keys[b // G * G:b // G * G + G].tolist())) > 1 for b in blocks)


def test_a_whole_group_without_a_counting_item(small):
    ds, pairs = small
    feats, prods, b0, nblk = bg.silent_features(ds, pairs, G)
    assert len(feats) == 2 or G == 8
    inside = [g0 for g0 in range(0, 1392, G) if b0 <= g0 and g0 + G <= b0 + nblk]
    assert inside                                                              # an aligned group of G blocks wholly inside the silent keys
    assert ds.n_products - len(prods) >= 1500                                  # enough other products for a batch
    lists = bg.block_lists(ds, pairs, 120, 170)
    batch = [ds.product(i) for i in range(ds.n_products) if ds.product(i) not in set(prods.tolist())][:1400]
    counts = bg.counts_of(lists, batch)
    for g0 in inside:
        assert counts[g0:g0 + G].sum() == 0 and sum(len(x) for x in lists[g0:g0 + G]) > 0   # items, none counts
    assert counts[:b0].sum() > 0 and counts[b0 + nblk:].sum() > 0              # neighbours on both sides emit


def test_empty_lists_inside_groups(small):
    """w1 = 7, w2 = 900: 24 blocks without a survivor, none of them a whole group — their groups have items from other blocks"""
    ds, pairs = small
    per = bl.block_survivors(ds, pairs, 7, 900)
    empty = np.flatnonzero(per == 0)
    assert len(empty) == 24
    assert any(per[b // G * G:b // G * G + G].sum() > 0 for b in empty)
    assert rf.band_pair_list_eligible(int(per.sum()), len(per))


def test_a_group_longer_than_the_prefetch(small):
    ds, pairs = small
    w1, w2, per = bg.long_group_windows(ds, pairs, G, AHEAD, rf.band_pair_list_eligible)
    sums = np.add.reduceat(per, np.arange(0, len(per), G))
    assert sums.max() > 64 * AHEAD and rf.band_pair_list_eligible(int(per.sum()), len(per))
    assert sums.min() <= 64 * AHEAD                                            # (and groups that fit the prefetch beside them)
    chosen = {(2, 12): (150, 200), (4, 16): (130, 180)}                        # (the narrowest candidates that do, for constants that were measured)
    if (G, AHEAD) in chosen:
        assert (w1, w2) == chosen[(G, AHEAD)]


def test_lists_restate_the_counts(small):
    ds, pairs = small
    for w1, w2 in ((120, 170), (7, 900)):
        lists = bg.block_lists(ds, pairs, w1, w2)
        np.testing.assert_array_equal([len(x) for x in lists], bl.block_survivors(ds, pairs, w1, w2))
    assert all(((x[:, 0] < 64) & (x[:, 1] < 64)).all() for x in lists)


@pytest.mark.parametrize("store", ["plain", "odd", "straddle"])
def test_grouped_restatement_equals_the_per_block_one(small, store):
    """the same output arrays, element by element, for every candidate G — also with the output capacity running out inside a group"""
    ds, pairs = small
    if store == "odd":
        pairs = pairs[~bg.odd_cut(ds, pairs)]
    elif store == "straddle":
        pairs = pairs[~bg.straddle_cut(ds, pairs)[0]]
    rng = np.random.default_rng(51)
    for w1, w2 in ((120, 170), (7, 900)):
        lists = bg.block_lists(ds, pairs, w1, w2)
        batch = pc.batch_of(ds, rng, 1400)[1]
        exp, total = bg.emit_per_block(lists, batch)
        assert total == len(exp) and (exp >= 0).all()
        for g in (2, 4, 8):
            got, n = bg.emit_grouped(lists, batch, g)
            assert n == total
            np.testing.assert_array_equal(got, exp)
            cap = total // 2 + 7
            got, n = bg.emit_grouped(lists, batch, g, cap)
            assert n == total
            np.testing.assert_array_equal(got, bg.emit_per_block(lists, batch, cap)[0])
            np.testing.assert_array_equal(got, exp[:cap])


def test_capacity_recipe_runs_out_inside_a_group(small):
    """the recipe of the GPU test: steady batches of about 1 100, then 1 990 products with the capacity speculated from the step before (its rows
    + 25 % + 256).  The block in which the big batch crosses that capacity is not the first of its group for any candidate G (its index is odd)."""
    ds, pairs = small
    lists = bg.block_lists(ds, pairs, 120, 170)
    rng = np.random.default_rng(bg.CAPACITY_SEED)
    for step in range(6):
        last = pc.batch_of(ds, rng, 1100 + step)[1]
    big = pc.batch_of(ds, rng, 1990)[1]
    n_last = int(bg.counts_of(lists, last).sum())
    cap = n_last + n_last // 4 + 256
    counts = bg.counts_of(lists, big)
    bofs = np.concatenate([[0], np.cumsum(counts)])
    assert bofs[-1] > cap
    blk = int(np.searchsorted(bofs, cap, side="right")) - 1                    # bofs[blk] <= cap < bofs[blk + 1]
    assert bofs[blk] < cap < bofs[blk + 1] and blk % 2 == 1
