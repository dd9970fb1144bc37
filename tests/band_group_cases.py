"""The grouped list form of the band join's emit pass (band_join.hip, band_emit_list) restated with numpy, and the small stores its tests
use.  A wave owns kBandEmitGroup consecutive blocks of the in-place layout: one contiguous range of the slice's list of surviving pairs, one
contiguous range of the output.  Shared by the CPU facts (test_band_emit_groups_cpu) and the GPU checks (test_gpu_band_emit_groups)."""
import os
import re

import numpy as np

import band_list_cases as bl

SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rdf-fusion_amd", "csrc", "band_join.hip")
CAPACITY_SEED = 65                                                          # (test_band_emit_groups_cpu: the capacity recipe crosses inside block 953, odd)
WINDOWS = [(120, 170), (130, 180), (140, 190), (150, 200), (155, 210)]     # candidates for "a group longer than the prefetch", narrowest first


def constants():
    """(kBandEmitGroup, kBandEmitAhead) as band_join.hip states them"""
    text = open(SOURCE).read()
    found = [re.search(r"constexpr\s+u32\s+%s\s*=\s*(\d+)\s*;" % name, text) for name in ("kBandEmitGroup", "kBandEmitAhead")]
    assert all(found), "band_join.hip no longer states kBandEmitGroup / kBandEmitAhead"
    return tuple(int(m.group(1)) for m in found)


def slice_rows(pairs):
    """the slice's order: by feature, then product"""
    return pairs[np.lexsort((pairs[:, 0], pairs[:, 1]))]


def block_keys(pairs):
    """per block of the layout, in order: the index (in slice order) of the feature group it belongs to"""
    sizes = np.unique(pairs[:, 1], return_counts=True)[1]
    chunks = (sizes + 63) // 64
    return np.repeat(np.arange(len(sizes)), chunks * chunks)


def block_lists(ds, pairs, w1, w2):
    """Per block of the layout (feature groups ascending; within a group entry chunk major, then row chunk) its list of surviving pairs in the
    list's order — rows ascending, entries ascending within a row — as an (n, 4) array {row in block, entry in block, row's product, entry's
    product}: the pair test of band_list_cases.block_survivors, listed instead of counted."""
    v1, v2 = bl.numeric(ds, bl.NUM1), bl.numeric(ds, bl.NUM2)
    rows = slice_rows(pairs)
    cuts = np.flatnonzero(np.diff(rows[:, 1])) + 1
    out = []
    for prods in np.split(rows[:, 0].astype(np.int64), cuts):
        group = prods - ds.product_base
        a, b = v1[group], v2[group]
        has = (a != bl.NONE) & (b != bl.NONE)
        m = (np.abs(a[:, None] - a[None, :]) < w1) & (np.abs(b[:, None] - b[None, :]) < w2) & has[:, None] & has[None, :]
        np.fill_diagonal(m, False)                                   # m[r, e]
        n = len(group)
        for eb in range(0, n, 64):
            for rb in range(0, n, 64):
                r, e = np.nonzero(m[rb:rb + 64, eb:eb + 64])         # (row major: the list's order)
                out.append(np.stack([r, e, prods[rb + r], prods[eb + e]], axis=1).reshape(-1, 4))
    return out


def counts_of(lists, batch):
    """per block: the items whose row's product is in the batch (bcount of a steady step over distinct products)"""
    batch = np.asarray(sorted(set(int(x) for x in batch)), dtype=np.int64)
    return np.array([int(np.isin(items[:, 2], batch).sum()) for items in lists], dtype=np.int64)


def emit_per_block(lists, batch, cap=None):
    """The one-block form: block blk filters its own list and writes its rows from bofs[blk] on, below the capacity.  Returns (out, total):
    out[i] = {row's product, entry's product} of output row i, -1 where nothing was written."""
    batch = np.asarray(sorted(set(int(x) for x in batch)), dtype=np.int64)
    keep = [np.isin(items[:, 2], batch) for items in lists]
    bofs = np.concatenate([[0], np.cumsum([int(k.sum()) for k in keep])])
    total = int(bofs[-1])
    cap = total if cap is None else cap
    out = np.full((min(cap, total), 2), -1, np.int64)
    for blk, (items, k) in enumerate(zip(lists, keep)):
        rows = items[k][:, 2:]
        at = int(bofs[blk])
        fit = max(0, min(len(rows), len(out) - at))
        out[at:at + fit] = rows[:fit]
    return out, total


def emit_grouped(lists, batch, group, cap=None):
    """The grouped form: a wave owns `group` consecutive blocks, reads ONE contiguous range of the concatenated list, walks it in rounds of 64
    items that do not restart at block boundaries, finds an item's block by counting the inner offsets <= its position, looks the row's
    validity up in that block's table, compacts the round and stores from bofs[first block] + what the earlier rounds kept."""
    batch = np.asarray(sorted(set(int(x) for x in batch)), dtype=np.int64)
    n = len(lists)
    off = np.concatenate([[0], np.cumsum([len(items) for items in lists])])
    flat = np.concatenate(lists) if n else np.zeros((0, 4), np.int64)
    keep = [np.isin(items[:, 2], batch) for items in lists]
    bofs = np.concatenate([[0], np.cumsum([int(k.sum()) for k in keep])])
    total = int(bofs[-1])
    cap = total if cap is None else cap
    out = np.full((min(cap, total), 2), -1, np.int64)
    for g0 in range(0, n, group):
        g1 = min(g0 + group, n)                                      # (the last group is partial)
        l0, l1 = int(off[g0]), int(off[g1])
        if bofs[g1] == bofs[g0] or l1 == l0:
            continue
        # the rows' values of every block of the group that has items and rows that count: valid[i][row]; others stay "none"
        valid = np.zeros((group, 64), bool)
        for i in range(g1 - g0):
            if off[g0 + i + 1] != off[g0 + i] and bofs[g0 + i + 1] != bofs[g0 + i]:
                items = lists[g0 + i]
                valid[i, items[:, 0]] = np.isin(items[:, 2], batch)
        inner = off[g0 + 1:g1] - l0
        run = int(bofs[g0])
        for p0 in range(0, l1 - l0, 64):
            p = np.arange(p0, min(p0 + 64, l1 - l0))
            blk = (p[:, None] >= inner[None, :]).sum(axis=1) if len(inner) else np.zeros(len(p), np.int64)
            items = flat[l0 + p]
            counts = valid[blk, items[:, 0]]
            rows = items[counts][:, 2:]
            fit = max(0, min(len(rows), len(out) - run))
            out[run:run + fit] = rows[:fit]
            run += len(rows)
        assert run == bofs[g1]                                       # compaction never reorders: the next group starts where this one ended
    return out, total


def cut(ds, pairs, keep_rows):
    """drop mask over `pairs`: feature group f (index of the feature, not of the group) keeps its first keep_rows[f] pairs"""
    drop = np.zeros(len(pairs), bool)
    for f, keep in keep_rows.items():
        drop[np.flatnonzero(pairs[:, 1] == ds.feature_base + f)[keep:]] = True
    return drop


def sizes_of(ds, pairs):
    return np.bincount(pairs[:, 1] - ds.feature_base, minlength=ds.n_features)


def odd_cut(ds, pairs):
    """one four-block feature group cut to 64 rows, one block: the block count drops by three and is odd"""
    sizes = sizes_of(ds, pairs)
    f = next(f for f in range(5, ds.n_features) if 64 < sizes[f] <= 128)
    return cut(ds, pairs, {f: 64})


def straddle_cut(ds, pairs):
    """the first feature group cut to 64 rows — one block, so the four-block groups behind it all start one block off a multiple of four —
    and another cut to one row; the store's own 129-row groups (3 x 3 blocks) stay"""
    sizes = sizes_of(ds, pairs)
    first = int(np.flatnonzero(sizes)[0])
    one = next(f for f in range(first + 20, ds.n_features) if 64 < sizes[f] <= 128)
    return cut(ds, pairs, {first: 64, one: 1}), first, one


def silent_features(ds, pairs, group):
    """adjacent feature groups (two, for groups of up to four blocks) whose blocks hold a whole aligned group of `group` blocks for sure: 2 *
    group - 1 consecutive blocks.  Returns (their feature indices, their products, first block, blocks)."""
    sizes = sizes_of(ds, pairs)
    live = np.flatnonzero(sizes)
    chunks = (sizes[live] + 63) // 64
    first_block = np.concatenate([[0], np.cumsum(chunks * chunks)])
    at = 1
    n = 2
    while int(first_block[at + n] - first_block[at]) < 2 * group - 1:
        n += 1
    feats = live[at:at + n]
    prods = np.unique(pairs[np.isin(pairs[:, 1], ds.feature_base + feats), 0])
    return feats, prods, int(first_block[at]), int(first_block[at + n] - first_block[at])


def long_group_windows(ds, pairs, group, ahead, eligible):
    """the narrowest candidate windows whose list stays eligible and has a group of more than 64 * ahead items; (w1, w2, per block)"""
    for w1, w2 in WINDOWS:
        per = bl.block_survivors(ds, pairs, w1, w2)
        sums = np.add.reduceat(per, np.arange(0, len(per), group))
        if eligible(int(per.sum()), len(per)) and sums.max() > 64 * ahead:
            return w1, w2, per
    raise AssertionError("no candidate windows give a group longer than the prefetch")
