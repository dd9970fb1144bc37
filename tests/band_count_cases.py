"""The per-row counts of the batched Q5's cached pair verdicts restated with numpy, beside band_list_cases.block_survivors: for every 64 x 64
block of the in-place layout and every row of it, how many of the block's entries survive both windows.  That is the popcount of the row's
cached word, the byte SliceTable::BandRowWindows::pair_cnt keeps and band_mask_kernel's counts form adds up.  And the store on which some
rows count all 64 entries.  Shared by the CPU facts and the GPU route checks."""
import numpy as np

import band_list_cases as bl


def row_counts(ds, pairs, w1, w2, v1=None, v2=None):
    """[n_blocks, 64] in the layout's order (block_survivors'): entry [blk, r] = surviving entries of row r of block blk (0 past the block's rows)"""
    v1 = bl.numeric(ds, bl.NUM1) if v1 is None else v1
    v2 = bl.numeric(ds, bl.NUM2) if v2 is None else v2
    rows = pairs[np.lexsort((pairs[:, 0], pairs[:, 1]))]
    cuts = np.flatnonzero(np.diff(rows[:, 1])) + 1
    out = []
    for group in np.split(rows[:, 0].astype(np.int64) - ds.product_base, cuts):
        a, b = v1[group], v2[group]
        has = (a != bl.NONE) & (b != bl.NONE)
        m = (np.abs(a[:, None] - a[None, :]) < w1) & (np.abs(b[:, None] - b[None, :]) < w2) & has[:, None] & has[None, :]
        np.fill_diagonal(m, False)                                   # m[r, e]
        n = len(group)
        for eb in range(0, n, 64):
            for rb in range(0, n, 64):
                c = np.zeros(64, np.int64)
                c[:min(64, n - rb)] = m[rb:rb + 64, eb:eb + 64].sum(axis=1)
                out.append(c)
    return np.array(out, dtype=np.int64)


def largest_group(ds, pairs):
    """(feature index, product ids) of the largest feature group"""
    sizes = np.bincount(pairs[:, 1] - ds.feature_base, minlength=ds.n_features)
    f = int(sizes.argmax())
    return f, pairs[pairs[:, 1] == ds.feature_base + f][:, 0]


def full_rows_edit(ds, pairs, value1=500, value2=700):
    """Every product of the largest feature group gets the same numeric1 and the same numeric2 literal: (quads to remove, quads to extend, v1, v2
    of the store afterwards).  The group's off-diagonal blocks are then full: every row of them counts 64."""
    _, products = largest_group(ds, pairs)
    sel = np.isin(ds.p, [ds.pred[bl.NUM1], ds.pred[bl.NUM2]]) & np.isin(ds.s, products)
    old = [c[sel] for c in (ds.g, ds.s, ds.p, ds.o)]
    n = len(products)
    new = [np.zeros(2 * n, np.uint32), np.concatenate([products, products]).astype(np.uint32),
           np.concatenate([np.full(n, ds.pred[bl.NUM1]), np.full(n, ds.pred[bl.NUM2])]).astype(np.uint32),
           np.concatenate([np.full(n, ds.int_base + value1 - 1), np.full(n, ds.int_base + value2 - 1)]).astype(np.uint32)]
    v1, v2 = bl.numeric(ds, bl.NUM1), bl.numeric(ds, bl.NUM2)
    at = products.astype(np.int64) - ds.product_base
    v1[at], v2[at] = value1, value2
    return old, new, v1, v2


def edge_store_pairs(ds, pairs):
    """Four feature groups cut to 65, 64, 63 rows and to one row beside the store's own groups of 127, 128 and 129 rows: (pairs kept, pairs dropped)"""
    sizes = np.bincount(pairs[:, 1] - ds.feature_base, minlength=ds.n_features)
    assert sizes.min() > 65 and {127, 128, 129} <= set(sizes.tolist())
    plain = [f for f in range(ds.n_features) if sizes[f] not in (127, 128, 129)][:4]
    drop = np.zeros(len(pairs), bool)
    for f, keep in zip(plain, (65, 64, 63, 1)):
        drop[np.flatnonzero(pairs[:, 1] == ds.feature_base + f)[keep:]] = True
    return pairs[~drop], pairs[drop]
