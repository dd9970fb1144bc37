"""The pair test of the batched Q5's band join restated with numpy, block by block of the in-place layout (band_join.hip): how many
pairs of every 64 x 64 block survive both windows.  That is the number of set bits in the slice's cached verdicts, hence the length of
the block's list of surviving pairs (SliceTable::BandRowWindows::pair_list).  Shared by the CPU facts and the GPU route checks."""
import numpy as np

PF, NUM1, NUM2 = "bsbm:productFeature", "bsbm:productPropertyNumeric1", "bsbm:productPropertyNumeric2"
NONE = np.iinfo(np.int64).min


def feature_pairs(ds):
    """the productFeature slice as the store holds it: distinct (product, feature) pairs"""
    sel = ds.p == ds.pred[PF]
    return np.unique(np.stack([ds.s[sel], ds.o[sel]], axis=1), axis=0)


def numeric(ds, name, s=None, p=None, o=None):
    """value of property `name` by product index (NONE: the product has none); s, p, o: the store's quads when they are not the dataset's"""
    s, p, o = (ds.s, ds.p, ds.o) if s is None else (s, p, o)
    out = np.full(ds.n_products, NONE, np.int64)
    sel = p == ds.pred[name]
    out[s[sel].astype(np.int64) - ds.product_base] = o[sel].astype(np.int64) - ds.int_base + 1
    return out


def block_survivors(ds, pairs, w1, w2, v1=None, v2=None):
    """Survivors of every block, in the layout's order (feature groups ascending; within a group entry chunk major, then row chunk): the
    pair (row r, entry e) of a group survives when r != e, both products have both values, |v1[e] - v1[r]| < w1 and |v2[e] - v2[r]| < w2."""
    v1 = numeric(ds, NUM1) if v1 is None else v1
    v2 = numeric(ds, NUM2) if v2 is None else v2
    rows = pairs[np.lexsort((pairs[:, 0], pairs[:, 1]))]             # the slice's order: by feature, then product
    cuts = np.flatnonzero(np.diff(rows[:, 1])) + 1
    out = []
    for group in np.split(rows[:, 0].astype(np.int64) - ds.product_base, cuts):
        a, b = v1[group], v2[group]
        has = (a != NONE) & (b != NONE)
        m = (np.abs(a[:, None] - a[None, :]) < w1) & (np.abs(b[:, None] - b[None, :]) < w2) & has[:, None] & has[None, :]
        np.fill_diagonal(m, False)                                   # m[r, e]
        n = len(group)
        for eb in range(0, n, 64):
            for rb in range(0, n, 64):
                out.append(int(m[rb:rb + 64, eb:eb + 64].sum()))
    return np.array(out, dtype=np.int64)


def list_bytes(per_block):
    """what the list form of the emit pass records for the list: 2 bytes per survivor and the blocks' offsets"""
    return 2 * int(per_block.sum()) + 4 * (len(per_block) + 1)
