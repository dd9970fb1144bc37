"""The band join of the batched Q5 counting a steady step's blocks from the slice's per-row COUNTS (band_join.hip, band_mask_kernel's counts
form; store.hpp, SliceTable::BandRowWindows::pair_cnt): a step that emits from the list needs the cached verdicts only for bcount[blk], the
set bits of the rows that have a value in this execution, and the set bits of every row are a table beside the list, one byte each.
Every step is compared with the oracle as a multiset; against a plan with NO_BAND_PAIR_COUNTS on the same store the fetched columns are
compared element by element; that plan's steps are compared with the counts plan's, as multisets, in every step (Beside), which spares the oracle's
second run of the same batch.  Which form ran shows in the bytes recorded for the band_mask_kernel class: 84 per block + 4 per slice row from
the counts, 540 per block + 4 per slice row from the bits.  The form is taken from BAND_PAIR_COUNT_BLOCKS blocks upward (0 = 2^16: far above
these stores' 1 392), so the plans here set the bound to 1 unless they say otherwise."""
import numpy as np
import pytest

from rdf_fusion_amd import bsbm
import kat_util as ku
import band_list_cases as bl
import band_count_cases as bc
import test_gpu_band_pair_cache as pc
import test_gpu_band_pair_list as pl

gpu = pytest.mark.gpu

ENGINE_TOGGLED = pc.ENGINE_TOGGLED
COUNTS, DECLINED = {"BAND_PAIR_COUNT_BLOCKS": 1}, {"BAND_PAIR_COUNT_BLOCKS": 1, "NO_BAND_PAIR_COUNTS": 1}


def counted(s, nb, n_blocks, per):
    """a quiet step on the list whose mask pass read the counts"""
    return s.quiet() and s.mask_bytes == 84 * n_blocks + 4 * nb and s.extra(nb) == bl.list_bytes(per)


def from_bits(s, nb, n_blocks, per):
    """.. whose mask pass streamed the bits (the parent's form: pl.Step.listed pins 540 per block)"""
    return s.listed(nb, n_blocks, per)


class Beside(pl.Runner):
    """the plan run beside a counts plan on the same batches: its steps are compared with that plan's (same_rows), which answered like the oracle"""
    def run(self, params):
        keep, ptrs = pc.on_device(self.torch, params)
        self.plan.bind_table(0, ptrs, len(params[0]))
        got = self.plan.execute().fetch()
        return pl.Step(self.plan.metrics(), self.plan.kernel_stats(), got)


def same_rows(sa, sb):
    assert sa.n_out == sb.n_out
    np.testing.assert_array_equal(ku.multiset(sa.cols), ku.multiset(sb.cols))


def equal_columns(sa, sb):
    assert len(sa.cols) == len(sb.cols) == 3
    for ca, cb in zip(sa.cols, sb.cols):
        np.testing.assert_array_equal(ca, cb)


@pytest.fixture(scope="module")
def small(torch_cuda):
    ds = bsbm.generate(2000)
    gs, os_ = pc.stores(ds)
    pairs = bl.feature_pairs(ds)
    return ds, gs, os_, pc.layout_of(pairs), pairs, bl.block_survivors(ds, pairs, 120, 170)


@gpu
def test_same_arrays_as_the_bits(small, torch_cuda):
    """Eight batches (ids that are no product's on odd steps) through a counts plan and a NO_BAND_PAIR_COUNTS plan on the same store: the last
    four steps record the two byte formulas, their columns are equal element by element, each waits once, builds nothing, re-runs nothing."""
    ds, gs, os_, (nb, n_blocks), pairs, per = small
    assert len(per) == n_blocks == 1392
    rng = np.random.default_rng(51)
    a, b = pl.Runner(torch_cuda, gs, os_, ds, COUNTS), Beside(torch_cuda, gs, os_, ds, DECLINED)
    seen_a, seen_b = [], []
    for step in range(8):
        params = pc.batch_of(ds, rng, 1500 - 20 * step, foreign=40 if step % 2 else 0)
        seen_a.append(a.run(params))
        seen_b.append(b.run(params))
        same_rows(seen_a[-1], seen_b[-1])
    if ENGINE_TOGGLED:
        return
    for sa, sb in zip(seen_a[-4:], seen_b[-4:]):
        assert counted(sa, nb, n_blocks, per), sa.why()
        assert from_bits(sb, nb, n_blocks, per), sb.why()
        equal_columns(sa, sb)
        for s in (sa, sb):
            assert s.m.host_syncs == 1 and s.m.tables_built == 0 and s.m.exact_reruns == 0, s.why()


@gpu
def test_default_plan_keeps_the_bits(small, torch_cuda):
    """no option set: 1 392 blocks are below 2^16, the step streams the bits as before"""
    ds, gs, os_, (nb, n_blocks), pairs, per = small
    assert n_blocks < 1 << 16
    rng = np.random.default_rng(52)
    s = pl.until_steady(pl.Runner(torch_cuda, gs, os_, ds), ds, rng, steps=5)[-1]
    if not ENGINE_TOGGLED:
        assert from_bits(s, nb, n_blocks, per) and s.mask_bytes == 540 * n_blocks + 4 * nb, s.why()


@gpu
def test_rows_entering_and_leaving(torch_cuda):
    """The batches of test_gpu_band_pair_list's test of the same name: alternating halves; a feature group whose rows 0 .. 63 all have no
    instance (blocks that count 0); a second row chunk with exactly one valid row.  Beside a NO_BAND_PAIR_COUNTS plan, element by element.
    A repeated product re-runs exactly on the counted route; the steps after it come back to the counts."""
    ds = bsbm.generate(2000, seed=12)
    pairs = bl.feature_pairs(ds)
    nb, n_blocks = pc.layout_of(pairs)
    per = bl.block_survivors(ds, pairs, 120, 170)
    gs, os_ = pc.stores(ds)
    rng = np.random.default_rng(53)
    r, d = pl.Runner(torch_cuda, gs, os_, ds, COUNTS), Beside(torch_cuda, gs, os_, ds, DECLINED)
    for step in range(5):
        params = pc.batch_of(ds, rng, 1400 + step)
        s, sd = r.run(params), d.run(params)
        same_rows(s, sd)
    if not ENGINE_TOGGLED:
        assert counted(s, nb, n_blocks, per), s.why()
        assert from_bits(sd, nb, n_blocks, per), sd.why()
    order = rng.permutation(ds.n_products)
    halves = [[ds.product(int(i)) for i in order[:1500]], [ds.product(int(i)) for i in order[500:]]]
    batches = [pc.batch_with(halves[step % 2]) for step in range(4)]
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
    batches.append(pc.batch_with(ids))
    for params in batches:
        sa, sb = r.run(params), d.run(params)
        equal_columns(sa, sb)
        if not ENGINE_TOGGLED:
            assert counted(sa, nb, n_blocks, per), sa.why()
            assert from_bits(sb, nb, n_blocks, per), sb.why()
    twice = list(halves[0])
    twice[7] = twice[900]
    s = r.run(pc.batch_with(twice))                                             # (equal to the oracle, like every step)
    if not ENGINE_TOGGLED:
        assert s.m.exact_reruns >= 1 and not s.quiet(), s.why()
    after = [r.run(pc.batch_with(halves[step % 2])) for step in range(3)]
    if not ENGINE_TOGGLED:
        assert counted(after[1], nb, n_blocks, per) and counted(after[2], nb, n_blocks, per), (after[1].why(), after[2].why())
    sd = d.run(pc.batch_with(halves[0]))                                        # (the same batch as after[2])
    equal_columns(after[2], sd)


@gpu
def test_group_and_block_edges(torch_cuda):
    """The store of test_gpu_band_pair_list's test of the same name: groups of 65, 64, 63 rows and of one row beside 127, 128 and 129.  Its
    1 383 blocks are 3 mod 4 and 7 mod 16: a wave taking 2, 4, 8 or 16 blocks ends in the middle of its group, and the blocks of one row and
    of 63, 64 and 65 rows put every guard of the rows' loads to work."""
    ds = bsbm.generate(2000)
    pairs = bl.feature_pairs(ds)
    kept, dropped = bc.edge_store_pairs(ds, pairs)
    nb, n_blocks = pc.layout_of(kept)
    assert n_blocks == 1383 and n_blocks % 2 == 1 and n_blocks % 4 == 3 and n_blocks % 8 == 7 and n_blocks % 16 == 7
    per = bl.block_survivors(ds, kept, 120, 170)
    assert len(per) == n_blocks
    gs, os_ = pc.stores(ds)
    q = pc.quads(ds, dropped[:, 0], ds.pred[bl.PF], dropped[:, 1])
    assert gs.remove(*q) == os_.remove(*q) == len(dropped)
    rng = np.random.default_rng(54)
    a, b = pl.Runner(torch_cuda, gs, os_, ds, COUNTS), Beside(torch_cuda, gs, os_, ds, DECLINED)
    for step in range(6):
        params = pc.batch_of(ds, rng, 1400 + step)
        sa, sb = a.run(params), b.run(params)
        same_rows(sa, sb)
        if step >= 4:
            equal_columns(sa, sb)
            if not ENGINE_TOGGLED:
                assert counted(sa, nb, n_blocks, per), sa.why()
                assert from_bits(sb, nb, n_blocks, per), sb.why()


@gpu
def test_full_rows(torch_cuda):
    """Every product of the largest feature group (139) gets one numeric1 and one numeric2 literal: its off-diagonal blocks are full, 150 rows
    of blocks count exactly 64 — a value that needs the byte's seventh bit — and two blocks take 64 rounds of the list (band_count_cases;
    the CPU test asserts these facts).  Batches of nearly all products, so that those rows count."""
    ds = bsbm.generate(2000)
    pairs = bl.feature_pairs(ds)
    nb, n_blocks = pc.layout_of(pairs)
    old, new, v1, v2 = bc.full_rows_edit(ds, pairs)
    per = bl.block_survivors(ds, pairs, 120, 170, v1, v2)
    rc = bc.row_counts(ds, pairs, 120, 170, v1, v2)
    assert rc.max() == 64 and int((rc == 64).sum()) == 150 and int((per == 4096).sum()) == 2
    gs, os_ = pc.stores(ds)
    assert gs.remove(*old) == os_.remove(*old) == len(old[0])
    assert gs.extend(*new) == os_.extend(*new) == len(new[0])
    rng = np.random.default_rng(55)
    a, b = pl.Runner(torch_cuda, gs, os_, ds, COUNTS), Beside(torch_cuda, gs, os_, ds, DECLINED)
    for step in range(6):
        params = pc.batch_of(ds, rng, 1990 + step)
        sa, sb = a.run(params), b.run(params)
        same_rows(sa, sb)
        if step >= 4:
            equal_columns(sa, sb)
            if not ENGINE_TOGGLED:
                assert counted(sa, nb, n_blocks, per), sa.why()
                assert from_bits(sb, nb, n_blocks, per), sb.why()


@gpu
def test_mutation_and_drop_tables(torch_cuda):
    """A mutation of the operand slice, then drop_tables, on two equal stores, one under a counts plan and one under a NO_BAND_PAIR_COUNTS plan:
    after either the counts are rebuilt with the list inside one step — the step reports the tables the other plan's reports, the counts are
    no table of their own — and the step after is back on the counts, with the new store's answers."""
    ds = bsbm.generate(2000, seed=15)
    pairs = bl.feature_pairs(ds)
    nb, n_blocks = pc.layout_of(pairs)
    per = bl.block_survivors(ds, pairs, 120, 170)
    (gs, os_), (gs2, os2) = pc.stores(ds), pc.stores(ds)
    rng = np.random.default_rng(56)
    a, b = pl.Runner(torch_cuda, gs, os_, ds, COUNTS), Beside(torch_cuda, gs2, os2, ds, DECLINED)
    for step in range(5):
        params = pc.batch_of(ds, rng, 1400 + step)
        sa, sb = a.run(params), b.run(params)
        same_rows(sa, sb)
        assert sa.m.tables_built == sb.m.tables_built, (step, sa.why(), sb.why())
    if not ENGINE_TOGGLED:
        assert counted(sa, nb, n_blocks, per), sa.why()
        assert from_bits(sb, nb, n_blocks, per), sb.why()
    touched = [ds.product(int(i)) for i in rng.choice(ds.n_products, 120, replace=False)]
    sel = (ds.p == ds.pred[bl.NUM1]) & np.isin(ds.s, touched)
    old = [c[sel] for c in (ds.g, ds.s, ds.p, ds.o)]
    moved = np.array(touched[60:], dtype=np.uint32)
    new = pc.quads(ds, moved, ds.pred[bl.NUM1], ds.int_base + rng.integers(0, 2000, 60))
    assert gs.remove(*old) == os_.remove(*old) == gs2.remove(*old) == 120
    assert gs.extend(*new) == os_.extend(*new) == gs2.extend(*new) == 60
    v1 = bl.numeric(ds, bl.NUM1)
    v1[np.array(touched[:60]) - ds.product_base] = bl.NONE
    v1[moved.astype(np.int64) - ds.product_base] = new[3].astype(np.int64) - ds.int_base + 1
    per_new = bl.block_survivors(ds, pairs, 120, 170, v1=v1)
    assert per_new.sum() != per.sum()
    others = sorted(set(range(ds.n_products)) - {x - ds.product_base for x in touched})
    built = []
    for step in range(5):
        params = pc.batch_of(ds, rng, 1400 + step, among=others)   # (no product twice: a repeated one would close the in-place route)
        params[1][:40] = touched[:20] + touched[60:80]             # products without the stage row, and products whose windows moved
        sa, sb = a.run(params), b.run(params)
        same_rows(sa, sb)
        assert sa.m.tables_built == sb.m.tables_built, (step, sa.why(), sb.why())
        built.append(sa.built_list)
    if ENGINE_TOGGLED:
        return
    assert sum(built) == 1                                          # list and counts of the new store: one step
    assert counted(sa, nb, n_blocks, per_new), sa.why()
    assert from_bits(sb, nb, n_blocks, per_new), sb.why()
    equal_columns(sa, sb)
    gs.drop_tables()
    gs2.drop_tables()
    params = pc.batch_of(ds, rng, 1410)
    sa, sb = a.run(params), b.run(params)
    same_rows(sa, sb)
    assert sa.built and sa.built_list and sa.m.exact_reruns == 0, sa.why()
    assert sa.m.tables_built == sb.m.tables_built and sa.m.host_syncs == sb.m.host_syncs, (sa.why(), sb.why())
    params = pc.batch_of(ds, rng, 1420)
    sa, sb = a.run(params), b.run(params)
    assert counted(sa, nb, n_blocks, per_new), sa.why()
    assert from_bits(sb, nb, n_blocks, per_new), sb.why()
    equal_columns(sa, sb)


@gpu
def test_the_bound_is_the_layouts_blocks(small, torch_cuda):
    """BAND_PAIR_COUNT_BLOCKS one above the layout's blocks: the bits are streamed; at exactly the layout's blocks: the counts"""
    ds, gs, os_, (nb, n_blocks), pairs, per = small
    rng = np.random.default_rng(57)
    s = pl.until_steady(pl.Runner(torch_cuda, gs, os_, ds, {"BAND_PAIR_COUNT_BLOCKS": n_blocks + 1}), ds, rng, steps=5)[-1]
    if not ENGINE_TOGGLED:
        assert from_bits(s, nb, n_blocks, per), s.why()
    s = pl.until_steady(pl.Runner(torch_cuda, gs, os_, ds, {"BAND_PAIR_COUNT_BLOCKS": n_blocks}), ds, rng, steps=5)[-1]
    if not ENGINE_TOGGLED:
        assert counted(s, nb, n_blocks, per), s.why()
