"""The band join of the batched Q5 reading the slice's rows in place with the ROWS' decoded windows kept on the slice (band_join.hip,
BandArgs::row_win; store.hpp, SliceTable::BandRowWindows): in Q5 both window operands of a row are reached from its product alone, so
they are decoded once per store version and a step carries 4 bytes per slice row (the instance tag) instead of a 16-byte record.
Every check compares whole result multisets with the oracle; NO_BAND_ROW_CACHE keeps the form without the table, and which form a step
took shows in the bytes per row of its in-place pass (12 with the table, 36 without) and in the two build kernels."""
import os

import numpy as np
import pytest

import rdf_fusion_amd as rf
from rdf_fusion_amd import abi, bsbm
from oracle import oracle as orc
import kat_util as ku

gpu = pytest.mark.gpu

ENGINE_TOGGLED = any(k.startswith(("RDFGPU_NO_", "RDFGPU_FORCE_")) for k in os.environ)   # a debugging toggle is set for the whole run
IN_PLACE = "OjInPlace"          # the in-place form's kernel name carries its tag type
BUILD = ("band_row_win_keys_kernel", "band_row_win_rows_kernel")
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


def quads(ds, s, p, o):
    s = np.asarray(s, dtype=np.uint32)
    return [np.zeros(len(s), np.uint32), s, np.full(len(s), p, np.uint32), np.asarray(o, dtype=np.uint32)]


def feature_pairs(ds):
    """the productFeature slice as the store holds it: distinct (product, feature) pairs"""
    sel = ds.p == ds.pred[PF]
    return np.unique(np.stack([ds.s[sel], ds.o[sel]], axis=1), axis=0)


class Runner:
    def __init__(self, torch, gs, os_, ds, option=None, **windows):
        self.torch, self.os_, self.desc = torch, os_, bsbm.q5_batch_plan(ds, **windows)
        self.plan = gs.plan(self.desc).enable_kernel_timing(True)
        if option:
            self.plan.set_option(option, 1)

    def run(self, params):
        """one step, checked against the oracle: (metrics, kernel classes that ran, bytes per row of the in-place pass or None)"""
        keep, ptrs = on_device(self.torch, params)
        self.plan.bind_table(0, ptrs, len(params[0]))
        got = self.plan.execute().fetch()
        exp, n_exp, _ = self.os_.execute(self.desc, [params])
        np.testing.assert_array_equal(ku.multiset(got), ku.multiset(exp, n_exp))
        stats = self.plan.kernel_stats()
        per_row = [nbytes // rows for name, launches, ms, nbytes, rows in stats if IN_PLACE in name and rows]
        return self.plan.metrics(), {k[0] for k in stats}, (per_row[0] if per_row else None)


def built(ran):
    return [any(b in k for k in ran) for b in BUILD]


def steady(m, ran, per_row):
    """the in-place route with the cached windows, nothing built or waited for inside the step"""
    return per_row == 12 and not any(built(ran)) and not any("oj_count_kernel" in k or "band_desc_kernel" in k for k in ran) and \
        m.tables_built == 0 and m.host_syncs == 1 and m.exact_reruns == 0


def until_steady(r, ds, rng, n=1400, steps=8):
    for step in range(steps):
        m, ran, per_row = r.run(batch_of(ds, rng, n + step))
    return m, ran, per_row


@pytest.fixture(scope="module")
def small(torch_cuda):
    ds = bsbm.generate(2000)
    gs, os_ = stores(ds)
    return ds, gs, os_


@gpu
def test_against_the_uncached_form_and_the_oracle(small, torch_cuda):
    """Eight different batches (ids that are no product's on odd steps): with the table and without it (NO_BAND_ROW_CACHE) every step
    answers like the oracle.  The last four steps of the default plan run the in-place kernel over 12 bytes per row, build nothing and
    wait once; the plan with the option never builds the table and keeps the 36-byte pass."""
    ds, gs, os_ = small
    rng = np.random.default_rng(21)
    a, b = Runner(torch_cuda, gs, os_, ds), Runner(torch_cuda, gs, os_, ds, "NO_BAND_ROW_CACHE")
    seen_a, seen_b = [], []
    for step in range(8):
        params = batch_of(ds, rng, 1500 - 20 * step, foreign=40 if step % 2 else 0)
        seen_a.append(a.run(params))
        seen_b.append(b.run(params))
    if ENGINE_TOGGLED:
        return
    for m, ran, per_row in seen_a[-4:]:
        assert steady(m, ran, per_row), (m.tables_built, m.host_syncs, m.exact_reruns, per_row, sorted(ran))
    assert sum(all(built(ran)) for _, ran, _ in seen_a) <= 1        # (none at all when an earlier test's plan left the table on the store)
    for m, ran, per_row in seen_b:
        assert not any(built(ran)), sorted(ran)
    m, ran, per_row = seen_b[-1]
    assert per_row == 36 and m.tables_built == 0 and m.host_syncs == 1, (per_row, m.tables_built, m.host_syncs, sorted(ran))


@gpu
def test_products_entering_and_leaving_the_batch(torch_cuda):
    """Two disjoint halves of the products on alternate steps: a slice row that carried a value in one step has none in the next (its
    key's entry says "no table row" again) and must emit nothing.  The halves cover the same number of slice rows, so that each still
    covers half of the slice and the route stays."""
    ds = bsbm.generate(2000, seed=12)
    pairs = feature_pairs(ds)
    rows = np.bincount(pairs[:, 0] - ds.product_base, minlength=ds.n_products)
    rng = np.random.default_rng(22)
    order = rng.permutation(ds.n_products)
    half = [list(order[:1000]), list(order[1000:])]
    if rows.sum() % 2:                                             # an odd slice cannot be halved: one pair of a product with many goes
        victim = int(np.argmax(rows))
        gone = pairs[pairs[:, 0] == ds.product(victim)][:1]
        rows[victim] -= 1
    else:
        gone = pairs[:0]
    diff = int(rows[half[0]].sum() - rows[half[1]].sum())          # even; swapping i and j moves it by 2 (rows[j] - rows[i])
    while diff:
        step = max(-19, min(19, diff // 2))
        i, j = next((i, j) for i in range(1000) for j in range(1000) if rows[half[0][i]] - rows[half[1][j]] == step)
        half[0][i], half[1][j] = half[1][j], half[0][i]
        diff -= 2 * step
    assert rows[half[0]].sum() == rows[half[1]].sum() and not set(half[0]) & set(half[1])
    gs, os_ = stores(ds)
    if len(gone):
        q = quads(ds, gone[:, 0], ds.pred[PF], gone[:, 1])
        assert gs.remove(*q) == os_.remove(*q) == 1
    r = Runner(torch_cuda, gs, os_, ds)
    until_steady(r, ds, rng)
    seen = [r.run(batch_of(ds, rng, 1000, among=half[step % 2])) for step in range(6)]
    if not ENGINE_TOGGLED:
        for m, ran, per_row in seen[1:]:                           # (the first half-batch follows a larger one: any route)
            assert steady(m, ran, per_row), (m.tables_built, m.host_syncs, m.exact_reruns, per_row, sorted(ran))


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
    gs, os_ = stores(ds)
    q = quads(ds, pairs[drop][:, 0], ds.pred[PF], pairs[drop][:, 1])
    assert gs.remove(*q) == os_.remove(*q) == int(drop.sum())
    rng = np.random.default_rng(23)
    r = Runner(torch_cuda, gs, os_, ds)
    m, ran, per_row = until_steady(r, ds, rng)
    if not ENGINE_TOGGLED:
        assert steady(m, ran, per_row), (m.tables_built, m.host_syncs, m.exact_reruns, per_row, sorted(ran))


@gpu
def test_two_literal_sets_on_one_store(small, torch_cuda):
    """The windows depend on the plan's literals: two plans with different widths keep two tables on the slice, and neither replaces the
    other's (a plan that lost its table would build it again)."""
    ds, gs, os_ = small
    rng = np.random.default_rng(24)
    a, b = Runner(torch_cuda, gs, os_, ds), Runner(torch_cuda, gs, os_, ds, w1=7, w2=900)
    seen = []
    for step in range(8):
        params = batch_of(ds, rng, 1300 + step)
        seen.append((a.run(params), b.run(params)))
    if not ENGINE_TOGGLED:
        for pair in seen[-3:]:
            for m, ran, per_row in pair:
                assert steady(m, ran, per_row), (m.tables_built, m.host_syncs, m.exact_reruns, per_row, sorted(ran))
        assert sum(all(built(ran)) for _, (m, ran, _) in seen) == 1     # w1 = 7, w2 = 900 is this test's alone: its table was built here, once


@gpu
def test_mutation_and_drop_tables(torch_cuda):
    """A mutation of the operand slice (60 products lose numeric1, 60 others get a new value) drops the table with the store version:
    the next executions answer like the oracle on the new store and come back to the steady form; drop_tables makes the next step build
    the table inside the step, the one after finds it."""
    ds = bsbm.generate(2000, seed=15)
    gs, os_ = stores(ds)
    rng = np.random.default_rng(25)
    r = Runner(torch_cuda, gs, os_, ds)
    m, ran, per_row = until_steady(r, ds, rng)
    if not ENGINE_TOGGLED:
        assert steady(m, ran, per_row), (m.tables_built, m.host_syncs, m.exact_reruns, per_row, sorted(ran))
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
        m, ran, per_row = r.run(params)
    if ENGINE_TOGGLED:
        return
    assert steady(m, ran, per_row), (m.tables_built, m.host_syncs, m.exact_reruns, per_row, sorted(ran))
    gs.drop_tables()
    m, ran, per_row = r.run(batch_of(ds, rng, 1410))
    assert m.tables_built >= 6 and all(built(ran)) and per_row == 12 and m.exact_reruns == 0, (m.tables_built, per_row, sorted(ran))
    m, ran, per_row = r.run(batch_of(ds, rng, 1420))
    assert steady(m, ran, per_row), (m.tables_built, m.host_syncs, m.exact_reruns, per_row, sorted(ran))


@gpu
def test_overflowing_windows_decline_the_table(torch_cuda):
    """Every integer literal of the store moved up to end at 2^63 - 1: for the products whose numeric1 lies within 120 of it (or numeric2 within
    170) `orig + w` is no xsd:integer, their windows are not plain integer intervals, and the table is declined for the whole store — built
    once, remembered as declined, never built again.  Every step answers like the oracle: batches without such a product run the in-place
    route over 36-byte records, batches with one take the full semantics for its rows.  (The operands of Q5's rows and of its entries are
    one slice, so an operand that is not an xsd:integer at all closes the band join itself: the next test.)"""
    ds = bsbm.generate(2000, seed=16)
    top = 2 ** 63 - 1
    ints = slice(ds.int_base, ds.int_base + 2000)
    ds.typed_values["lo"][ints] += top - 2000                      # 1 .. 2000 -> top - 1999 .. top
    value_of = lambda pname: {int(s_): int(ds.typed_values["lo"][o_]) for s_, o_ in zip(ds.s[ds.p == ds.pred[pname]], ds.o[ds.p == ds.pred[pname]])}
    v1, v2 = value_of(NUM1), value_of("bsbm:productPropertyNumeric2")
    over = [i for i in range(ds.n_products) if v1[ds.product(i)] + 120 > top or v2[ds.product(i)] + 170 > top]
    others = [i for i in range(ds.n_products) if i not in set(over)]
    assert 4 <= len(over) <= 100, len(over)
    gs, os_ = stores(ds)
    rng = np.random.default_rng(26)
    r = Runner(torch_cuda, gs, os_, ds)
    seen = [r.run(batch_of(ds, rng, 1400 + step, among=others)) for step in range(7)]
    for step in range(3):
        params = batch_of(ds, rng, 1380 + step, among=others)
        params[1][step] = ds.product(over[step])
        seen.append(r.run(params))
    seen += [r.run(batch_of(ds, rng, 1390 + step, among=others)) for step in range(3)]
    if not ENGINE_TOGGLED:
        assert sum(all(built(ran)) for _, ran, _ in seen) == 1 and sum(any(built(ran)) for _, ran, _ in seen) == 1, [built(ran) for _, ran, _ in seen]
        assert all(per_row in (None, 36) for _, _, per_row in seen) and seen[6][2] == 36, [p for _, _, p in seen]


@gpu
def test_non_integer_operand(torch_cuda):
    """One product's numeric1 is an xsd:double.  The slice's decoded value table is then unusable for rows and entries alike: the table is never
    built, and every step answers like the oracle, with that product in the batch and without it."""
    ds = bsbm.generate(2000, seed=16)
    gs, os_ = stores(ds)
    rng = np.random.default_rng(27)
    odd = 777
    sel = (ds.p == ds.pred[NUM1]) & (ds.s == ds.product(odd))
    old = [c[sel] for c in (ds.g, ds.s, ds.p, ds.o)]
    assert gs.remove(*old) == os_.remove(*old) == 1
    double_id = int(np.flatnonzero(ds.typed_values["tag"] == abi.TV_DOUBLE)[5])
    new = quads(ds, [ds.product(odd)], ds.pred[NUM1], [double_id])
    assert gs.extend(*new) == os_.extend(*new) == 1
    others = [i for i in range(ds.n_products) if i != odd]
    r = Runner(torch_cuda, gs, os_, ds)
    seen = [r.run(batch_of(ds, rng, 1400 + step, among=others)) for step in range(4)]
    for step in range(2):
        params = batch_of(ds, rng, 1380 + step, among=others)
        params[1][step] = ds.product(odd)
        seen.append(r.run(params))
    seen.append(r.run(batch_of(ds, rng, 1390, among=others)))
    if not ENGINE_TOGGLED:
        assert not any(any(built(ran)) for _, ran, _ in seen) and all(per_row in (None, 36) for _, _, per_row in seen), [p for _, _, p in seen]


def test_eligibility_predicate():
    """The host decision (host_logic.cpp, no device): Q5's shape — both operands of both windows from stages keyed by the join key — is
    eligible; a stage keyed by another table column, an operand of the table row itself, the option, and a route that is not the
    in-place one each decline."""
    q5 = [[(2, True), (2, True)], [(3, True), (3, True)]]
    assert rf.band_row_cache_eligible(q5)
    assert rf.band_row_cache_eligible(q5[:1]) and rf.band_row_cache_eligible([])
    assert not rf.band_row_cache_eligible([[(2, True), (2, True)], [(3, True), (3, False)]])       # ?Y numeric2 ?orig2 with Y another column
    assert not rf.band_row_cache_eligible([[(0, False), (2, True)], [(3, True), (3, True)]])        # an operand bound with the table row
    assert not rf.band_row_cache_eligible([[(0, True), (0, True)]]) and not rf.band_row_cache_eligible([[(1, True), (1, True)]])
    assert not rf.band_row_cache_eligible(q5, option_set=True)
    assert not rf.band_row_cache_eligible(q5, in_place=False)
    assert not rf.band_row_cache_eligible(q5, compact=False) and not rf.band_row_cache_eligible(q5, pack16=False)
    with pytest.raises(rf.RdfGpuError):
        rf.band_row_cache_eligible(q5 + q5[:1])
