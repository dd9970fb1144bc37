"""The ordered-slice-join cases of ordered_cases.py on the CPU: the oracle's operator-at-a-time answer must be the dict-and-loop reference's
on every case the device tests run (test_gpu_ordered_join_edges.py), so that a wrong reference cannot hide a device bug, and the stores and
tables must hold what they are for: the slice row counts around the 1024-row tile, the chains around the 255 cap at the rows where tiles
and rounds begin and end, the tile totals around the 256 lanes, the tiles without a match and with one match at either end."""
import numpy as np
import pytest

from oracle import oracle as orc
import band_cases as bc
import ordered_cases as oc
import kat_util as ku

_STORES = {}


def oracle_store(n):
    if n not in _STORES:
        _STORES[n] = orc.OracleStore()
        _STORES[n].extend(*oc.quads(n))
    return _STORES[n]


def table_by_name(n, name):
    return next(c.table for c in oc.cases_of(n) if c.name == name)


@pytest.mark.parametrize("n", oc.SLICE_ROWS)
def test_slices_are_what_the_store_sorts_them_to(n):
    """n rows exactly, unique (s, o) pairs already in (o, s) order, more than 1024 of them, a subject with two rows (the CSR form), subjects
    from 100 up; look-up slices of more than 1024 rows with unique subjects, each lacking some"""
    sl = oc.slice_of(n)
    pairs = list(zip(sl.o, sl.s))
    assert len(pairs) == n > 1024 and len(set(pairs)) == n and pairs == sorted(pairs)
    assert max(len(r) for r in sl.rows_of.values()) >= 2 and sl.rows_of[oc.LA][:3] == [0, 256, 1024] and sl.rows_of[oc.HA] == [255, 1023]
    assert sl.kmin == oc.S0 > 1 and oc.HOLE not in sl.rows_of and sl.kmin < oc.HOLE < sl.kmax and sl.kmax in sl.rows_of
    assert sl.tiles == {1025: 2, 2047: 2, 2048: 2, 2049: 3, 3072: 3}[n]
    g, s, p, o = oc.quads(n)
    assert int((p == oc.P_LINK).sum()) == n
    os_ = oracle_store(n)
    pb = oc.PlanBuilder()
    cols, n_rows, _ = os_.execute(pb.build(pb.data_source(oc.quad_pattern("s", oc.P_LINK, "v"))))
    assert n_rows == n                                                           # nothing was a duplicate
    for k, rows in enumerate(oc.STAGES):
        assert len(rows) > 1024 and int((p == oc.P_A[k]).sum()) == len(rows)
        edge = oc.stage_edge_keys(k)
        assert edge[0] == 0 and edge[1] == min(rows) - 1 and edge[2] == max(rows) + 1 and min(rows) < edge[3] < max(rows) and edge[3] not in rows


@pytest.mark.parametrize("n", oc.SLICE_ROWS)
def test_tables_hold_what_they_are_for(n):
    sl = oc.slice_of(n)
    for c in oc.cases_of(n):
        assert len(c.table[0]) <= n, oc.case_id(c)                               # else the engine would build on the table
        assert c.table[0].tolist() == list(range(1, len(c.table[0]) + 1))
    # chains of 254 .. 300 rows on the slice rows where a tile or a round begins or ends, whatever the number of stages
    for length in oc.CHAINS:
        for n_stages in (0, 3):
            chains = oc.chain_lengths(n, table_by_name(n, f"chain{length}"), n_stages)
            assert [i for i, c in enumerate(chains) if c] == [i for i in oc.CHAIN_ROWS if i < n] and set(chains) == {0, length}
    mixed = oc.chain_lengths(n, table_by_name(n, "mixed"))
    assert {0, 1, 2} <= set(mixed)
    keys = set(table_by_name(n, "mixed")[1].tolist())
    assert {0, sl.kmin - 1, sl.kmin, sl.kmax, sl.kmax + 1, 0xFFFFFFFF, oc.HOLE} <= keys
    stage_keys = [set(table_by_name(n, "mixed")[2 + k].tolist()) for k in range(3)]
    assert all(set(oc.stage_edge_keys(k)) <= stage_keys[k] for k in range(3))
    assert oc.tile_totals(n, table_by_name(n, "mixed"), 3)[-1] > 0               # the last (partial) tile with matches ..
    assert oc.tile_totals(n, table_by_name(n, "lone_chains"))[-1] == 0 or n % oc.TILE == 0   # .. and without
    # tile totals of 255, 256 and 257 matches
    totals = oc.tile_totals(n, table_by_name(n, "totals"), 3)
    assert totals[:n // oc.TILE] == [oc.tile_total_of(sl, t) for t in range(n // oc.TILE)], totals
    # a long chain next to rows without matches
    lone = oc.chain_lengths(n, table_by_name(n, "lone_chains"), 3)
    assert lone[512] == 300 and sum(lone[:oc.TILE]) == 300
    if n >= 2048:
        assert lone[1536] == 255 and sum(lone[oc.TILE:2 * oc.TILE]) == 255
        only = oc.chain_lengths(n, table_by_name(n, "only_q1023"), 3)
        assert [i for i, c in enumerate(only) if c and i >= oc.TILE] == [2047] and sum(only[:oc.TILE]) > 0
    if sl.tiles == 3:
        gap = oc.tile_totals(n, table_by_name(n, "gap"), 3)
        assert gap[0] > 0 and gap[1] == 0 and gap[2] > 0, gap
        only = oc.chain_lengths(n, table_by_name(n, "only_q0"), 3)
        assert [i for i, c in enumerate(only) if c and i >= oc.TILE] == [2048] and sum(only[:oc.TILE]) > 0
    assert len(table_by_name(n, "empty")[0]) == 0
    assert oc.reference(n, table_by_name(n, "nothing"), 0, ("tag",)) == [] and len(table_by_name(n, "nothing")[0]) > 0


def test_every_total_and_every_chain_is_met():
    totals = {t for n in oc.SLICE_ROWS for t in oc.tile_totals(n, table_by_name(n, "totals"))[:n // oc.TILE]}
    assert totals == {255, 256, 257}
    chains = {c for n in oc.SLICE_ROWS for case in oc.cases_of(n) for c in oc.chain_lengths(n, case.table)}
    assert {0, 1, 2, 254, 255, 256, 300} <= chains
    # the route boundary's tables: exactly 255 and 256 rows; the warm-up table leaves room for the longest case
    assert len(oc.reference(2048, oc.t_rows(oc.slice_of(2048), 255), 3, ("tag",))) == 255
    assert len(oc.reference(2048, oc.t_rows(oc.slice_of(2048), 256), 3, ("tag",))) == 256
    for n in oc.SLICE_ROWS:
        warm = len(oc.reference(n, oc.t_warm(oc.slice_of(n)), 3, ("tag",)))
        assert warm * 8 >= n and warm + warm // 4 + 256 >= max(len(oc.reference(n, c.table, 0, ("tag",))) for c in oc.cases_of(n)), n


def test_projections_cover_the_record_and_the_column_counts():
    for n_stages in range(4):
        projs = {name: oc.projection(name, n_stages) for name in oc.PROJECTIONS}
        assert {len(p) for p in projs.values()} == set(range(1, 10))
        assert {0, 4, 5, 8} <= {oc.words(p) for p in projs.values()}
        assert any(len(set(p)) < len(p) and oc.eligible(p) for p in projs.values())
        assert [name for name, p in projs.items() if not oc.eligible(p)] == ["9_cols"]
        assert all(int(c[1]) <= n_stages for p in projs.values() for c in p if c[0] == "v")
    assert oc.projection("8_words", 3) == ("tag", "key", "k1", "k2", "k3", "v1", "v2", "v3")


def test_reference_known_answers():
    tab = oc.table([oc.LA, 0, oc.HOLE, oc.HA, oc.LA], clean=(oc.LA, oc.HA))
    rows = oc.reference(1025, tab, 0, ("tag", "s", "o"))
    assert rows == [(1, oc.LA, oc.O0), (5, oc.LA, oc.O0), (4, oc.HA, oc.O0 + 63), (1, oc.LA, oc.O0 + 64), (5, oc.LA, oc.O0 + 64),
                    (4, oc.HA, oc.O0 + 255), (1, oc.LA, oc.O0 + 256), (5, oc.LA, oc.O0 + 256)]
    tab[2][0] = oc.stage_edge_keys(0)[3]                                         # row 1 loses its first stage row
    assert [r[0] for r in oc.reference(1025, tab, 1, ("tag", "v1"))] == [5, 4, 5, 4, 5]
    assert oc.reference(1025, tab, 1, ("v1",))[0] == (oc.STAGES[0][int(tab[2][4])],)
    # the comparison helper: a chain in another order passes, a slice row out of place does not
    cols = lambda rs: [np.array(c, np.uint32) for c in zip(*rs)]
    swapped = [rows[1], rows[0]] + rows[2:]
    oc.assert_slice_order(cols(swapped), rows, ("tag", "s", "o"))
    with pytest.raises(AssertionError):
        oc.assert_slice_order(cols([rows[2], rows[0], rows[1]] + rows[3:]), rows, ("tag", "s", "o"))
    with pytest.raises(AssertionError):
        oc.assert_slice_order(cols(rows[:-1] + [(4, oc.LA, oc.O0 + 256)]), rows, ("tag", "s", "o"))


@pytest.mark.parametrize("n", oc.SLICE_ROWS)
def test_oracle_equals_reference(n):
    """every table x 0 .. 3 stages x every projection; and the table that goes through a FilterExec"""
    os_ = oracle_store(n)
    for c in oc.cases_of(n):
        for n_stages in range(4):
            for name in oc.PROJECTIONS:
                proj = oc.projection(name, n_stages)
                want = oc.reference(n, c.table, n_stages, proj)
                exp, n_exp, _ = os_.execute(oc.ordered_plan(n_stages, proj), [c.table])
                assert n_exp == len(want), (oc.case_id(c), n_stages, name, n_exp, len(want))
                oc.assert_multiset([np.asarray(e)[:n_exp] for e in exp], want, proj, f"{oc.case_id(c)} {n_stages} stages {name}")
    sl = oc.slice_of(n)
    m = min(n, 1500)
    for flags in ([oc.KEEP if i % 10 == 0 else oc.DROP for i in range(m)], [oc.DROP] * m):
        tab = oc.t_sized(sl, m, flags)
        proj = oc.projection("stage_values", 2)
        want = oc.reference(n, tab, 2, proj)
        exp, n_exp, _ = os_.execute(oc.ordered_plan(2, proj, flagged=True), [tab])
        oc.assert_multiset([np.asarray(e)[:n_exp] for e in exp], want, proj, f"{n} flagged")
        assert (len(want) > 0) == (oc.KEEP in flags)


@pytest.mark.parametrize("extra_row", [False, True])
def test_band_store_over_an_ordered_join(extra_row):
    """the store of the band join that reads the ordered slice join's matches: 2048 (2049) pF rows, the first table's matches all in the
    first tile, one product twice; the oracle's rows of the whole plan are window_reference's over the constants table"""
    st = oc.band_store(extra_row)
    g, s, p, o = st.quads
    pf = sorted(zip(o[p == bc.PF].tolist(), s[p == bc.PF].tolist()))
    assert len(pf) == len(set(pf)) == st.n_build == (2049 if extra_row else 2048)
    sizes = np.bincount(o[p == bc.PF] - bc.FEAT0)
    assert st.n_build >= 4 * len(sizes) and sizes.max() <= 512 and all((p == pv).sum() > 1024 for pv in (bc.PV, bc.PV2))
    os_ = orc.OracleStore()
    os_.extend(*st.quads)
    os_.set_typed_values(st.tv, st.decimals)
    windows = (oc.BAND_WINDOW, oc.BAND_WINDOW_2)
    for second_tile in (False, True):
        params = oc.band_params(second_tile)
        xs = params[1].tolist()
        assert len(xs) <= st.n_build and max(xs.count(x) for x in set(xs)) == 2
        C = oc.band_constants(st, params)
        rows_of = [i for i, (f_, x) in enumerate(pf) if x in set(xs)]
        assert len(C[0]) * 8 >= st.n_build and (max(rows_of) < 1024) == (not second_tile)
        want, unfiltered = bc.window_reference(st.quads, st.terms, C, windows, True)
        assert 0 < len(want) < unfiltered
        exp, n_exp, _ = os_.execute(oc.band_over_ordered_plan(windows, True), [params])
        np.testing.assert_array_equal(ku.multiset(exp, n_exp), want)
