"""The hash-join cases of join_cases.py on the CPU: the oracle's answer must be the dict-and-loop reference's on every case the device
tests run (test_gpu_join_edges.py), so that a wrong reference cannot hide a device bug, and the tables must hold what they are for: the
rounds that fill, overfill and leave the wave queues, results exactly on and one past the output capacities, the wrap keys' home slots,
the tile of each chosen row, the row counts on both sides of the ITEMS switch, the fan-outs around the lanes per CSR row."""
import numpy as np
import pytest

from oracle import oracle as orc
import join_cases as jc

_STORE = []


def oracle_store():
    if not _STORE:
        _STORE.append(jc.fill_store(orc.OracleStore()))
    return _STORE[0]


def check(join, tables, what):
    want = jc.expected(join, tables)
    exp, n_exp, _ = oracle_store().execute(jc.plan_of(join), tables)
    assert n_exp == len(want), (what, n_exp, len(want))
    jc.assert_rows([np.asarray(e)[:n_exp] for e in exp], want, len(join.proj), what)
    return want


# ---------------------------------------------------------------------------------------------------
# the store and the reference
# ---------------------------------------------------------------------------------------------------
def test_store_is_what_the_cases_assume():
    """slices of more than 1024 rows; unique dense keys with holes (direct), the stated fan-outs with empty groups inside the range (CSR),
    one slice sorted by the key in (?o, ?s) order and one not, scattered keys (no dense table); the store keeps every quad"""
    g, s, p, o = jc.quads()
    os_ = oracle_store()
    for P, sl in jc.SLICES.items():
        assert len(sl[0]) > 1024 and int((p == P).sum()) == len(sl[0])
        pb = jc.PlanBuilder()
        assert os_.execute(pb.build(pb.data_source(jc.quad_pattern("s", P, "o"))))[1] == len(sl[0])   # nothing was a duplicate
    d = jc.SLICES[jc.P_D][0].tolist()
    assert len(set(d)) == len(d) == 2070 and jc.HOLE_D not in d and jc.KMIN_D < jc.HOLE_D < jc.KMAX_D and jc.KMIN_D - 1 > 1
    assert len(d) <= jc.KMAX_D - jc.KMIN_D + 1 <= 4 * len(d) + 1024                                  # build_direct: a direct-address attempt
    for P in (jc.P_CS, jc.P_CU):
        ks, os__ = jc.SLICES[P]
        counts = np.bincount(ks - jc.C0, minlength=jc.KMAX_C - jc.C0 + 1)
        for f in jc.FANS:
            assert all(counts[k - jc.C0] == f for k in jc.KEYS[f]), f
        assert len(ks) == 2056 > jc.KMAX_C - jc.KMIN_C + 1 and ks.min() == jc.KMIN_C and ks.max() == jc.KMAX_C   # more rows than ids: CSR outright
        by_o = ks[np.argsort(os__, kind="stable")].astype(np.int64)
        assert bool(np.all(np.diff(by_o) >= 0)) == (P == jc.P_CS)
        for k in jc.KEYS[6]:                                                                        # the partners of a key alternate 0 / 10
            vals = sorted(jc.TERMS[x][1] for x in os__[ks == k].tolist())
            assert vals == [0, 0, 0, 10, 10, 10]
    w = jc.SLICES[jc.P_W][0]
    assert int(w.max()) - int(w.min()) + 1 > 64 * len(w) + 1024                                     # build_dense_table: not worth a dense table
    assert jc.TERMS[jc.STRING_ID] is None and jc.TERMS[jc.DOUBLE_ID][0] == "double"
    ints = [jc.TERMS[i][1] for i in jc.INT_IDS]
    assert jc.I64_MIN in ints and jc.I64_MAX in ints and sum(v + 3 > jc.I64_MAX for v in ints) == 2


def test_reference_known_answers():
    left = [[1, 2, 3, 4], [10, 0, 11, 12]]
    right = [[10, 10, 12, 0], [7, 8, 9, 6]]
    assert sorted(jc.reference(left, right, [(1, 0)])) == [(1, 10, 10, 7), (1, 10, 10, 8), (4, 12, 12, 9)]
    assert sorted(jc.reference(left, right, [(1, 0)], "left", None, (0, 3))) == [(1, 7), (1, 8), (2, 0), (3, 0), (4, 9)]
    odd = lambda l, r: r[1] % 2 == 1
    assert sorted(jc.reference(left, right, [(1, 0)], "left", odd, (0, 3))) == [(1, 7), (2, 0), (3, 0), (4, 9)]
    assert jc.reference(left, right, [(1, 0), (0, 1)]) == [] and jc.reference([[], []], right, [(1, 0)], "left") == []
    big = [np.arange(1, (1 << 18) + 2), np.full((1 << 18) + 1, 99)]
    big[1][[5, 70000]] = [10, 12]
    assert sorted(jc.reference(big, right, [(1, 0)], "inner", None, (0, 3))) == [(6, 7), (6, 8), (70001, 9)]
    f = jc.pred_fn(("id", False, 0, 2))
    assert f((5,), (5, 6)) and not f((6,), (5, 6)) and not f((0,), (5, 6)) and not f((5,), (5, 0))
    w = jc.pred_fn(("win", jc.W3, 0, 1, 1))
    at = lambda v: jc.INT_IDS[jc.ZOO_INTS.index(v)]
    assert w((at(2), at(0)), ()) and not w((at(3), at(0)), ()) and not w((at(jc.I64_MAX), at(jc.I64_MAX)), ()) and not w((at(0), jc.STRING_ID), ())
    assert w((at(2), jc.DOUBLE_ID), ()) and not w((0, at(0)), ())
    vm = jc.pred_fn(("vm", 0, 1, 2))
    assert vm((at(2), at(0), 9), ()) and not vm((at(2), at(0), 0), ()) and not vm((at(3), at(0), 9), ()) and not vm((at(0), at(jc.I64_MAX - 2), 9), ())


# ---------------------------------------------------------------------------------------------------
# the cases, group by group
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", list(jc.PATTERNS))
def test_group1_queue_rounds(pattern):
    """what the wave of each pattern does to a queue of 64, 128 and 256 entries (size_wave_queue's smallest); the oracle on every table"""
    r = jc.rounds(jc.PATTERNS[pattern])
    trace = {q: jc.queue_trace(r, q) for q in (64, 128, 256)}
    if pattern == "m1":        # exactly full, nothing pended
        assert trace[64] == [(0, 64, False)]
    if pattern in ("m2", "m3", "m6"):      # every later round is pended and resumed
        assert all(t == (64, 64, True) for t in trace[64][1:]) and len(trace[64]) == int(pattern[1])
        assert [t[2] for t in trace[128]] == [False, False, True, False, True, False][:len(r)]   # 128: full after two rounds, then pended
    if pattern == "mod5":      # a round is pended with the queue partly full
        assert r == [51, 38, 25, 12]
        assert trace[64] == [(0, 51, False), (51, 38, True), (38, 25, False), (63, 12, True)]
        assert trace[128] == [(0, 51, False), (51, 38, False), (89, 25, False), (114, 12, False)] and 51 + 38 > 64
    if pattern == "hot":       # one lane, 300 rounds of one candidate: full at 64, 128, 256 with nothing beside it
        assert r == [1] * 300 and sum(t[2] for t in trace[64]) == 4 and sum(t[2] for t in trace[256]) == 1
    for n in jc.WAVE_ROWS:
        fans = jc.wave_fans(n, pattern)
        assert fans[:64] == jc.PATTERNS[pattern] == fans[448:512] and not any(fans[64:448])
        assert fans[512:] == jc.PATTERNS[pattern][:n - 512]                                          # the live lanes of the partial tile
        t = jc.wave_table(n, pattern)
        sl = jc.SLICES[jc.P_CS][0]
        assert [int((sl == k).sum()) for k in t[1].tolist()] == fans
        for fname, pred in jc.FILTERS.items():
            want = check(jc.slice_join(jc.P_CS, pred), [t], f"{pattern} {n} {fname}")
            total = sum(fans)
            assert len(want) == {"none": total, "all": 0, "alt": sum((f + 1) // 2 for f in fans)}[fname] or fname == "alt"
            if fname == "alt":
                assert 0 < len(want) < total or total <= 64


def test_group2_output_capacity():
    """512 probe rows with exactly 1536 = 512 + 1024 rows (first_guess of a hash / LDS table) and 1537; then exactly on and one past
    prev + prev / 4 + 256 twice over"""
    assert jc.spec_cap(1536) == 2176 and jc.spec_cap(2176) == 2976 and jc.spec_cap(1537) == 2177 and jc.spec_cap(2178) == 2978
    for total in (1536, 1537, 2176, 2178, 2976, 2977, 2978):
        t = jc.total_table(512, total)
        assert len(t[0]) == 512
        assert len(check(jc.slice_join(jc.P_CS), [t], f"total {total}")) == total


@pytest.mark.parametrize("n", jc.LDS_BUILDS)
def test_group3_lds_builds(n):
    """slot counts at the sizes where they change; the probe side is not smaller than the build side (the engine builds on the table of slot 0)"""
    assert [jc.lds_slots(x) for x in (1, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192)] == [2048, 2048, 4096, 4096, 8192, 8192, 16384, 16384, 16384, 16384]
    tables = [jc.lds_build(n), jc.lds_probe(n)]
    assert len(tables[0][0]) == n <= len(tables[1][0])
    want = check(jc.TABLE_JOIN, tables, f"build {n}")
    assert 0 < len(want) < len(tables[1][0])                                                           # absent and null keys among the probe rows
    assert {r[0] for r in want} >= {jc.K0L, jc.K0L + n - 1}                                            # the first and the last build row are met


def test_group3_null_build_and_one_key_chain():
    tables = [jc.lds_build(600, np.zeros(600)), jc.lds_probe(600)]
    assert check(jc.TABLE_JOIN, tables, "null build") == []
    assert len(check(jc.TABLE_JOIN._replace(how="left"), tables, "null build, left")) == 600
    tables = jc.one_key_tables()
    assert len(tables[0][0]) == 8192 == len(tables[1][0]) and len(check(jc.TABLE_JOIN, tables, "one key")) == 24576


def test_group4_wrap_keys():
    """eight keys whose home slot is mask - 1 or mask under every power-of-two mask up to 2^17: the cluster of the six that are built runs
    through slot 0, and the two absent ones walk across the wrap to the first empty slot"""
    assert len(jc.WRAP) == 8 == len(set(jc.WRAP))
    for bits in range(6, 18):
        mask = (1 << bits) - 1
        homes = (jc.hash1(jc.WRAP) & mask).tolist()
        assert set(homes) <= {mask - 1, mask}, (bits, homes)
    for keys, masks in ((jc.WRAP_BUILD, [(1 << b) - 1 for b in range(6, 18)]), (jc.WRAP_BUILD + jc.W_FILL, [4095, 8191, 16383, 32767])):
        for mask in masks:
            occ = jc.occupied(keys, mask)
            assert {mask, 0, 1, 2, 3} <= occ                                                           # seven rows from mask - 1 / mask on
            for absent in jc.WRAP[6:]:
                slots = jc.walk(absent, occ, mask)
                assert slots[0] >= mask - 1 and slots[-1] < mask - 1 and mask in slots and 0 in slots   # across the wrap
    want = check(jc.TABLE_JOIN, jc.wrap_tables(), "wrap tables")
    assert sorted(r[0] for r in want) == sorted(jc.WRAP_BUILD)
    want = check(jc.slice_join(jc.P_W), [jc.wrap_table()], "wrap slice")
    assert sorted(r[1] for r in want) == sorted(jc.WRAP_BUILD)


@pytest.mark.parametrize("n", jc.TILE_PROBES)
def test_group5_tiles_per_workgroup(n):
    """more than 256 tiles of 512 rows: max_wg = 256 for an LDS table over 64 KiB (launch_lds_join), so workgroup 0 walks tiles 0, 256, 512"""
    assert jc.lds_slots(8192) * 8 > 64 * 1024
    chosen = jc.tile_chosen(n)
    tiles = {r // 512 for r in chosen}
    n_tiles = (n + 511) // 512
    assert n_tiles == {131072: 256, 131073: 257, 262657: 514}[n] and {0, n_tiles - 1} <= tiles
    assert (256 in tiles) == (n > 131072) and (512 in tiles) == (n == 262657)
    assert {0, 511} <= set(chosen)
    if n == 262657:
        wave = sorted(r for r in chosen if r // 512 == 512 and r != n - 1)
        assert wave == list(range(512 * 512 + 192, 512 * 512 + 256)) and (wave[0] % 512) // 64 == 3 and chosen[n - 1] and (n - 1) // 512 == 513
    tables = [jc.tile_build(), jc.tile_probe(n)]
    for n_keys in (1, 2):
        want = check(jc.TILE_JOIN[n_keys], tables, f"{n} rows, {n_keys} keys")
        assert len(want) == len(chosen) + (64 if n == 262657 else 0) + (2 if n_keys == 1 else 0)


def test_group6_items_switch():
    """lds_join_items (kernels.hip): 4 from 2^20 probe rows for an LDS table, from 2^22 (rows << rl) for an HBM table; direct_stream_join_items:
    8 (hash form: 4) from 2^20"""
    assert jc.BIG_ROWS == (2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1)
    build = jc.items_build()
    os_ = oracle_store()
    for n in jc.BIG_ROWS:
        t = jc.big_table(n)
        assert len(t[0]) == n
        # wave 3 of tile ITEMS_TILE (2048 rows = 512 x 4): items 0 .. 3 are its rows 192 .. 255 of each 512-row quarter, two partners each:
        # rounds of 64, 64 | 64, 64 | ... fill a 256-entry queue at the end of item 1, so item 2's first round is pended
        kl = t[3]
        for item in range(4):
            rows = jc.ITEMS_TILE * 2048 + item * 512 + 192 + np.arange(64)
            assert all(int((build[0] == k).sum()) == 2 for k in kl[rows].tolist())
        trace = jc.queue_trace([64, 64] * 4, 256)
        assert [x[2] for x in trace] == [False, False, False, False, True, False, False, False]
        assert int(kl[n - 1]) in build[0].tolist()
        if n <= 1 << 20:
            want = check(jc.ITEMS_JOIN, [build, t], f"lds {n}")
            assert len(want) == 2 * 256 + 2
        for join, lo in ((jc.slice_join(jc.P_D, proj=(0, 1, 5), left=("t", 0, 4)), 900), (jc.slice_join(jc.P_CS, proj=(0, 2, 5), left=("t", 0, 4))._replace(on=((2, 0),)), 900)):
            want = check(join, [t], f"stream {n}")
            assert lo < len(want) < 5000 and (n in {r[0] for r in want})                               # a few thousand rows, the last row among them
    for n in (65535, 65536):
        assert ((n << 6) >= 1 << 22) == (n == 65536)
        want = check(jc.slice_join(jc.P_CS), [jc.lanes_big_table(n)], f"rl 6, {n}")
        assert n in {r[0] for r in want} and len(want) > 10000


@pytest.mark.parametrize("rl", jc.ROW_LANES)
def test_group7_lanes_per_row(rl):
    fans = jc.lane_fans(rl)
    assert {0, 1, (1 << rl) - 1, 1 << rl, (1 << rl) + 1, 300} == set(fans) <= set(jc.FANS)
    assert jc.lane_rows(rl) == {0: (511, 512, 513, 1537), 1: (255, 256, 257, 769), 3: (63, 64, 65, 193), 6: (7, 8, 9, 25)}[rl]
    for n in jc.lane_rows(rl):
        t = jc.lanes_table(rl, n)
        counts = np.bincount(jc.SLICES[jc.P_CS][0], minlength=jc.KMAX_C + 2)
        got = {int(counts[k]) if jc.KMIN_C <= k <= jc.KMAX_C else 0 for k in t[1].tolist()}
        assert got == set(fans) or n < 12, (rl, n, got)
        for P in (jc.P_CS, jc.P_CU):
            for fname in ("none", "alt"):
                check(jc.slice_join(P, jc.FILTERS[fname]), [t], f"rl {rl} {n} {P} {fname}")


@pytest.mark.parametrize("direct", [True, False])
def test_group8_dense_bounds(direct):
    t = jc.bounds_table(direct)
    kmin, kmax, hole = (jc.KMIN_D, jc.KMAX_D, jc.HOLE_D) if direct else (jc.KMIN_C, jc.KMAX_C, jc.HOLE_C)
    assert {kmin, kmax, kmin - 1, kmax + 1, 0, 1, 0xFFFFFFFF, hole} <= set(t[1].tolist())
    P = jc.P_D if direct else jc.P_CS
    want = check(jc.slice_join(P), [t], f"bounds {direct}")
    keys = {r[1] for r in want}
    assert {kmin, kmax} <= keys and not keys & {kmin - 1, kmax + 1, 0, 1, 0xFFFFFFFF, hole}


@pytest.mark.parametrize("how", ["inner", "left"])
@pytest.mark.parametrize("n_keys", [2, 3, 4])
def test_group9_key_columns(n_keys, how):
    tables = jc.key_tables()
    b, p = tables
    assert set(b[0].tolist()) == {5} == set(p[0].tolist()) and 0 in b[3] and 0 in p[3] and 0 not in b[1] and 0 not in p[2]
    join = jc.key_join(n_keys, how)
    assert len(join.on) == n_keys and join.on[0] == (0, 0) and join.on[-1] == (3, 3)
    want = check(join, tables, f"{n_keys} keys {how}")
    fewer = check(jc.key_join(n_keys - 1, how), tables, "") if n_keys > 2 else None
    assert fewer is None or len([r for r in want if r[2]]) < len([r for r in fewer if r[2]])           # every further key column removes pairs


def test_group10_to_14_and_predicates():
    for n_cols, proj in jc.PROJECTIONS.items():
        assert len(proj) == n_cols and any(c < 5 for c in proj) == (n_cols > 1) and any(c >= 5 for c in proj)
        check(jc.slice_join(jc.P_D, proj=proj), [jc.bounds_table(True)], f"{n_cols} columns")
    # left joins: both forms are one plan
    for direct, P in ((True, jc.P_D), (False, jc.P_CS), (False, jc.P_CU)):
        for name in ("unmatched64", "pend_null", "mixed"):
            t = jc.left_table(name, direct)
            assert len(t[0]) == 513 and 4 * 513 <= len(jc.SLICES[P][0])                                # choose_build_left: the probe-preserving form
            want = check(jc.slice_join(P, how="left", proj=(0, 1, 5, 6)), [t], f"left {name} {P}")
            nulls = [r for r in want if r[2] == 0]
            fans = jc.left_fans(name, 1 if direct else 6)
            assert len(nulls) == fans.count(0) and (name != "unmatched64" or fans[:64] == [0] * 64) and fans[512] == 0 and 0 in t[1][:64] or name != "unmatched64"
    r = jc.rounds(jc.left_fans("pend_null", 6)[:64], outer=True)
    assert r == [64, 63] and jc.queue_trace(r, 64) == [(0, 64, False), (64, 63, True)]                 # the null row is queued when the round behind it is pended
    tables = jc.classic_left_tables()
    want = check(jc.TABLE_JOIN._replace(how="left"), tables, "classic left")
    assert 0 < sum(r[2] == 0 for r in want) < 600
    # fused filters
    t = jc.flagged_wave_table()
    assert {0, jc.KEEP, jc.DROP} == set(t[5].tolist())
    n_all = len(check(jc.slice_join(jc.P_CS, left=("t", 0, 6), proj=(0, 1, 7))._replace(on=((1, 0),)), [t], "unfiltered"))
    for is_eq, lit in ((True, jc.KEEP), (False, jc.DROP)):
        j = jc.Join(("f", ("t", 0, 6), 5, lit, is_eq), ("s", jc.P_CS), ((1, 0),), "inner", None, (0, 1, 7))
        assert 0 < len(check(j, [t], f"probe filter {is_eq}")) < n_all
    assert jc.POST_LITERAL in jc.SLICES[jc.P_CS][1]
    for is_eq in (True, False):
        j = jc.Join(("t", 0, 6), ("f", ("s", jc.P_CS), 1, jc.POST_LITERAL, is_eq), ((1, 0),), "inner", None, (0, 1, 7))
        want = check(j, [t], f"build filter {is_eq}")
        assert 0 < len(want) < n_all and (len(want) < 10) == is_eq
    # two joins
    for every in (1, 10, 0):
        t = jc.sized_table(1500, True, every)
        lower = check(jc.LOWER, [t], f"lower {every}")
        assert (every == 0) == (len(lower) == 0)
        check(jc.UPPER_PROBE, [t], f"upper probe {every}")
        check(jc.UPPER_BUILD, [t, jc.upper_table()], f"upper build {every}")
    assert len(jc.expected(jc.LOWER, [jc.sized_table(1500, True, 10)])) * 9 < len(jc.expected(jc.LOWER, [jc.sized_table(1500, True, 1)]))
    # one plan, many tables
    for direct, P in ((True, jc.P_D), (False, jc.P_CS)):
        sizes = [len(check(jc.slice_join(P), [jc.sequence_table(name, direct)], f"sequence {name}")) for name in jc.SEQUENCE]
        assert sizes[0] > 300 and sizes[2] == 0 == sizes[4] and 0 < sizes[1] <= 18
    # predicate shapes over the zoo
    for name, pred in jc.PREDICATES.items():
        t = jc.zoo_table(name == "vm")
        want = check(jc.slice_join(jc.P_D, pred, proj=(0, 3, 4, 6)), [t], f"predicate {name}")
        unfiltered = len(jc.expected(jc.slice_join(jc.P_D, None, proj=(0,)), [t]))
        assert 0 < len(want) and (len(want) < unfiltered) == (name != "none"), (name, len(want), unfiltered)          # every filter rejects some pair and keeps some
