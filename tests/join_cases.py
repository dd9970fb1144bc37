"""The fused hash join (lds_join_kernel, join_device.hpp; stream_join_kernel, stream_join.hip) at its queue, tile and table edges: the
store, the bound tables, the plans and the exact expected rows shared by test_join_cases_cpu.py (oracle = reference, and every case
holds the edge it is built for, on a machine without a GPU) and test_gpu_join_edges.py (the device's rows = reference, and the kernel
form that ran is the one the case is built for).

A plan is a Join(left, right, on, how, pred, proj) over inputs: ("t", slot, n_cols) a bound table, ("s", P) the store slice
(?s P ?o) with columns (s, o), ("f", input, col, literal, is_eq) a FilterExec of `col = literal` / `col != literal`, ("j", Join) a
join below.  reference() is a dict from key tuple to right rows and a loop over the left rows; it shares nothing with oracle/ or
the device code.

The store.  Every slice has more than 1024 rows, so that the engine builds on it (choose_build_left, plan_join.cpp) and keeps its table:
  P_D   2070 unique subjects out of the 2300 ids from D0 (every tenth id missing): the direct-address table.  Objects: the twelve
        xsd:integers of the zoo (i64::MIN, i64::MAX, values whose + 3 overflows).
  P_CS  2056 rows over the keys from C0 with the fan-outs FANS (64 keys each for the fan-outs up to 6 and for 0 - ids inside the range
        without a row - two keys each for 7 .. 300): the CSR table.  Its objects rise with the subjects, so the slice (sorted by ?o) is
        sorted by the key as well and the CSR row list is the identity (csr_rows == nullptr).
  P_CU  the same subjects with objects that fall: not sorted by the key, the row list is materialised.
        The objects of both are xsd:integers 0 (even id) and 10 (odd id): the partners of a key alternate.
  P_W   1100 scattered subjects and six of the eight WRAP keys (one twice): no dense id range, a cached hash table.
Geometry of lds_join_kernel (lds_join_body): a tile is 512 x ITEMS >> rl probe rows; with ITEMS = 1 and rl = 0 wave w of a tile owns its
rows 64 w .. 64 w + 63; every fill round takes at most one candidate per lane, so a wave's round r brings as many candidates as it has
rows with more than r partners."""
from collections import namedtuple

import numpy as np

from rdf_fusion_amd import abi
from rdf_fusion_amd.engine import TV_DTYPE
from rdf_fusion_amd.plan import PlanBuilder, quad_pattern, col, lit_id, integer, ENC_TV, LT, ADD, EBV, AND, BOUND, ID_EQ, ID_NEQ
import band_cases as bc
import ordered_cases as oc

I64_MIN, I64_MAX = bc.I64_MIN, bc.I64_MAX
P_D, P_CS, P_CU, P_W = 1, 2, 3, 4
ZOO0 = 16
ZOO_INTS = (I64_MIN, I64_MIN + 1, -4, -1, 0, 1, 2, 3, 5, I64_MAX - 3, I64_MAX - 2, I64_MAX)
INT_IDS = tuple(range(ZOO0, ZOO0 + len(ZOO_INTS)))
ZERO_ID = INT_IDS[ZOO_INTS.index(0)]
DOUBLE_ID, STRING_ID = ZOO0 + len(ZOO_INTS), ZOO0 + len(ZOO_INTS) + 1
ZOO_IDS = INT_IDS + (DOUBLE_ID, STRING_ID)
C0, D0, ND = 1000, 4000, 2300
OBJ_S0, OBJ_U0, N_IDS = 8000, 11000, 14000
FANS = (1, 2, 3, 4, 6, 0, 7, 8, 9, 63, 64, 65, 300)
KEYS = {}                                                   # fan-out -> the keys of P_CS / P_CU that have it
_k = C0
for _f in FANS:
    KEYS[_f] = list(range(_k, _k + (64 if _f <= 6 else 2)))
    _k += len(KEYS[_f])
KMIN_C, KMAX_C, HOLE_C = C0, _k - 1, KEYS[0][0]
D_KEYS = [D0 + i for i in range(ND) if i % 10 != 3]
KMIN_D, KMAX_D, HOLE_D = D_KEYS[0], D_KEYS[-1], D0 + 3
K0L = 20000                                                 # keys of the bound build tables (no typed value: no filter reads them)
LDS_TILE, BIG = 512, 1 << 18


# ---------------------------------------------------------------------------------------------------
# hash_keys4 (join_device.hpp) for one key, restated to place keys, and the wrap keys
# ---------------------------------------------------------------------------------------------------
def hash1(keys):
    k = np.asarray(keys, np.uint64)
    m = np.uint64(0xFFFFFFFF)
    h = ((np.uint64(0x9E3779B9) ^ k) * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


def _wrap_keys():
    ids = np.arange(100_000, 100_000 + (1 << 22), dtype=np.uint64)
    return [int(x) for x in ids[(hash1(ids) & 0x1FFFF) >= (1 << 17) - 2][:8]]


WRAP = _wrap_keys()                                         # home slot = mask - 1 or mask in every table of up to 2^17 slots
WRAP_BUILD = WRAP[:6] + [WRAP[2]]                           # six of them, one twice
W_FILL = [300_000 + 211 * i for i in range(1100)]


def occupied(keys, mask):
    """the slots of an open-addressing table with linear probing that holds `keys` (a set: it does not depend on the insertion order)"""
    occ = set()
    for h in hash1(keys).tolist():
        s = h & mask
        while s in occ:
            s = (s + 1) & mask
        occ.add(s)
    return occ


def walk(key, occ, mask):
    """the slots a probe for `key` reads up to and including the first empty one"""
    s, out = int(hash1([key])[0]) & mask, []
    while True:
        out.append(s)
        if s not in occ:
            return out
        s = (s + 1) & mask


# ---------------------------------------------------------------------------------------------------
# the store
# ---------------------------------------------------------------------------------------------------
def _slices():
    out = {P_D: ([], []), P_CS: ([], []), P_CU: ([], []), P_W: ([], [])}
    for i, s in enumerate(D_KEYS):
        out[P_D][0].append(s); out[P_D][1].append(INT_IDS[(s - D0) % len(INT_IDS)])
    rows = [key for f in FANS for key in KEYS[f] for _ in range(f)]
    for r, s in enumerate(rows):
        out[P_CS][0].append(s); out[P_CS][1].append(OBJ_S0 + r)
        out[P_CU][0].append(s); out[P_CU][1].append(OBJ_U0 + len(rows) - 1 - r)
    for i, s in enumerate(WRAP_BUILD + W_FILL):
        out[P_W][0].append(s); out[P_W][1].append(500_000 + i)
    return {p: [np.asarray(c, np.uint32) for c in sl] for p, sl in out.items()}


SLICES = _slices()
TERMS = [None] * N_IDS
for _i, _v in zip(INT_IDS, ZOO_INTS):
    TERMS[_i] = ("integer", _v)
TERMS[DOUBLE_ID] = ("double", 2.5)
for _o in list(range(OBJ_S0, OBJ_S0 + 2056)) + list(range(OBJ_U0, OBJ_U0 + 2056)):
    TERMS[_o] = ("integer", 10 * (_o % 2))


def quads():
    s = np.concatenate([SLICES[p][0] for p in SLICES]); o = np.concatenate([SLICES[p][1] for p in SLICES])
    p = np.concatenate([np.full(len(SLICES[q][0]), q, np.uint32) for q in SLICES])
    order = np.random.default_rng(7).permutation(len(s))
    return np.zeros(len(s), np.uint32), s[order], p[order], o[order]


def typed_values():
    tv = np.zeros(N_IDS, dtype=TV_DTYPE)
    tv["tag"][1:] = abi.TV_NAMED_NODE
    tv["lo"][1:] = np.arange(1, N_IDS)
    for i, t in enumerate(TERMS):
        if t is not None and t[0] == "integer":
            tv["tag"][i] = abi.TV_INTEGER; tv["lo"][i] = t[1]
    tv["tag"][DOUBLE_ID] = abi.TV_DOUBLE; tv["lo"][DOUBLE_ID] = np.float64(2.5).view(np.int64)
    tv["tag"][STRING_ID] = abi.TV_STRING; tv["lo"][STRING_ID] = 0
    return tv, np.zeros(0, np.int64)


def fill_store(store):
    store.extend(*quads())
    store.set_typed_values(*typed_values())
    return store


# ---------------------------------------------------------------------------------------------------
# plans and predicates: each predicate is a plan expression and a Python function over Python ints
# ---------------------------------------------------------------------------------------------------
Join = namedtuple("Join", "left right on how pred proj", defaults=("inner", None, None))
W3 = bc.Window("lt+3_gt-3", "LT", False, 3, "GT", True, 3)             # |x - ya| < 3, both halves on ya
W3_TWO = bc.Window("leq+3_geq-3_two", "LEQ", False, 3, "GEQ", True, 3, True)   # x <= ya + 3 and x >= yb - 3


def width(inp):
    return inp[2] if inp[0] == "t" else 2 if inp[0] == "s" else width(inp[1]) if inp[0] == "f" else len(inp[1].proj)


def pred_expr(pred):
    if pred is None:
        return None
    if pred[0] == "id":
        return (ID_EQ if pred[1] else ID_NEQ)(col(pred[2]), col(pred[3]))
    if pred[0] == "win":
        return bc.window_expr(pred[1], pred[2], pred[3], pred[4])
    a, b, c = pred[1:]
    return AND(EBV(LT(ENC_TV(col(a)), ADD(ENC_TV(col(b)), integer(3)))), BOUND(col(c)))


def _term(i):
    return TERMS[i] if 0 < i < N_IDS else None


def pred_fn(pred):
    """(left row, right row) -> the predicate is true (an error or an unbound operand is not)"""
    if pred is None:
        return None
    if pred[0] == "id":
        _, is_eq, a, b = pred
        return lambda l, r: (l + r)[a] != 0 and (l + r)[b] != 0 and ((l + r)[a] == (l + r)[b]) == is_eq
    if pred[0] == "win":
        _, w, x, ya, yb = pred
        return lambda l, r: bc.window_holds(w, _term((l + r)[x]), _term((l + r)[ya]), _term((l + r)[yb]))
    _, a, b, c = pred
    return lambda l, r: (l + r)[c] != 0 and bc._holds("LT", _term((l + r)[a]), bc._arith(_term((l + r)[b]), ("integer", 3), False))


def _node(pb, inp):
    if inp[0] == "t":
        return pb.table(inp[1], inp[2])
    if inp[0] == "s":
        return pb.data_source(quad_pattern("s", inp[1], "o"))
    if inp[0] == "f":
        child = _node(pb, inp[1])
        return pb.filter(child, (ID_EQ if inp[4] else ID_NEQ)(col(inp[2]), lit_id(inp[3])), projection=list(range(width(inp))))
    j = inp[1]
    return pb.hash_join(_node(pb, j.left), _node(pb, j.right), on=list(j.on), join_type=abi.JOIN_LEFT if j.how == "left" else abi.JOIN_INNER,
                        filter=pred_expr(j.pred), projection=list(j.proj))


def plan_of(join):
    pb = PlanBuilder()
    return pb.build(_node(pb, ("j", join)))


# ---------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------
def reference(left, right, on, join_type="inner", predicate=None, projection=None):
    """left, right: lists of columns.  -> the rows [left columns, right columns][projection] as tuples, a multiset.  NullEqualsNothing: a 0 in any
    key column never matches; join_type "left": a left row without a surviving partner comes out once with 0 in every right column.  An inner
    join of more than 2^18 rows on a side first drops that side's rows whose key is 0 or not among the other side's (np.isin); what is left
    goes through the dict and the loop unchanged."""
    L, R = [np.asarray(c) for c in left], [np.asarray(c) for c in right]
    if join_type == "inner":
        for side, other, mine in ((L, R, 0), (R, L, 1)):
            if side and len(side[0]) > BIG:
                keep = np.ones(len(side[0]), bool)
                for pair in on:
                    keep &= (side[pair[mine]] != 0) & np.isin(side[pair[mine]], other[pair[1 - mine]])
                side[:] = [c[keep] for c in side]
    lrows, rrows = list(zip(*[c.tolist() for c in L])), list(zip(*[c.tolist() for c in R]))
    by_key = {}
    for r in rrows:
        k = tuple(r[b] for _, b in on)
        if 0 not in k:
            by_key.setdefault(k, []).append(r)
    proj = list(range(len(L) + len(R))) if projection is None else list(projection)
    nulls, out = (0,) * len(R), []
    for l in lrows:
        k, n = tuple(l[a] for a, _ in on), 0
        if 0 not in k:
            for r in by_key.get(k, ()):
                if predicate is None or predicate(l, r):
                    row = l + r
                    out.append(tuple(row[p] for p in proj)); n += 1
        if join_type == "left" and n == 0:
            row = l + nulls
            out.append(tuple(row[p] for p in proj))
    return out


def columns_of(inp, tables):
    if inp[0] == "t":
        return [np.asarray(c, np.uint32) for c in tables[inp[1]]]
    if inp[0] == "s":
        return SLICES[inp[1]]
    if inp[0] == "f":
        cols = columns_of(inp[1], tables)
        v = cols[inp[2]]
        keep = (v != 0) & ((v == inp[3]) == bool(inp[4]))                      # (a null is neither equal nor different)
        return [c[keep] for c in cols]
    rows = expected(inp[1], tables)
    return [np.asarray(c, np.uint32) for c in zip(*rows)] if rows else [np.zeros(0, np.uint32)] * len(inp[1].proj)


def expected(join, tables):
    return reference(columns_of(join.left, tables), columns_of(join.right, tables), join.on, join.how, pred_fn(join.pred), join.proj)


def assert_rows(got_cols, want, n_cols, what=""):
    oc.assert_multiset(got_cols, want, range(n_cols), what)


# ---------------------------------------------------------------------------------------------------
# tables over the slices: (tag, key, x, ya, yb[, flag])
# ---------------------------------------------------------------------------------------------------
STRANGERS_C = (0, KMIN_C - 1, HOLE_C, KMAX_C + 1, 0xFFFFFFFF, 1)
STRANGERS_D = (0, KMIN_D - 1, HOLE_D, KMAX_D + 1, 0xFFFFFFFF, 1)
KEEP, DROP = 7, 8


def ckey(fan, i):
    """a key of the CSR slices with `fan` partners (fan 0: one of the strangers)"""
    return KEYS[fan][i % len(KEYS[fan])] if fan else STRANGERS_C[i % len(STRANGERS_C)]


def dkey(fan, i):
    """a key of the direct slice (fan 1) or a stranger to it (fan 0)"""
    return D_KEYS[(37 * i) % len(D_KEYS)] if fan else STRANGERS_D[i % len(STRANGERS_D)]


def table_of(keys, flags=None):
    n = len(keys)
    i = np.arange(n)
    x = np.where(i % 9 == 4, 0, 7).astype(np.uint32)                           # never an object; some unbound
    cols = [np.arange(1, n + 1, dtype=np.uint32), np.asarray(keys, np.uint32), x, np.full(n, ZERO_ID, np.uint32),
            np.asarray(ZOO_IDS, np.uint32)[i % len(ZOO_IDS)] if n else np.zeros(0, np.uint32)]
    return cols + ([np.asarray(flags, np.uint32)] if flags is not None else [])


def slice_join(p, pred=None, proj=(0, 1, 6), how="inner", left=("t", 0, 5)):
    return Join(left, ("s", p), ((1, 0),), how, pred, proj)


FILTERS = {"none": None, "all": ("id", True, 2, 6), "alt": ("win", W3, 6, 3, 3)}   # FS 0; FS 2: x is never ?o; FS 3: ?o is 0 or 10, ya is 0

# -- group 1: the queue ---------------------------------------------------------------------------------
PATTERNS = {"m1": [1] * 64, "m2": [2] * 64, "m3": [3] * 64, "m6": [6] * 64, "mod5": [l % 5 for l in range(64)], "hot": [300] + [0] * 63}
WAVE_ROWS = (512, 513, 575)


def wave_fans(n, pattern):
    """fan-out per probe row: the pattern on waves 0 and 7 of the first tile and on the live lanes of the last, partial tile; 0 elsewhere"""
    fans = [0] * n
    for i in range(n):
        if i < 512 and i // 64 in (0, 7) or i >= 512:
            fans[i] = PATTERNS[pattern][i % 64]
    return fans


def wave_table(n, pattern, key=ckey):
    return table_of([key(f, i) for i, f in enumerate(wave_fans(n, pattern))])


def rounds(fans, outer=False):
    """candidates per fill round of a wave whose rows have these fan-outs; outer: a row without a partner brings its null row in round 0"""
    c = [max(f, 1) if outer else f for f in fans]
    return [sum(x > r for x in c) for r in range(max(c, default=0))]


def queue_trace(round_counts, q):
    """-> [(candidates queued before the round, candidates of the round, the round was pended)]: `qn + n_found > qcap` (lds_join_body)
    hands the round over in pend[] and resolves the queue first"""
    qn, out = 0, []
    for n in round_counts:
        pended = qn + n > q
        out.append((qn, n, pended))
        qn = n if pended else qn + n
    return out


# -- group 2: output capacity ----------------------------------------------------------------------------
def _reachable(total, n_rows):
    """n_rows fan-outs out of 0, 1, 2, 3, 4 and 6 can add up to total"""
    return 0 <= total <= 6 * n_rows and (total != 6 * n_rows - 1 or n_rows == 0)


def fans_with_total(n_rows, total):
    fans = []
    for i in range(n_rows):
        left = n_rows - i - 1
        f = next(f for f in (6, 4, 3, 2, 1, 0) if f <= total and _reachable(total - f, left))
        fans.append(f); total -= f
    assert total == 0
    return fans


def total_table(n_rows, total):
    return table_of([ckey(f, i) for i, f in enumerate(fans_with_total(n_rows, total))])


def spec_cap(prev):
    return max(1024, prev + prev // 4 + 256)                                   # run_speculative (plan_join.cpp): 25 % head room + 256


# -- group 3: the LDS table ------------------------------------------------------------------------------
LDS_BUILDS = (1, 1024, 1025, 4096, 4097, 8192, 8193)
TABLE_JOIN = Join(("t", 0, 2), ("t", 1, 2), ((0, 0),), "inner", None, (0, 1, 3))


def lds_build(n, keys=None):
    return [np.asarray(keys if keys is not None else K0L + np.arange(n), np.uint32), 30000 + np.arange(n, dtype=np.uint32)]


def lds_probe(n_build, n=None):
    n = n if n is not None else max(n_build, 1024) + 549
    i = np.arange(n, dtype=np.int64)
    key = np.where(i % 11 == 5, 0, K0L + (7 * i) % (n_build + 50)).astype(np.uint32)
    key[[0, n - 1]] = [K0L, K0L + n_build - 1]                                 # the first and the last build row have partners
    return [key, np.arange(1, n + 1, dtype=np.uint32)]


def lds_slots(n_build):
    """choose_join_table: load <= 0.5, LDS tables load <= 0.25 and at least 2048 slots while that stays within 16384"""
    s = 64
    while s < 2 * n_build:
        s <<= 1
    while (s < 4 * n_build or s < 2048) and s < 16384:
        s <<= 1
    return s


def one_key_tables():
    """8192 build rows on one key; three probe rows with it, a null, and 8188 rows whose key is absent (the engine builds on the side
    that is not larger): an 8192-hop chain, 24576 rows"""
    probe = np.full(8192, K0L + 1, np.uint32)
    probe[[0, 4000, 8191]] = K0L; probe[3] = 0
    return [lds_build(8192, np.full(8192, K0L)), [probe, np.arange(1, 8193, dtype=np.uint32)]]


# -- group 4: wrap-around --------------------------------------------------------------------------------
def wrap_tables():
    return [lds_build(len(WRAP_BUILD), WRAP_BUILD), [np.asarray(WRAP + [0, 99], np.uint32), np.arange(1, 11, dtype=np.uint32)]]


def wrap_table():
    return table_of(WRAP + [0, 99])


# -- group 5: several tiles per workgroup -----------------------------------------------------------------
TILE_PROBES = (256 * 512, 256 * 512 + 1, 2 * 256 * 512 + 513)
TILE_JOIN = {1: Join(("t", 0, 3), ("t", 1, 3), ((0, 0),), "inner", None, (0, 2, 5)),
             2: Join(("t", 0, 3), ("t", 1, 3), ((0, 0), (1, 1)), "inner", None, (0, 2, 5))}


def tile_build():
    """8192 rows: 128 keys twice, then unique keys; second key 7"""
    i = np.arange(8192)
    key = np.where(i < 256, K0L + i // 2, K0L + 128 + i - 256)
    return [key.astype(np.uint32), np.full(8192, 7, np.uint32), 30000 + i.astype(np.uint32)]


def tile_chosen(n):
    """probe row -> key: the first and last row of the first tile, the single row of workgroup 0's second tile, the last row overall,
    one full wave (3) of workgroup 0's third tile with two partners per row"""
    rows = {0: K0L + 200, 511: K0L + 201, n - 1: K0L + 203}
    if n > 256 * 512:
        rows[256 * 512] = K0L + 202
    if n > 512 * 512 + 256:
        for lane in range(64):
            rows[512 * 512 + 192 + lane] = K0L + lane
    return rows


def tile_probe(n):
    i = np.arange(n)
    key = np.where(i % 2 == 0, 0, K0L - 1).astype(np.uint32)
    k2 = np.full(n, 7, np.uint32)
    for r, k in tile_chosen(n).items():
        key[r] = k
    key[1] = K0L + 300; k2[1] = 8                                              # agrees on the first key only
    key[2] = K0L + 301; k2[2] = 0
    return [key, k2, np.arange(1, n + 1, dtype=np.uint32)]


# -- group 6: ITEMS = 4 ----------------------------------------------------------------------------------
BIG_ROWS = ((1 << 20) - 1, 1 << 20, (1 << 20) + 1)
ITEMS_TILE = 3                                                                 # the 2048-row tile whose wave 3 is filled
ITEMS_JOIN = Join(("t", 0, 2), ("t", 1, 4), ((0, 3),), "inner", None, (0, 1, 2))
K6 = K0L + 9000


def items_build():
    """1100 rows, every key twice"""
    return lds_build(1100, K6 + np.arange(1100) // 2)


def big_table(n):
    """(tag, kd, kc, kl): keys into the direct slice, the CSR slices and items_build(); 0 or absent but for a few thousand rows"""
    i = np.arange(n, dtype=np.int64)
    kd = np.where(i % 2 == 0, 0, KMAX_D + 1)
    hit = i % 997 == 0
    kd[hit] = D0 + (i[hit] // 997) % ND
    for r in (4095, 4096, n - 1):
        kd[r] = D_KEYS[r % len(D_KEYS)]
    kc = np.where(i % 2 == 0, KMIN_C - 1, 0)
    hit = i % 1499 == 0
    kc[hit] = [ckey((1, 2, 3, 0, 7)[j % 5], j) for j in range(int(hit.sum()))]
    for r in (2047, 2048, n - 1):
        kc[r] = KEYS[2][r % 64]
    kl = np.where(i % 2 == 0, 0, K6 - 1)
    for item in range(4):
        rows = ITEMS_TILE * 2048 + item * 512 + 192 + np.arange(64)
        kl[rows] = K6 + (64 * item + np.arange(64)) % 550
    kl[n - 1] = K6 + 549
    return [np.arange(1, n + 1, dtype=np.uint32)] + [c.astype(np.uint32) for c in (kd, kc, kl)]


def lanes_big_table(n):
    """65535 / 65536 rows against the CSR slice with 64 lanes per row: every 251st row has partners"""
    keys = [ckey((1, 63, 64, 65, 300, 2)[(i // 251) % 6], i) if i % 251 == 0 or i == n - 1 else (0, KMAX_C + 1)[i % 2] for i in range(n)]
    return table_of(keys)


# -- group 7: lanes per CSR row ---------------------------------------------------------------------------
ROW_LANES = (0, 1, 3, 6)


def lane_fans(rl):
    return sorted({0, 1, (1 << rl) - 1, 1 << rl, (1 << rl) + 1, 300})


def lane_rows(rl):
    t = 512 >> rl
    return (t - 1, t, t + 1, 3 * t + 1)


def lanes_table(rl, n):
    fans = lane_fans(rl)
    return table_of([0 if i % 13 == 7 else ckey(fans[i % len(fans)], i) for i in range(n)])


# -- group 8: dense-table bounds --------------------------------------------------------------------------
def bounds_table(direct):
    kmin, kmax, hole = (KMIN_D, KMAX_D, HOLE_D) if direct else (KMIN_C, KMAX_C, HOLE_C)
    edge = [kmin, kmax, kmin - 1, kmax + 1, 0, 1, 0xFFFFFFFF, hole]
    return table_of(edge + [(dkey if direct else ckey)(1, i) for i in range(20)] + edge[::-1])


# -- group 9: key columns --------------------------------------------------------------------------------
def key_tables():
    """build (k0, k1, k2, k3, payload) of 600 rows, probe (k0, k1, k2, k3, tag) of 1300: k0 = 5 everywhere, k1 = 6 and k2 = 7 but for a few
    rows, k3 varies; a 0 in the last key only on either side"""
    def side(n, mod):
        i = np.arange(n)
        k1 = np.where(i % 41 == 3, 9, 6); k2 = np.where(i % 43 == 5, 9, 7)
        k3 = 100 + i % mod
        k3[i % 29 == 11] = 0
        return [np.full(n, 5, np.uint32)] + [c.astype(np.uint32) for c in (k1, k2, k3)] + [np.arange(1, n + 1, dtype=np.uint32)]
    return [side(600, 450), side(1300, 500)]


def key_join(n_keys, how):
    on = ((0, 0), (1, 1), (2, 2), (3, 3))
    return Join(("t", 0, 5), ("t", 1, 5), (on[0],) + on[5 - n_keys:], how, None, (4, 3, 9, 8))


# -- group 10: output columns ----------------------------------------------------------------------------
PROJECTIONS = {1: (6,), 4: (0, 6, 1, 5), 5: (6, 0, 5, 1, 2), 8: (0, 1, 2, 3, 4, 5, 6, 0), 9: (6, 5, 4, 3, 2, 1, 0, 6, 1)}


# -- group 11: left joins --------------------------------------------------------------------------------
def left_fans(name, fan_max):
    """513 rows: the first wave as named, matched rows behind it, the one row of the second tile without a partner"""
    first = {"unmatched64": [0] * 64, "pend_null": [min(2, fan_max)] * 17 + [0] + [min(2, fan_max)] * 46, "mixed": [l % 3 % (fan_max + 1) for l in range(64)]}[name]
    return first + [1 if i % 5 else 0 for i in range(448)] + [0]


def left_table(name, direct):
    fans = left_fans(name, 1 if direct else 6)
    return table_of([(dkey if direct else ckey)(f, i) for i, f in enumerate(fans)])


def classic_left_tables():
    """600 left rows (the build side), 1300 right rows; a third of the left keys have no partner, some are 0"""
    i, j = np.arange(600), np.arange(1300)
    lk = np.where(i % 7 == 2, 0, K0L + i % 400).astype(np.uint32)
    rk = np.where(j % 9 == 1, 0, K0L + 130 + j % 500).astype(np.uint32)
    return [[lk, 30000 + i.astype(np.uint32)], [rk, np.arange(1, 1301, dtype=np.uint32)]]


# -- group 12: fused filters of the inputs ------------------------------------------------------------------
def flagged_wave_table(n=513):
    fans = wave_fans(n, "mod5")
    return table_of([ckey(f, i) for i, f in enumerate(fans)], flags=[(KEEP, DROP, 0, KEEP)[i % 4] for i in range(n)])


POST_LITERAL = OBJ_S0 + 1                                                      # the object of the one row of KEYS[1][1] in P_CS


# -- groups 13 and 14: sized tables ------------------------------------------------------------------------
def sized_table(m, direct, match_every=1):
    """m rows; every match_every-th has a partner (0: none has), an edge key every 17 rows"""
    strangers = STRANGERS_D if direct else STRANGERS_C
    keys = []
    for i in range(m):
        if i % 17 == 16 or match_every == 0 or i % match_every:
            keys.append(strangers[i % len(strangers)])
        else:
            keys.append(dkey(1, i) if direct else ckey((1, 2, 3, 1, 6)[i % 5], i))
    t = table_of(keys)
    t[2] = np.asarray([ckey((1, 2, 0, 3)[i % 4], i) for i in range(m)], np.uint32) if m else t[2]   # x: a key of the CSR slices (the upper join of group 13)
    return t


LOWER = Join(("t", 0, 5), ("s", P_D), ((1, 0),), "inner", None, (0, 2, 6))    # -> (tag, x, ?o of P_D)
UPPER_PROBE = Join(("j", LOWER), ("s", P_CS), ((1, 0),), "inner", None, (0, 1, 2, 4))
UPPER_BUILD = Join(("j", LOWER), ("t", 1, 2), ((1, 0),), "inner", None, (0, 2, 4))


def upper_table():
    """4000 rows (key, tag) over the CSR slices' keys: larger than the lower join's output, so that output is the build side"""
    return [np.asarray([ckey((1, 2, 0, 3, 4)[i % 5], i // 5) for i in range(4000)], np.uint32), np.arange(1, 4001, dtype=np.uint32)]


SEQUENCE = ("big", "three", "empty", "big", "nothing", "big", "big")


def sequence_table(name, direct):
    return {"big": lambda: sized_table(500, direct), "three": lambda: sized_table(3, direct), "empty": lambda: table_of([]),
            "nothing": lambda: sized_table(40, direct, 0)}[name]()


# -- the predicate shapes over the zoo -----------------------------------------------------------------------
def zoo_table(ints_only):
    """every pair (ya, yb) of the zoo's ids against direct keys whose ?o run through the twelve integers"""
    ids = INT_IDS if ints_only else ZOO_IDS
    rows = [(a, b) for a in ids for b in ids]
    t = table_of([D_KEYS[(5 * i) % len(D_KEYS)] for i in range(len(rows) * 12)])
    t[3] = np.asarray([rows[i // 12][0] for i in range(len(t[0]))], np.uint32)
    t[4] = np.asarray([rows[i // 12][1] for i in range(len(t[0]))], np.uint32)
    return t


PREDICATES = {"none": None, "id_eq": ("id", True, 3, 6), "id_neq": ("id", False, 4, 6), "window": ("win", W3, 6, 3, 3),
              "window_two": ("win", W3_TWO, 6, 3, 4), "vm": ("vm", 6, 3, 2)}
