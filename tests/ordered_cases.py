"""The ordered slice join (ordered_join.hip) at its tile, chain and record edges: the stores, tables, plans and the exact expected rows
shared by test_ordered_join_cpu.py (oracle = reference, on a machine without a GPU) and test_gpu_ordered_join_edges.py (the device's
rows, in the slice's order, = reference).

The plan:  T(tag, key, k1, k2, k3) JOIN (?s P_LINK ?o) ON key = ?s  [JOIN (?s P_Ak ?vk) ON kk = ?s, k = 1 .. n_stages]
with any projection of (tag, key, k1, k2, k3, s, o, v1, v2, v3).  The link slice is the GPOS one: sorted by ?o, ties by ?s, and joined on
?s; the device form streams it in that order, 1024 rows per tile (256 lanes x 4 rounds), and emits for every slice row the chain of the
table rows with its key, so its output is the slice's rows in order, each repeated by its chain length.

Geometry.  Slice row i has object O0 + i // 4, so every object has four rows (the last one may have fewer) and the ties in ?o are broken
by ?s.  An ordinary subject belongs to one tile and one of the four places of an object: M0 + 512 tile + 128 place + group % 128 - two
rows in a full tile, 512 slice rows apart.  The special subjects sit at chosen rows: the low ones (ids below every ordinary subject) on the
first row of an object, the high ones (ids above) on the last.  LA has rows 0, 256 and 1024, HA rows 255 and 1023: the long chains hang on
these.  LB (row 2048), HB (2047), HC (3071), LM[t] (1024 t + 512), LR (768) and HR (511) have one row each.  Every look-up predicate has
1200 unique subjects out of 1400 ids (above 1024 rows: a cached direct-address table, so the chain fuses), the link slice has more than
1024 rows with repeated subjects (the CSR form), and the subjects start at 100."""
from collections import namedtuple

import numpy as np

from rdf_fusion_amd import abi
from rdf_fusion_amd.engine import TV_DTYPE
from rdf_fusion_amd.plan import PlanBuilder, quad_pattern, col, lit_id, ID_EQ
import band_cases as bc

P_LINK, P_A = 50_001, (50_002, 50_003, 50_004)
TILE, PLACES, BAND = 1024, 4, 128
S0, N_LOW = 100, 16                                   # the first subject: kmin - 1 = 99 is an id of its own, and not the null id
M0 = S0 + N_LOW                                       # ordinary subjects M0 .. H0 - 1
H0 = M0 + 3 * PLACES * BAND
O0, A0, NA, V0 = 10_000, 3_000, 1_400, 20_000
SLICE_ROWS = (1025, 2047, 2048, 2049, 3072)
LA, LB, LR, HOLE = S0, S0 + 1, S0 + 5, S0 + 10        # HOLE: inside the key range, on no slice row
LM = (S0 + 2, S0 + 3, S0 + 4)
HA, HB, HC, HR = H0, H0 + 1, H0 + 2, H0 + 3
SPECIAL_ROWS = {0: LA, 256: LA, 1024: LA, 255: HA, 1023: HA, 2048: LB, 2047: HB, 3071: HC, 512: LM[0], 1536: LM[1], 2560: LM[2], 768: LR, 511: HR}
CHAIN_ROWS = (0, 255, 256, 1023, 1024)                # the slice rows of LA and HA
CHAINS = (254, 255, 256, 300)
KEEP, DROP = 7, 8                                     # the flag column of a table that goes through a FilterExec
COLUMNS = ("tag", "key", "k1", "k2", "k3", "s", "o", "v1", "v2", "v3")


# ---------------------------------------------------------------------------------------------------
# the store
# ---------------------------------------------------------------------------------------------------
class Slice:
    """The link slice of `n` rows in its own order: s[i], o[i]; rows_of[subject] = its slice rows"""
    def __init__(self, n):
        self.n = n
        self.s, self.o = [], []
        for i in range(n):
            tile, group, place = i // TILE, (i % TILE) // PLACES, i % PLACES
            self.s.append(SPECIAL_ROWS.get(i, M0 + (tile * PLACES + place) * BAND + group % BAND))
            self.o.append(O0 + i // PLACES)
        self.rows_of = {}
        for i, s in enumerate(self.s):
            self.rows_of.setdefault(s, []).append(i)
        self.kmin, self.kmax = min(self.s), max(self.s)
        self.tiles = (n + TILE - 1) // TILE

    def subjects(self, tile=None, rows=None):
        """sorted subjects [all of whose rows are in `tile`] [with `rows` slice rows]"""
        return [s for s, r in sorted(self.rows_of.items()) if (tile is None or all(i // TILE == tile for i in r)) and (rows is None or len(r) == rows)]

    def pairs(self, tile):
        """ordinary subjects with two rows, both in `tile`"""
        return [s for s in self.subjects(tile, 2) if M0 <= s < H0]


_SLICES = {}


def slice_of(n):
    if n not in _SLICES:
        _SLICES[n] = Slice(n)
    return _SLICES[n]


def stage_rows(k):
    """(?s P_A[k] ?v): subject -> value; one subject in seven has no row"""
    return {A0 + j: V0 + (13 * j + 5 * k) % 97 for j in range(NA) if (j + k) % 7 != 3}


STAGES = tuple(stage_rows(k) for k in range(3))


def stage_edge_keys(k):
    """null, below and above the stage's id range, in range without a row"""
    return (0, A0 - 1, A0 + NA, A0 + (3 - k) % 7)


def quads(n):
    """(g, s, p, o) of the store with a link slice of n rows, in no particular order"""
    sl = slice_of(n)
    s, p, o = list(sl.s), [P_LINK] * n, list(sl.o)
    for k, rows in enumerate(STAGES):
        s += list(rows); p += [P_A[k]] * len(rows); o += list(rows.values())
    order = np.random.default_rng(n).permutation(len(s))
    u32 = lambda x: np.asarray(x, np.uint32)[order]
    return np.zeros(len(s), np.uint32), u32(s), u32(p), u32(o)


# ---------------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------------
def table(keys, clean=(), flags=None):
    """(tag, key, k1, k2, k3[, flag]) with tag = 1 .. n.  The stage keys of a row have rows in their slices, except that every fourth row has
    one edge key (stage_edge_keys) in one of its stages; the rows of the keys in `clean` have none, so that their chain lengths hold with
    any number of stages."""
    clean = set(clean)
    cols = [[], [], [], [], []]
    for i, key in enumerate(keys):
        cols[0].append(i + 1); cols[1].append(key)
        for k in range(3):
            if key not in clean and i % 4 == 1 and (i // 4) % 3 == k:
                sk = stage_edge_keys(k)[(i // 12) % 4]
            else:
                j = (7 * i + 11 * k) % (NA - 1)
                sk = A0 + (j if (j + k) % 7 != 3 else j + 1)
            cols[2 + k].append(sk)
    if flags is not None:
        cols.append(list(flags))
    return [np.asarray(c, np.uint32) for c in cols]


def edge_keys(sl):
    return [0, sl.kmin - 1, sl.kmin, sl.kmax, sl.kmax + 1, 0xFFFFFFFF, HOLE]


def strangers(sl):
    """keys that join nothing"""
    return [0, sl.kmin - 1, sl.kmax + 1, 0xFFFFFFFF, HOLE]


def t_mixed(sl):
    """a quarter of the subjects once, a twelfth twice (the second row far from the first), every special subject, every edge key"""
    subj = sl.subjects()
    special = [s for s in subj if not M0 <= s < H0]
    twice = [s for u, s in enumerate(subj) if u % 12 == 5]
    keys = [s for u, s in enumerate(subj) if u % 4 == 0] + twice
    return table(keys[:len(keys) // 2] + edge_keys(sl) + special + keys[len(keys) // 2:] + twice[::-1], clean=special)


def t_chain(sl, c):
    """c rows on LA (slice rows 0, 256, 1024) and c on HA (255, 1023), interleaved, a stranger every 50 rows"""
    keys = []
    for i in range(c):
        keys += [LA, HA] + ([strangers(sl)[(i // 50) % 5]] if i % 50 == 49 else [])
    return table(keys, clean=(LA, HA))


def t_gap(sl):
    """matches in the first and the last tile, none in the tile between"""
    last = sl.tiles - 1
    tail = sl.pairs(last)[:40] if sl.pairs(last) else [LB, LB]
    return table(sl.pairs(0)[:40] + tail, clean=tail)


def t_only(sl, subject):
    """two rows on a subject with one slice row (HB: q = 1023 of the second tile; LB: q = 0 of the third), some matches in the first tile"""
    return table(sl.pairs(0)[:15] + [subject] + sl.pairs(0)[15:30] + [subject], clean=[subject])


TOTALS = (255, 256, 257)


def tile_total_of(sl, tile):
    return TOTALS[(tile + SLICE_ROWS.index(sl.n)) % 3]


def t_totals(sl):
    """every full tile has 255, 256 or 257 matches: one row on total / 2 two-row subjects, and on LM[tile] if the total is odd"""
    keys = []
    for tile in range(sl.n // TILE):
        total = tile_total_of(sl, tile)
        keys += sl.pairs(tile)[:total // 2] + ([LM[tile]] if total % 2 else [])
    return table(keys, clean=keys)


def t_lone_chains(sl):
    """300 rows on LM[0], 255 on LM[1], 254 on LM[2] (q = 512, one slice row each) and nothing else: a long chain next to rows without matches"""
    keys = []
    for tile, c in zip(range(sl.n // TILE), (300, 255, 254)):
        keys += [LM[tile]] * c
    return table(keys, clean=LM)


def t_rows(sl, total):
    """a table whose join has exactly `total` rows"""
    keys = sl.pairs(0)[:total // 2] + ([LM[0]] if total % 2 else [])
    return table(keys, clean=keys)


def t_warm(sl):
    """every subject of the first tile once (about 1000 matches): what a plan runs first, so that its next execution takes the ordered form
    with room for 1500 rows"""
    keys = sl.subjects(0)
    return table(keys, clean=keys)


def t_sized(sl, m, flags=None):
    """m rows over the slice's subjects, an edge key every 17 rows"""
    subj = sl.subjects()
    keys = [edge_keys(sl)[(i // 17) % 7] if i % 17 == 16 else subj[(5 * i) % len(subj)] for i in range(m)]
    return table(keys, flags=flags)


def t_nothing(sl):
    return table(strangers(sl) * 8)


Case = namedtuple("Case", "name rows table")


def cases_of(n):
    """the tables of the slice with n rows"""
    sl = slice_of(n)
    out = [("mixed", t_mixed(sl))] + [(f"chain{c}", t_chain(sl, c)) for c in CHAINS]
    out += [("totals", t_totals(sl)), ("lone_chains", t_lone_chains(sl)), ("empty", table([])), ("nothing", t_nothing(sl)), ("three", t_sized(sl, 3))]
    if sl.tiles == 3:
        out += [("gap", t_gap(sl)), ("only_q0", t_only(sl, LB))]
    if n >= 2048:
        out += [("only_q1023", t_only(sl, HB))]
    return [Case(name, n, t) for name, t in out]



def case_id(c):
    return f"{c.rows}-{c.name}"


# ---------------------------------------------------------------------------------------------------
# plans
# ---------------------------------------------------------------------------------------------------
# every column count 1 .. 8 (one oj_write_kernel<N> each) and 9 (not eligible); 0, 4, 5 and 8 words of the packed record (= columns that
# are not the slice's); a column twice.  A projection with v_k needs k stages: the ones below stand in with fewer.
PROJECTIONS = {
    "o": ("o",),
    "tag": ("tag",),
    "s_o": ("s", "o"),
    "tag_o_s": ("tag", "o", "s"),
    "4_table_cols": ("tag", "key", "k1", "k2"),
    "twice": ("tag", "o", "tag", "s", "key"),
    "4_words": ("tag", "key", "o", "k1", "k2", "s"),
    "5_words": ("tag", "key", "k1", "k2", "k3", "o", "s"),
    "8_cols": ("tag", "s", "key", "o", "k1", "k2", "k3", "tag"),
    "8_words": ("tag", "key", "k1", "k2", "k3", "v1", "v2", "v3"),
    "stage_values": ("v3", "o", "s", "tag", "v1", "v2"),
    "9_cols": ("tag", "key", "k1", "k2", "k3", "s", "o", "tag", "key"),
}
_STAND_IN = {"v1": "tag", "v2": "key", "v3": "k1"}


def projection(name, n_stages):
    """the columns of projection `name` under a plan with n_stages look-ups: v_k of a stage the plan does not have becomes a table column"""
    return tuple(_STAND_IN[c] if c[0] == "v" and int(c[1]) > n_stages else c for c in PROJECTIONS[name])


def words(proj):
    """words of the packed table record: the output columns taken from the table row or a stage row"""
    return sum(c not in ("s", "o") for c in proj)


def eligible(proj):
    return len(proj) <= 8 and words(proj) <= 8


def ordered_plan(n_stages, proj, flagged=False):
    """proj: column names out of COLUMNS.  flagged: the table has a sixth column and goes through FilterExec(flag = KEEP), which drops it"""
    pb = PlanBuilder()
    scan = lambda p: pb.data_source(quad_pattern("s", p, "v"))
    t = pb.filter(pb.table(0, 6), ID_EQ(col(5), lit_id(KEEP)), projection=[0, 1, 2, 3, 4]) if flagged else pb.table(0, 5)
    names = list(COLUMNS[:7])
    if n_stages == 0:
        return pb.build(pb.hash_join(t, scan(P_LINK), on=[(1, 0)], projection=[names.index(c) for c in proj]))
    node = pb.hash_join(t, scan(P_LINK), on=[(1, 0)], projection=list(range(7)))
    for k in range(1, n_stages + 1):
        full = names + ["", f"v{k}"]
        names = names + [f"v{k}"]
        out = names if k < n_stages else list(proj)
        node = pb.hash_join(node, scan(P_A[k - 1]), on=[(1 + k, 0)], projection=[full.index(c) for c in out])
    return pb.build(node)


# ---------------------------------------------------------------------------------------------------
# the reference: dicts and loops over Python ints
# ---------------------------------------------------------------------------------------------------
def reference(n, tab, n_stages, proj):
    """The rows of the plan over the slice with n rows and table `tab` (a sixth column is the flag of the FilterExec),
    in the slice's order: the slice's rows by (o, s), for each the table rows with its key, non-null, for which every stage has a row."""
    sl = slice_of(n)
    rows = list(zip(*[c.tolist() for c in tab[:5]]))
    if len(tab) > 5:
        rows = [r for r, flag in zip(rows, tab[5].tolist()) if flag == KEEP]
    by_key = {}
    for r in rows:
        if r[1] == 0:
            continue
        vs = []
        for k in range(n_stages):
            if r[2 + k] == 0 or r[2 + k] not in STAGES[k]:
                break
            vs.append(STAGES[k][r[2 + k]])
        else:
            by_key.setdefault(r[1], []).append(r + (None, None) + tuple(vs))
    at = [COLUMNS.index(c) for c in proj]
    out = []
    for o, s in sorted(zip(sl.o, sl.s)):
        for r in by_key.get(s, ()):
            full = r[:5] + (s, o) + r[7:]
            out.append(tuple(full[a] for a in at))
    return out


def as_rows(cols, n_rows, width):
    if width == 0 or n_rows == 0:
        return np.zeros((n_rows, width), np.uint32)
    return np.stack([np.asarray(c, np.uint32)[:n_rows] for c in cols], axis=1)


def _sorted_rows(m, lead=None):
    keys = [m[:, k] for k in reversed(range(m.shape[1]))] + ([lead] if lead is not None else [])
    return m[np.lexsort(tuple(keys))] if len(m) else m


def assert_multiset(got_cols, want, proj, what=""):
    """the same rows, in any order"""
    got, exp = as_rows(got_cols, len(got_cols[0]) if got_cols else 0, len(proj)), np.asarray(want, np.uint32).reshape(-1, len(proj))
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    np.testing.assert_array_equal(_sorted_rows(got), _sorted_rows(exp), err_msg=what)


def assert_slice_order(got_cols, want, proj, what=""):
    """The device's rows against reference(): with both slice columns in the projection, their sequence is the reference's exactly and,
    within the run of one slice row, the rows are the reference's as a sorted list (the chain of a key is built with atomic exchanges: its
    order is not stated).  Without both, the multiset is the reference's and the sort column ?o, if there, does not decrease."""
    assert_multiset(got_cols, want, proj, what)
    got, exp = as_rows(got_cols, len(got_cols[0]) if got_cols else 0, len(proj)), np.asarray(want, np.uint32).reshape(-1, len(proj))
    if "o" in proj:
        o = got[:, proj.index("o")].astype(np.int64)
        assert np.all(np.diff(o) >= 0), (what, "the sort column decreases")
    if "s" in proj and "o" in proj and len(exp):
        at = [proj.index("o"), proj.index("s")]
        np.testing.assert_array_equal(got[:, at], exp[:, at], err_msg=f"{what}: the slice's rows in its order")
        run = np.concatenate([[0], np.cumsum(np.any(exp[1:, at] != exp[:-1, at], axis=1))])
        np.testing.assert_array_equal(_sorted_rows(got, run), _sorted_rows(exp, run), err_msg=f"{what}: the rows of each slice row")


# ---------------------------------------------------------------------------------------------------
# what a table does to the tiles (for the CPU test's "the tables hold what they are for")
# ---------------------------------------------------------------------------------------------------
def chain_lengths(n, tab, n_stages=0):
    """slice row -> the number of table rows it emits"""
    per_row = {}
    for r in reference(n, tab, n_stages, ("s", "o")):
        per_row[r] = per_row.get(r, 0) + 1
    sl = slice_of(n)
    return [per_row.get((s, o), 0) for s, o in zip(sl.s, sl.o)]


def tile_totals(n, tab, n_stages=0):
    c = chain_lengths(n, tab, n_stages)
    return [sum(c[t:t + TILE]) for t in range(0, n, TILE)]


# ---------------------------------------------------------------------------------------------------
# the band join above the ordered slice join: a store of band geometry whose pF slice has exactly 2048 (or 2049) rows
# ---------------------------------------------------------------------------------------------------
B_FEATURES, B_GROUP, B_FEATURED, B_PRODUCTS, B_VALUES = 32, 64, 512, 1300, 40
B_PROD0 = bc.FEAT0 + B_FEATURES + 6
B_LIT0 = B_PROD0 + B_PRODUCTS
BAND_WINDOW = bc.Window("leq+6_geq-6", "LEQ", False, 6, "GEQ", True, 6)
BAND_WINDOW_2 = bc.Window("lt+9_gt-9_two", "LT", False, 9, "GT", True, 9, True)


def band_store(extra_row=False):
    """pF: 32 features of 64 products = 2048 rows in two tiles of the GPOS slice.  The first 256 products have their four features among the
    first 16 (slice rows 0 .. 1023), the next 256 among the last 16.  extra_row: one more product on the last feature (2049 rows).  pV and pV2
    give 1250 of the 1300 products an xsd:integer each (above 1024 rows: cached direct-address tables).  -> a band_cases.BandEdgeStore"""
    st = bc.BandEdgeStore()
    terms = [None] * B_LIT0 + [("integer", 3 * v - 20) for v in range(B_VALUES)]
    tv = np.zeros(len(terms), dtype=TV_DTYPE)
    tv["tag"][1:] = abi.TV_NAMED_NODE
    tv["lo"][1:] = np.arange(1, len(terms))
    tv["tag"][B_LIT0:] = abi.TV_INTEGER
    tv["lo"][B_LIT0:] = [t[1] for t in terms[B_LIT0:]]
    st.tv, st.decimals, st.terms = tv, np.zeros(0, np.int64), terms
    s, p, o = [], [], []
    for f in range(B_FEATURES):
        half = f // 16
        members = [256 * half + a for a in range(256) if (a + f) % 4 == 0]
        assert len(members) == B_GROUP
        for a in members:
            s.append(B_PROD0 + a); p.append(bc.PF); o.append(bc.FEAT0 + f)
    if extra_row:
        s.append(B_PROD0 + 256 + 255); p.append(bc.PF); o.append(bc.FEAT0 + B_FEATURES - 1)      # (255 + 31) % 4 != 0: not yet there
    st.n_build = len(s)
    for k, pv in enumerate((bc.PV, bc.PV2)):
        for a in range(B_PRODUCTS):
            if (a + k) % 26 != 7:
                s.append(B_PROD0 + a); p.append(pv); o.append(B_LIT0 + (7 * a + 3 * k) % B_VALUES)
    order = np.random.default_rng(5).permutation(len(s))
    u32 = lambda x: np.asarray(x, np.uint32)[order]
    st.quads = (np.zeros(len(s), np.uint32), u32(s), u32(p), u32(o))
    return st


def band_params(second_tile):
    """PARAMS(inst, X): 200 products of the first 256 (one of them twice: a chain of two table rows, so the ordered join below the band
    join has to count its matches), a product without a pV row, ids that are no product's; second_tile: 100 products of the next 256 too"""
    xs = [B_PROD0 + (3 * i) % 256 for i in range(200)] + [B_PROD0 + 9, B_PROD0 + 7, 0, B_PROD0 + B_FEATURED + 3, bc.FEAT0]
    if second_tile:
        xs += [B_PROD0 + 256 + (5 * i) % 256 for i in range(100)]
    return [np.arange(1, len(xs) + 1, dtype=np.uint32), np.asarray(xs, np.uint32)]


def band_over_ordered_plan(windows, neq):
    """band_cases.band_plan with its table computed in the plan: C(inst, X, f, ya, yb) = PARAMS JOIN (X pF f) JOIN (X pV ya) JOIN (X pV2 yb),
    the first of them an ordered slice join whose output the band join reads by f"""
    def constants(pb):
        scan = lambda p: pb.data_source(quad_pattern("s", p, "v"))
        c = pb.hash_join(pb.table(0, 2), scan(bc.PF), on=[(1, 0)], projection=[0, 1, 3])
        c = pb.hash_join(c, scan(bc.PV), on=[(1, 0)], projection=[0, 1, 2, 4])
        return pb.hash_join(c, scan(bc.PV2), on=[(1, 0)], projection=[0, 1, 2, 3, 5])
    return bc.band_plan(windows, neq, probe=constants)


def band_constants(st, params):
    """The table C(inst, X, f, ya, yb) of band_over_ordered_plan as five arrays, by dicts and loops: what window_reference takes as its probe table"""
    g, s, p, o = (c.tolist() for c in st.quads)
    feats, val = {}, ({}, {})
    for s_, p_, o_ in zip(s, p, o):
        if p_ == bc.PF:
            feats.setdefault(s_, []).append(o_)
        else:
            val[0 if p_ == bc.PV else 1][s_] = o_
    rows = [(inst, x, f, val[0][x], val[1][x]) for inst, x in zip(*[c.tolist() for c in params]) if x and x in val[0] and x in val[1] for f in feats.get(x, ())]
    return [np.asarray(c, np.uint32) for c in zip(*rows)]
