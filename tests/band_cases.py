"""Integer-window joins at the edges of their biased intervals: the stores, probe tables, windows and the exact expected rows shared
by test_band_window_cpu.py (oracle = reference, on a machine without a GPU) and test_gpu_band_edges.py (every device form = reference).

The plan is the band join's:  T(inst, X, f, ya, yb) JOIN (product pF f) ON f [product != X]
                              JOIN (product pV v1) ON product [window(v1; ya, yb)] [JOIN (product pV2 v2) ON product [window(v2; ya, yb)]]
with output (inst, product, v1[, v2]).  A window is  cmp0(x, y0 +/- lit0) AND cmp1(x, y1 +/- lit1).

Geometry: the band path wants build rows >= 4 x key range, probe rows x 4 >= key range and groups of at most 512 rows; a base join's
build side of more than 1024 rows (below that the join table lives in LDS and there is no CSR table to walk group by group), and stage
slices of more than 1024 rows each (below that a stage has no cached direct-address table and the chain never fuses).  Hence 1200
products - not fewer - over 24 features, about 1500 slice rows and 1450 probe rows."""
from collections import namedtuple
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

from rdf_fusion_amd import abi
from rdf_fusion_amd.engine import TV_DTYPE
from rdf_fusion_amd.plan import (PlanBuilder, quad_pattern, col, integer, decimal, ENC_TV, GT, LT, GEQ, LEQ, ADD, SUB, EBV, ID_NEQ, AND)

I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
PF, PV, PV2 = 1, 2, 3
FEAT0, N_FEAT, N_PROD = 10, 24, 1200
PROD0 = FEAT0 + N_FEAT + 6
LIT0 = PROD0 + N_PROD
GROUP_SIZES = (512, 129, 128, 65, 64, 63, 1, 0)           # the first eight features; the others draw 8 .. 56 rows
PROBE_ROWS = (65, 129, 64, 63, 65, 64, 129, 63)           # probe rows of those keys; the others cycle through PROBE_CYCLE
PROBE_CYCLE = (0, 1, 63, 64, 65, 129)

# ---------------------------------------------------------------------------------------------------
# values: the slice side, one case on each side of every limit of the biased forms
# ---------------------------------------------------------------------------------------------------
SPREADS = {"one": (0,), "pack_max": (0, 1, 65529, 65530), "pack_over": (0, 65531), "wide": (0, 2 ** 31, 2 ** 32 - 33),
           "band_over": (0, 2 ** 32 - 32), "index_max": (0, 2 ** 32 - 17), "index_over": (0, 2 ** 32 - 16)}
BASES = {"min": lambda spread: I64_MIN + 1, "neg": lambda spread: -2 ** 62, "zero": lambda spread: -3, "max": lambda spread: I64_MAX - spread}
Y_OFFSETS = (-5, 0, 1, 65530, 65535, 2 ** 32 - 33, 2 ** 32)
Y_FIXED = (0, I64_MAX, -I64_MAX, I64_MIN)

ValueSet = namedtuple("ValueSet", "name values y_values spread has_min")


def value_sets():
    out = []
    for sname, spread in SPREADS.items():
        for bname, base_of in BASES.items():
            base = base_of(max(spread))
            ys = sorted({y for y in [base + d for d in Y_OFFSETS] + list(Y_FIXED) if I64_MIN <= y <= I64_MAX})
            out.append(ValueSet(f"{sname}-{bname}", tuple(base + d for d in spread), tuple(ys), max(spread), False))
    ys = sorted({y for y in list(Y_OFFSETS) + list(Y_FIXED) + [I64_MAX - 65530, I64_MIN + 65531]})
    out.append(ValueSet("extremes", (I64_MIN + 1, 0, I64_MAX), tuple(ys), 2 ** 64 - 2, False))
    out.append(ValueSet("i64_min", (I64_MIN, I64_MIN + 1, I64_MIN + 65530), tuple(sorted({I64_MIN + d for d in Y_OFFSETS if d >= 0} | set(Y_FIXED))), 65530, True))
    return out


VALUE_SETS = value_sets()
BAND_SPREAD_LIMIT, PACK_SPREAD_MAX, INDEX_SPREAD_LIMIT = 0xFFFFFFE0, 65530, 0xFFFFFFF0   # chain_band_args refuses at, packs up to, chain_range_index refuses at

# ---------------------------------------------------------------------------------------------------
# windows
# ---------------------------------------------------------------------------------------------------
# op / sub / lit of each half; lit = an int (xsd:integer) or a Fraction (xsd:decimal); two: the halves read ya and yb instead of ya twice
Window = namedtuple("Window", "name op0 sub0 lit0 op1 sub1 lit1 two empty", defaults=(False, False))
_OPS = {"LT": LT, "LEQ": LEQ, "GT": GT, "GEQ": GEQ}
WINDOWS = [
    Window("lt+1_gt-1", "LT", False, 1, "GT", True, 1),
    Window("leq+0_geq-0", "LEQ", False, 0, "GEQ", True, 0),
    Window("leq+65530_gt-65530", "LEQ", False, 65530, "GT", True, 65530),
    Window("geq-65531_lt+65531_two", "GEQ", True, 65531, "LT", False, 65531, True),
    Window("leq+2^32_geq-2^32", "LEQ", False, 2 ** 32, "GEQ", True, 2 ** 32),
    Window("lt+max_gt-max", "LT", False, I64_MAX, "GT", True, I64_MAX),
    Window("gt+neg65530_lt-neg65530", "GT", False, -65530, "LT", True, -65530),
    Window("geq+neg1_leq-neg1_two", "GEQ", False, -1, "LEQ", True, -1, True),
    Window("lt-min_geq+0", "LT", True, I64_MIN, "GEQ", False, 0),
    Window("lt+65531_geq-1", "LT", False, 65531, "GEQ", True, 1),
    Window("leq+0_gt-2^32_two", "LEQ", False, 0, "GT", True, 2 ** 32, True),
    Window("lt+65530_leq+1", "LT", False, 65530, "LEQ", False, 1),
    Window("gt-1_geq-65531", "GT", True, 1, "GEQ", True, 65531),
    Window("lt+300.5_gt-300.5", "LT", False, Fraction(601, 2), "GT", True, Fraction(601, 2)),
    Window("lt-3_gt+3_empty", "LT", True, 3, "GT", False, 3, False, True),
    Window("gt-max_leq+65531_two", "GT", True, I64_MAX, "LEQ", False, 65531, True),
]
ZERO_WINDOW = WINDOWS[1]          # literal 0: no operand overflows, every all-integer row is decided by the biased interval

Case = namedtuple("Case", "value_set windows neq")


def cases_of(k):
    """The (windows, ID_NEQ) combinations value set k runs: six of the sixteen windows (every window meets about eleven value sets), two of them
    followed by a second window stage, ID_NEQ on the base join in every other one."""
    out = []
    for j in range(6):
        ws = [WINDOWS[(k + 5 * j) % len(WINDOWS)]]
        if j in (1, 4):
            ws.append(WINDOWS[(k + 5 * j + 7) % len(WINDOWS)])
        out.append(Case(VALUE_SETS[k], tuple(ws), (j + k) % 2 == 0))
    return out


def case_id(c):
    return "+".join(w.name for w in c.windows) + ("_neq" if c.neq else "")


# ---------------------------------------------------------------------------------------------------
# store and probe table
# ---------------------------------------------------------------------------------------------------
@dataclass
class BandEdgeStore:
    quads: tuple = None            # (g, s, p, o)
    tv: np.ndarray = None          # typed values, index = object id
    decimals: np.ndarray = None    # their i128 side table
    terms: list = None             # what the reference knows of an id: None (no number) or (kind, value)
    value_ids: list = None         # ids of the slice values, of the probe rows' integer operands, of the operands of other kinds
    y_ids: list = None
    zoo_ids: list = None
    T: list = None                 # the probe table (inst, X, f, ya, yb)
    T_int: list = None             # the same rows with every operand an xsd:integer (null keys and null X stay)
    n_build: int = 0               # rows of the pF slice (after deduplication)


def band_edge_store(rng, values, y_values, big_group=False):
    """values: the xsd:integer literals of pV / pV2; y_values: the xsd:integer operands of the probe rows.  big_group: one more feature
    whose group has 513 rows (one past what the band path takes)."""
    st = BandEdgeStore()
    n_feat = N_FEAT + (1 if big_group else 0)
    assert n_feat <= PROD0 - FEAT0 - 1
    # the dictionary: slice values, probe operands, other kinds
    terms = [None] * LIT0
    def add(kind, v):
        terms.append((kind, v)); return len(terms) - 1
    st.value_ids = [add("integer", v) for v in values]
    st.y_ids = [add("integer", y) for y in y_values]
    mid = values[len(values) // 2]
    st.zoo_ids = [add("double", float(mid)), add("double", float("nan")), add("decimal", Fraction(25, 2)), add("int", 7), add("double", 0.5)]
    terms.append(None); st.zoo_ids.append(len(terms) - 1)                     # an IRI
    tv = np.zeros(len(terms), dtype=TV_DTYPE)
    tv["tag"][1:] = abi.TV_NAMED_NODE
    tv["lo"][1:] = np.arange(1, len(terms))
    dec = []
    for i, t in enumerate(terms):
        if t is None:
            continue
        kind, v = t
        if kind == "integer":
            tv["tag"][i] = abi.TV_INTEGER; tv["lo"][i] = v
        elif kind == "int":
            tv["tag"][i] = abi.TV_INT; tv["lo"][i] = v
        elif kind == "double":
            tv["tag"][i] = abi.TV_DOUBLE; tv["lo"][i] = np.float64(v).view(np.int64)
        else:
            raw = int(v * 10 ** 18) & ((1 << 128) - 1)
            tv["tag"][i] = abi.TV_DECIMAL; tv["lo"][i] = len(dec) // 2
            dec += [raw & ((1 << 64) - 1), raw >> 64]
    st.tv, st.decimals, st.terms = tv, np.array(dec, dtype=np.uint64).astype(np.int64), terms
    # quads
    prod = np.arange(PROD0, PROD0 + N_PROD, dtype=np.uint32)
    sizes = list(GROUP_SIZES) + [int(x) for x in rng.integers(8, 57, N_FEAT - len(GROUP_SIZES))] + ([513] if big_group else [])
    S, P, O = [], [], []
    def emit(s, p, o):
        S.append(np.asarray(s, np.uint32)); P.append(np.full(len(s), p, np.uint32)); O.append(np.asarray(o, np.uint32))
    groups = [rng.choice(prod, size, replace=False) for size in sizes]
    for f, members in enumerate(groups):
        emit(members, PF, np.full(len(members), FEAT0 + f))
    for pv in (PV, PV2):
        keep = rng.random(N_PROD) >= 0.04                                      # products without the value: no stage row
        emit(prod[keep], pv, rng.choice(st.value_ids, int(keep.sum())))
    emit(groups[1][:40], PF, np.full(40, FEAT0 + 1))                           # duplicates: the store keeps one of each
    s, p, o = np.concatenate(S), np.concatenate(P), np.concatenate(O)
    order = rng.permutation(len(s))
    st.quads = (np.zeros(len(s), np.uint32), s[order], p[order], o[order])
    # probe rows
    rows_per_key = list(PROBE_ROWS) + [PROBE_CYCLE[i % len(PROBE_CYCLE)] for i in range(N_FEAT - len(PROBE_ROWS))] + ([2] if big_group else [])
    f = np.concatenate([np.full(r, FEAT0 + k, np.uint32) for k, r in enumerate(rows_per_key)] +
                       [np.full(10, FEAT0 - 1, np.uint32), np.full(10, FEAT0 + n_feat, np.uint32), np.zeros(20, np.uint32)])   # strangers and null keys
    f = f[rng.permutation(len(f))]
    n = len(f)
    X = (PROD0 + rng.integers(0, N_PROD, n)).astype(np.uint32)
    X[rng.random(n) < 0.03] = 0                                                # unbound: `product != X` is not true
    def operand(odd):
        y = rng.choice(st.y_ids, n).astype(np.uint32)
        if odd:
            sel = rng.random(n) < 0.06
            y[sel] = rng.choice(st.zoo_ids, int(sel.sum()))
            y[rng.random(n) < 0.01] = 0
        return y
    inst = np.arange(1, n + 1, dtype=np.uint32)
    st.T = [inst, X, f, operand(True), operand(True)]
    st.T_int = [inst, X, f, operand(False), operand(False)]
    st.n_build = len(set(zip(s[p == PF].tolist(), o[p == PF].tolist())))
    return st


def store_of(vs, big_group=False):
    """The store of a value set: the same one (seeded by the set's position) wherever it is asked for."""
    k = [v.name for v in VALUE_SETS].index(vs.name)
    return band_edge_store(np.random.default_rng(1000 + k + (500 if big_group else 0)), vs.values, vs.y_values, big_group)


# ---------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------
def window_expr(w, x, ya, yb):
    def half(op, sub, lit, y):
        l = decimal(int(lit * 10 ** 18)) if isinstance(lit, Fraction) else integer(lit)
        return EBV(_OPS[op](ENC_TV(col(x)), (SUB if sub else ADD)(ENC_TV(col(y)), l)))
    return AND(half(w.op0, w.sub0, w.lit0, ya), half(w.op1, w.sub1, w.lit1, yb if w.two else ya))


def band_plan(windows, neq, probe=None):
    """probe: builds the node that computes T(inst, X, f, ya, yb) in the plan (ordered_cases.py); None: T is the table bound at slot 0"""
    pb = PlanBuilder()
    t = probe(pb) if probe else pb.table(0, 5)
    scan = lambda p, v: pb.data_source(quad_pattern("product", p, v))
    node = pb.hash_join(t, scan(PF, "f"), on=[(2, 1)], filter=ID_NEQ(col(5), col(1)) if neq else None, projection=[0, 5, 3, 4])   # (inst, product, ya, yb)
    if len(windows) == 1:
        node = pb.hash_join(node, scan(PV, "v1"), on=[(1, 0)], filter=window_expr(windows[0], 5, 2, 3), projection=[0, 1, 5])
    else:
        node = pb.hash_join(node, scan(PV, "v1"), on=[(1, 0)], filter=window_expr(windows[0], 5, 2, 3), projection=[0, 1, 2, 3, 5])
        node = pb.hash_join(node, scan(PV2, "v2"), on=[(1, 0)], filter=window_expr(windows[1], 6, 2, 3), projection=[0, 1, 4, 6])
    return pb.build(node)


# ---------------------------------------------------------------------------------------------------
# the reference: Python ints (Fractions, floats) straight from the SPARQL rule
# ---------------------------------------------------------------------------------------------------
_RANK = {"int": 0, "integer": 1, "decimal": 2, "double": 3}
DEC_MAX = 2 ** 127                                          # xsd:decimal here: an i128 of 10^-18 units


def _promote(a, b):
    return max(a[0], b[0], key=_RANK.get)


def _as(kind, t):
    return float(t[1]) if kind == "double" else Fraction(t[1]) if kind == "decimal" else int(t[1])


def _arith(a, b, sub):
    """a +/- b by the operator mapping: both promoted to the wider kind; an integer result outside its type is an error (None)"""
    if a is None or b is None:
        return None
    kind = _promote(a, b)
    x, y = _as(kind, a), _as(kind, b)
    z = x - y if sub else x + y
    if kind == "integer" and not I64_MIN <= z <= I64_MAX:
        return None
    if kind == "int" and not -2 ** 31 <= z < 2 ** 31:
        return None
    if kind == "decimal" and not -DEC_MAX <= z * 10 ** 18 < DEC_MAX:
        return None
    return (kind, z)


def _holds(op, a, b):
    """a op b is true (an error, a NaN or an incomparable pair is not)"""
    if a is None or b is None:
        return False
    kind = _promote(a, b)
    x, y = _as(kind, a), _as(kind, b)
    if x != x or y != y:
        return False
    return {"LT": x < y, "LEQ": x <= y, "GT": x > y, "GEQ": x >= y}[op]


def window_holds(w, x, ya, yb):
    lit = lambda l: ("decimal", l) if isinstance(l, Fraction) else ("integer", l)
    return (_holds(w.op0, x, _arith(ya, lit(w.lit0), w.sub0)) and
            _holds(w.op1, x, _arith(yb if w.two else ya, lit(w.lit1), w.sub1)))


def base_pairs(quads, T, neq):
    """(probe row, product) of the base join on f, as index arrays; quads deduplicated first (the store does)."""
    q = np.unique(np.stack(quads, axis=1), axis=0)
    pf = q[q[:, 2] == PF]
    by_feature = {}
    for s, o in zip(pf[:, 1].tolist(), pf[:, 3].tolist()):
        by_feature.setdefault(o, []).append(s)
    rows, prods = [], []
    for r, (x, f) in enumerate(zip(T[1].tolist(), T[2].tolist())):
        if f == 0:
            continue
        for s in by_feature.get(f, ()):
            if neq and (x == 0 or s == x):
                continue
            rows.append(r); prods.append(s)
    value_of = []
    for pv in (PV, PV2):
        sel = q[q[:, 2] == pv]
        assert len(set(sel[:, 1].tolist())) == len(sel), "one value per product"
        value_of.append(dict(zip(sel[:, 1].tolist(), sel[:, 3].tolist())))
    return np.array(rows, np.int64), np.array(prods, np.uint32), value_of


def window_reference(quads, terms, T, windows, neq):
    """The expected rows (inst, product, v1[, v2]) as a sorted (n, k) array, and the number of rows of the join without its windows
    (every product with all its stage rows): what a window that passes everything would give."""
    rows, prods, value_of = base_pairs(quads, T, neq)
    term = lambda i: terms[i] if 0 < i < len(terms) else None
    keep = np.ones(len(rows), bool)
    out = [T[0][rows], prods]
    for w, vals in zip(windows, value_of):
        lut = np.zeros(len(terms), np.uint32)
        lut[list(vals)] = list(vals.values())
        v = lut[prods]
        keep &= v != 0
        ya, yb = T[3][rows], T[4][rows]
        assert len(terms) < 1 << 21
        keys, inverse = np.unique((v.astype(np.int64) << 42) | (ya.astype(np.int64) << 21) | yb, return_inverse=True)   # the rule once per distinct (x, ya, yb)
        ids = [(k >> 42, (k >> 21) & 0x1FFFFF, k & 0x1FFFFF) for k in keys.tolist()]
        verdict = np.array([x != 0 and window_holds(w, term(x), term(a), term(b)) for x, a, b in ids], bool)
        ok = verdict[inverse.reshape(-1)] if len(keys) else np.zeros(0, bool)
        out.append(v)
        windowed = ok if len(out) == 3 else windowed & ok
    unfiltered = int(keep.sum())
    sel = keep & windowed
    m = np.stack([np.asarray(c, np.uint32)[sel] for c in out], axis=1)
    order = np.lexsort(tuple(m[:, k] for k in reversed(range(m.shape[1]))))
    return m[order], unfiltered
