"""MIN / MAX of AggregateExec (abi.AGG_MIN / AGG_MAX, plans with abi.PLAN_AGG_COLUMNS): the typed-value table, the reference's accumulator
restated over a row order, the device's rule (include/rdfgpu.h), the hand-written cases, the row layouts and the BI Q5 / Q6 shaped plans,
shared by test_minmax_cpu.py (the rule is an answer of the reference, on a machine without a GPU) and test_gpu_minmax.py (the device =
the rule).

A value is (tag, payload) as in agg_cases.py: an int for xsd:int / xsd:integer, the raw i128 (value x 10^18) for xsd:decimal, a Python
float for xsd:float (a binary32 value) / xsd:double.  ERR is the error value (an unbound id).  Two results are compared as the device's
(tag, lo, hi) records, bit for bit, so -0 and +0 differ; only an all-NaN group's payload is left open."""
import itertools
import math
import struct
from collections import namedtuple
from functools import lru_cache

import numpy as np

from rdf_fusion_amd import abi
from rdf_fusion_amd.engine import TV_DTYPE
from rdf_fusion_amd.plan import PlanBuilder, col, decimal, EBV, EQ, GT, MUL, ENC_TV
import agg_cases as ac

E18 = ac.E18
MIN, MAX, COUNT, AVG, SUM, STAR = abi.AGG_MIN, abi.AGG_MAX, abi.AGG_COUNT, abi.AGG_AVG, abi.AGG_SUM, abi.AGG_COUNT_STAR
INT, INTEGER, DEC, FLOAT, DOUBLE = abi.TV_INT, abi.TV_INTEGER, abi.TV_DECIMAL, abi.TV_FLOAT, abi.TV_DOUBLE
KINDS = (INT, INTEGER, DEC, FLOAT, DOUBLE)            # the order in which an unbeaten candidate is preferred
ERR = (abi.TV_NULL, None)
UNSUPPORTED = "unsupported"                           # rule 3: the execute fails
MINMAX_WORDS = 7                                      # kAggMinMaxWords (kernels.hpp)
RT_MINMAX_KIND = 128                                  # kRtMinMaxKind (expr_device.hpp)
HI5 = 5 << 64                                         # decimals that share the high word 5

# ---------------------------------------------------------------------------------------------------
# the typed-value table: agg_cases' ids unchanged, then what MIN / MAX need
# ---------------------------------------------------------------------------------------------------
EXTRA = [
    ("fNaN", FLOAT, math.nan), ("gNaN", DOUBLE, math.nan),
    ("f+0", FLOAT, 0.0), ("f-0", FLOAT, -0.0), ("g+0", DOUBLE, 0.0), ("g-0", DOUBLE, -0.0),
    ("f+inf", FLOAT, math.inf), ("f-inf", FLOAT, -math.inf), ("g+inf", DOUBLE, math.inf), ("g-inf", DOUBLE, -math.inf),
    ("i2^24+1", INTEGER, 2 ** 24 + 1), ("f2^24", FLOAT, 2.0 ** 24), ("i2^24", INTEGER, 2 ** 24),      # equal as f32, different exactly
    ("i2^53+1", INTEGER, 2 ** 53 + 1), ("g2^53", DOUBLE, 2.0 ** 53),
    ("dHI+0", DEC, HI5), ("dHI+1", DEC, HI5 + 1), ("dHI+2", DEC, HI5 + 2), ("dHI+top", DEC, HI5 + 2 ** 64 - 1),   # one high word
    ("d-HI-1", DEC, -(HI5 + 1)),                                                                       # dHI+1 with the other sign
    ("int7", INT, 7),                                                                                  # and id 7 is the xsd:integer 7
    ("f1.5", FLOAT, 1.5), ("g2.5", DOUBLE, 2.5), ("g-3.5", DOUBLE, -3.5),
    ("bool", abi.TV_BOOLEAN, 1),
]


def typed_table():
    """agg_cases.typed_table() over its NAMED followed by EXTRA"""
    saved = ac.NAMED
    ac.NAMED = saved + EXTRA
    try:
        return ac.typed_table()
    finally:
        ac.NAMED = saved


TV, DECIMALS, IDS, VALUES = typed_table()
IDS["i7"] = 7
assert TV.dtype == TV_DTYPE and all(IDS[k] == v for k, v in ac.IDS.items())


def val(i):
    return VALUES[i] if 0 < i < len(VALUES) else ERR


def _s64(u):
    u &= (1 << 64) - 1
    return u - (1 << 64) if u >> 63 else u


def record(v):
    """a value as the device's rdfgpu_agg_value: (tag, lo, hi) with signed 64-bit words"""
    tag, p = v
    if tag == abi.TV_NULL:
        return 0, 0, 0
    if tag == DEC:
        raw = p & ((1 << 128) - 1)
        return tag, _s64(raw), _s64(raw >> 64)
    if tag == FLOAT:
        return tag, struct.unpack("<I", struct.pack("<f", p))[0], 0
    if tag == DOUBLE:
        return tag, _s64(struct.unpack("<Q", struct.pack("<d", p))[0]), 0
    return tag, int(p), 0


def is_nan(v):
    return v[0] in (FLOAT, DOUBLE) and math.isnan(v[1])


def same_result(a, b):
    """two results are the same record; an all-NaN result: the tag and NaN-ness only"""
    if a == UNSUPPORTED or b == UNSUPPORTED:
        return a == b
    if is_nan(a) or is_nan(b):
        return is_nan(a) and is_nan(b) and a[0] == b[0]
    return record(a) == record(b)


# ---------------------------------------------------------------------------------------------------
# Numeric::partial_cmp, numeric.rs:90-190
# ---------------------------------------------------------------------------------------------------
def _dec_to_f64(raw):
    """From<Decimal> for Double, decimal.rs:445-462: trailing zeros stripped from value and scale, one division"""
    neg, mag, shift = raw < 0, abs(raw), E18
    while mag != 0 and shift != 1 and mag % 10 == 0:
        mag //= 10
        shift //= 10
    d = float(mag) / float(shift)                     # int -> float rounds to nearest even, like `as f64`
    return -d if neg else d


def to_f64(v):
    tag, p = v
    return float(p) if tag in (INT, INTEGER) else _dec_to_f64(p) if tag == DEC else float(p)


def to_f32(v):
    tag, p = v
    if tag in (INT, INTEGER):
        return np.asarray(p, np.int64).astype(np.float32)[()]        # i64 as f32: one rounding
    if tag == DEC:
        return np.float32(_dec_to_f64(p))                            # decimal.rs:437-443: through f64
    return np.float32(p)


def to_dec(v):
    return v[1] if v[0] == DEC else v[1] * E18


def partial_cmp(a, b):
    """-1 / 0 / 1, None = no order (a NaN).  NumericPair::with_casts_from: double if either is, else float, else decimal, else integer"""
    return _cmp_cached(a[0], _key(a), b[0], _key(b))


def _key(v):
    return record(v)[1:]


@lru_cache(maxsize=None)
def _cmp_cached(ta, ka, tb, kb):
    a, b = _unrecord(ta, ka), _unrecord(tb, kb)
    tags = {ta, tb}
    if DOUBLE in tags:
        x, y = to_f64(a), to_f64(b)
    elif FLOAT in tags:
        x, y = to_f32(a), to_f32(b)
    elif DEC in tags:
        x, y = to_dec(a), to_dec(b)
    else:
        x, y = a[1], b[1]
    return -1 if x < y else 1 if x > y else 0 if x == y else None


def _unrecord(tag, k):
    lo, hi = k
    if tag == DEC:
        raw = ((hi & ((1 << 64) - 1)) << 64) | (lo & ((1 << 64) - 1))
        return tag, raw - (1 << 128) if raw >> 127 else raw
    if tag == FLOAT:
        return tag, struct.unpack("<f", struct.pack("<I", lo))[0]
    if tag == DOUBLE:
        return tag, struct.unpack("<d", struct.pack("<q", lo))[0]
    return tag, lo


# ---------------------------------------------------------------------------------------------------
# the reference's accumulator (min.rs:42-53, max.rs:43-54) over one row order, and the device's rule
# ---------------------------------------------------------------------------------------------------
def reference_accumulator(values, fn):
    executed_once, cur = False, ERR                   # min: ThinError::expected()
    for value in values:
        if not executed_once:                         # if !self.executed_once { self.min = value; self.executed_once = true }
            cur, executed_once = value, True
        elif cur != ERR:                              # else if let Ok(min) = self.min
            if value != ERR:                          #   if let Ok(value) = value
                if fn == MIN:
                    if partial_cmp(value, cur) == -1:     # if value < min
                        cur = value
                elif partial_cmp(cur, value) == -1:       # if max < value
                    cur = value
    return cur


def device_rule(values, fn):
    """rules 1 to 4 of include/rdfgpu.h"""
    if any(v[0] not in KINDS and v != ERR for v in values):
        return UNSUPPORTED                            # 3: a bound value that is not numeric
    if not values or ERR in values:
        return ERR                                    # 1, 2
    cands = []
    for kind in KINDS:                                # 4: one candidate per kind, its exact extremum among the values that are not NaN
        mine = [v for v in values if v[0] == kind]
        if not mine:
            continue
        real = [v for v in mine if not is_nan(v)]
        if not real:
            cands.append((kind, math.nan))
        elif kind in (FLOAT, DOUBLE):                 # IEEE order, the bit pattern deciding between the zeros: -0 below +0
            key = lambda v: (v[1], math.copysign(1.0, v[1]))
            cands.append(min(real, key=key) if fn == MIN else max(real, key=key))
        else:
            cands.append(min(real, key=lambda v: v[1]) if fn == MIN else max(real, key=lambda v: v[1]))
    real = [c for c in cands if not is_nan(c)]
    if not real:
        return cands[0]                               # every candidate a NaN: the lowest kind's
    beats = -1 if fn == MIN else 1
    for c in real:                                    # (in the order of KINDS)
        if not any(partial_cmp(o, c) == beats for o in real if o is not c):
            return c
    raise AssertionError("no unbeaten candidate")


def reference_answers(values, fn):
    """the accumulator's answers over every order of the rows"""
    out = []
    for p in set(itertools.permutations(range(len(values)))):
        r = reference_accumulator([values[i] for i in p], fn)
        if not any(same_result(r, o) for o in out):
            out.append(r)
    return out


# ---------------------------------------------------------------------------------------------------
# the hand-written cases: the expected MIN and MAX worked by hand
# ---------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name ids min max")
NAN_F, NAN_G = (FLOAT, math.nan), (DOUBLE, math.nan)


def _cases():
    n, C = IDS, Case
    v = lambda name: val(n[name])
    return [
        C("integers", [n["i3"], n["i5"], n["i1"]], (INTEGER, 1), (INTEGER, 5)),
        # i64 keys 0 and 2^64 - 1: MAX of the smallest integer is key 0, MIN of the largest is the complemented key 0
        C("integer-key-0-max", [n["iMIN"]], v("iMIN"), v("iMIN")),
        C("integer-key-0-min", [n["iMAX"]], v("iMAX"), v("iMAX")),
        C("integer-ends", [n["i0"], n["iMAX"], n["iMIN"], n["i-1"]], v("iMIN"), v("iMAX")),
        C("xsd-int", [n["int-1"], n["int2^31-1"], n["int-2^31"]], v("int-2^31"), v("int2^31-1")),
        # int 7 and integer 7 are equal: neither candidate is beaten, int is the lower kind
        C("int-and-integer-equal", [n["i7"], n["int7"]], (INT, 7), (INT, 7)),
        # int -1 < integer 0: MIN is the int; MAX is the integer
        C("int-below-integer", [n["int-1"], n["i0"]], (INT, -1), (INTEGER, 0)),
        # f32(2^24 + 1) = 2^24 (a tie, to even): the integer candidates 2^24 (MIN) and 2^24 + 1 (MAX) equal the float 2^24 after the
        # cast, nothing is beaten, integer is the lower kind
        C("f32-cast-ties", [n["i2^24+1"], n["f2^24"], n["i2^24"]], (INTEGER, 2 ** 24), (INTEGER, 2 ** 24 + 1)),
        # f64(2^53 + 1) = 2^53: equal to the double, integer is the lower kind
        C("f64-cast-ties", [n["i2^53+1"], n["g2^53"]], (INTEGER, 2 ** 53 + 1), (INTEGER, 2 ** 53 + 1)),
        # one high word, four low words
        C("decimal-low-word", [n["dHI+1"], n["dHI+top"], n["dHI+0"], n["dHI+2"]], (DEC, HI5), (DEC, HI5 + 2 ** 64 - 1)),
        C("decimal-sign", [n["dHI+1"], n["d-HI-1"]], (DEC, -(HI5 + 1)), (DEC, HI5 + 1)),
        C("decimal-ends", [n["d0"], n["dMAX"], n["dMIN"]], v("dMIN"), v("dMAX")),
        C("decimal-key-0-max", [n["dMIN"]], v("dMIN"), v("dMIN")),
        C("decimal-key-0-min", [n["dMAX"]], v("dMAX"), v("dMAX")),
        # high words -1 (d-1 = -10^-18), 0 (2^64 - 1: every low bit set) and 5
        C("decimal-high-words", [n["d2^64-1"], n["dHI+0"], n["d-1"]], (DEC, -1), (DEC, HI5)),
        # decimal 1.0 = integer 1: nothing is beaten, integer is the lower kind
        C("decimal-equals-integer", [n["dE18"], n["i1"]], (INTEGER, 1), (INTEGER, 1)),
        # -1.0 < 1 < 3: MIN is the decimal, MAX the integer
        C("decimal-and-integers", [n["i3"], n["d-E18"], n["i1"]], (DEC, -E18), (INTEGER, 3)),
        C("float-zeros", [n["f+0"], n["f-0"], n["f+0"]], (FLOAT, -0.0), (FLOAT, 0.0)),
        C("double-zeros", [n["g-0"], n["g+0"]], (DOUBLE, -0.0), (DOUBLE, 0.0)),
        # float -0 and double +0 are equal as doubles: nothing is beaten, float is the lower kind, for MIN and for MAX
        C("zeros-across-kinds", [n["g+0"], n["f-0"]], (FLOAT, -0.0), (FLOAT, -0.0)),
        C("infinities", [n["f+inf"], n["i5"], n["g-inf"]], (DOUBLE, -math.inf), (FLOAT, math.inf)),
        C("float-infinities", [n["f-inf"], n["f0.75"], n["f+inf"]], (FLOAT, -math.inf), (FLOAT, math.inf)),
        # NaNs are left out while another value is there
        C("nan-among-values", [n["fNaN"], n["i3"], n["gNaN"], n["i5"]], (INTEGER, 3), (INTEGER, 5)),
        C("nan-and-its-kind", [n["fNaN"], n["f1.5"], n["f0.75"]], (FLOAT, 0.75), (FLOAT, 1.5)),
        C("float-nan-double-value", [n["fNaN"], n["g0.5"]], (DOUBLE, 0.5), (DOUBLE, 0.5)),
        # every value a NaN: the lowest kind's
        C("all-nan", [n["gNaN"], n["fNaN"]], NAN_F, NAN_F),
        C("all-nan-double", [n["gNaN"], n["gNaN"]], NAN_G, NAN_G),
        # int -1 is below everything; 0.75 (float) is above 0.5 (double), 0, -10^-18 and -1
        C("five-kinds", [n["g0.5"], n["i0"], n["f0.75"], n["d-1"], n["int-1"]], (INT, -1), (FLOAT, 0.75)),
        # -3.5 (double) < -1 ...; 2.5 (double) > 1.5 (float) > 1
        C("doubles-win", [n["g2.5"], n["i1"], n["f1.5"], n["g-3.5"], n["i-1"]], (DOUBLE, -3.5), (DOUBLE, 2.5)),
        # rule 2
        C("unbound-among-integers", [n["i3"], 0, n["i5"]], ERR, ERR),
        C("unbound-alone", [0], ERR, ERR),
        C("unbound-last", [n["f0.75"], n["dE18"], 0], ERR, ERR),
        # rule 3
        C("string-among-integers", [n["i3"], n["str"], n["i5"]], UNSUPPORTED, UNSUPPORTED),
        C("boolean-among-integers", [n["bool"], n["i5"]], UNSUPPORTED, UNSUPPORTED),
        C("string-and-unbound", [0, n["str"]], UNSUPPORTED, UNSUPPORTED),
    ]


CASES = _cases()
ANSWERED = [c for c in CASES if c.min != UNSUPPORTED]
REFUSED = [c for c in CASES if c.min == UNSUPPORTED]
# what the seeded groups of test_minmax_cpu.py draw from: every numeric id of the table, NaNs and the unbound id included
NUMERIC_IDS = [0] + [i for i in list(range(1, 12)) + list(range(ac.N_SMALL + 1, len(VALUES))) if val(i)[0] in KINDS]


def seeded_groups(n=2000, seed=17):
    rng = np.random.default_rng(seed)
    return [[int(x) for x in rng.choice(NUMERIC_IDS, int(rng.integers(1, 6)))] for _ in range(n)]


# ---------------------------------------------------------------------------------------------------
# row layouts and plans over bound tables
# ---------------------------------------------------------------------------------------------------
FILLER_GROUPS = 37


def case_table(cases, order="sorted", seed=5):
    """(group, value): one group per case (group id = 10 + its index) among FILLER_GROUPS filler groups of small integers (ids 2000 + j)"""
    key = [10 + g for g, c in enumerate(cases) for _ in c.ids]
    value = [i for c in cases for i in c.ids]
    rng = np.random.default_rng(seed)
    for j in range(FILLER_GROUPS):
        k = int(rng.integers(1, 9))
        key += [2000 + j] * k
        value += rng.integers(1, 1001, k).tolist()
    key, value = np.asarray(key, np.uint32), np.asarray(value, np.uint32)
    if order == "shuffled":
        perm = rng.permutation(len(key))
        key, value = key[perm], value[perm]
    return [key, value]


def expected(cols, keys, aggs, value=val):
    """{key tuple: [device_rule per (fn, column) of aggs]} over host columns"""
    kc = [np.asarray(cols[k]).tolist() for k in keys]
    groups = {}
    for r in range(len(cols[0])):
        groups.setdefault(tuple(c[r] for c in kc), []).append(r)
    return {k: [device_rule([value(int(cols[c][r])) for r in rows], fn) for fn, c in aggs] for k, rows in groups.items()}


def aggregate_plan(n_cols, keys, aggs):
    pb = PlanBuilder()
    return pb.build(pb.aggregate(pb.table(0, n_cols), keys, aggs), agg_columns=True)


def q5_plan(pb, t):
    """BI Q5's shape over (country, product, review): COUNT(review) per (country, product); MAX of it per country; the join back with
    `?nrOfReviews = ?maxReviews`; ORDER BY the count descending, then country and product.  -> (country, product, count)"""
    counts = pb.aggregate(t, [0, 1], [(COUNT, 2)])                     # country, product, count
    best = pb.aggregate(counts, [0], [(MAX, 2)])                       # country, max
    joined = pb.hash_join(counts, best, [(0, 0)], filter=EBV(EQ(ENC_TV(col(2)), ENC_TV(col(4)))), projection=[0, 1, 2])
    return pb.sparql_order_by(joined, [(2, True), (0, False), (1, False)])


def q6_plan(pb, t):
    """BI Q6's shape over (reviewer, score): the global AVG(score); cross join; AVG(score) and MIN(global average) per reviewer; HAVING
    `avg > min * 1.5`.  -> (reviewer, avg, min)"""
    overall = pb.aggregate(t, [], [(AVG, 1)])                          # avg
    both = pb.cross_join(t, overall)                                   # reviewer, score, avg
    per = pb.aggregate(both, [0], [(AVG, 1), (MIN, 2)])                # reviewer, avg, min
    return pb.sparql_having(per, EBV(GT(ENC_TV(col(1)), MUL(ENC_TV(col(2)), decimal(15 * E18 // 10)))))
