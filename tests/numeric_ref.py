"""A restatement of the numeric expression ops (MUL, DIV, NEG, PLUS, ABS, ROUND, CEIL, FLOOR, CAST) over (tag, payload) values, from
reading the reference: lib/functions/src/scalar/numeric/*.rs, scalar/conversion/cast_*.rs and lib/model/src/xsd/{decimal,int,integer,
boolean,numeric}.rs.  The payload is a Python int for TV_INT / TV_INTEGER / TV_BOOLEAN, the scaled i128 (value * 10^18) for
TV_DECIMAL, a numpy float32 / float64 scalar for TV_FLOAT / TV_DOUBLE, None otherwise.  ERR is the SPARQL error value.  The GPU tests
(test_gpu_numeric.py) take their expected values from here; test_numeric_cpu.py checks it against the reference's own known answers."""
import numpy as np

from rdf_fusion_amd import abi

INT, INTEGER, DEC, FLT, DBL, BOOL, STR = abi.TV_INT, abi.TV_INTEGER, abi.TV_DECIMAL, abi.TV_FLOAT, abi.TV_DOUBLE, abi.TV_BOOLEAN, abi.TV_STRING
ERR = (abi.TV_NULL, None)
E18 = 10 ** 18
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I128_MIN, I128_MAX = -(1 << 127), (1 << 127) - 1
NUMERIC = (INT, INTEGER, DEC, FLT, DBL)
RANK = {INT: 0, INTEGER: 1, DEC: 2, FLT: 3, DBL: 4}      # NumericPair::with_casts_from, numeric.rs:127-201


class CastFromString(Exception):
    """A numeric cast met a simple literal: the device refuses the execute (RDFGPU_ERR_UNSUPPORTED)."""


def trunc_div(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def fits128(v):
    return I128_MIN <= v <= I128_MAX


def dec_to_f64(v):
    """From<Decimal> for Double, decimal.rs:445-462"""
    mag, shift = abs(v), E18
    while mag and shift != 1 and mag % 10 == 0:
        mag //= 10
        shift //= 10
    d = np.float64(mag) / np.float64(shift)
    return -d if v < 0 else d


def to_f64(tag, v):
    return np.float64(v) if tag in (INT, INTEGER, FLT, DBL) else dec_to_f64(v)


def to_f32(tag, v):
    return np.float32(v) if tag in (INT, INTEGER, FLT, DBL) else np.float32(dec_to_f64(v))


def to_dec(tag, v):
    return v if tag == DEC else v * E18


def dec_mul(left, right):
    """Decimal::checked_mul, decimal.rs:93-125; None = error"""
    sl = sr = 0
    if left != 0:
        while left % 10 == 0:
            left = trunc_div(left, 10)
            sl += 1
    if right != 0:
        while right % 10 == 0:
            right = trunc_div(right, 10)
            sr += 1
    shift = sl + sr - 18
    if shift < 0 or not fits128(left * right) or not fits128(10 ** shift):
        return None
    p = left * right * 10 ** shift
    return p if fits128(p) else None


def dec_div(left, right):
    """Decimal::checked_div, decimal.rs:131-163"""
    sl = sr = 0
    if left != 0:
        while fits128(left * 10):
            left *= 10
            sl += 1
    if right != 0:
        while right % 10 == 0:
            right = trunc_div(right, 10)
            sr += 1
    shift = sl + sr - 18
    if shift < 0 or right == 0 or not fits128(10 ** shift):
        return None
    q = trunc_div(left, right)
    if not fits128(q):
        return None
    return trunc_div(q, 10 ** shift)


def dec_round(v):
    """decimal.rs:211-222"""
    value = trunc_div(v, E18 // 10)
    if value >= 0:
        r = value // 10 + (value % 10 >= 5)
    else:
        r = trunc_div(value, 10) - ((-value) % 10 > 5)
    r *= E18
    return r if fits128(r) else None


def dec_ceil(v):
    """decimal.rs:228-238"""
    r = (trunc_div(v, E18) + 1 if v > 0 and abs(v) % E18 != 0 else trunc_div(v, E18)) * E18
    return r if fits128(r) else None


def dec_floor(v):
    """decimal.rs:244-254"""
    r = (trunc_div(v, E18) if v >= 0 or abs(v) % E18 == 0 else trunc_div(v, E18) - 1) * E18
    return r if fits128(r) else None


def dec_from_f64(x):
    """TryFrom<Double> for Decimal, decimal.rs:420-435: in [-2^127, 2^127], then a truncating, saturating `as i128`"""
    with np.errstate(all="ignore"):
        shifted = np.float64(x) * np.float64(1e18)
    if not (-(2.0 ** 127) <= shifted <= 2.0 ** 127):
        return None
    return min(max(int(shifted), I128_MIN), I128_MAX)


def round_half_away(x):
    """Rust's f32 / f64 `round`; keeps the sign of a zero result"""
    t = np.trunc(x)
    with np.errstate(all="ignore"):
        r = t + np.copysign(type(x)(1), x) if abs(x - t) >= 0.5 else t
    return np.copysign(r, x)


def _dec(v):
    return ERR if v is None else (DEC, v)


def binary(op, a, b):
    """MUL / DIV, mul.rs:50-76, div.rs:51-80"""
    (ta, va), (tb, vb) = a, b
    if ta not in NUMERIC or tb not in NUMERIC:
        return ERR
    k = ta if RANK[ta] >= RANK[tb] else tb
    div = op == abi.EX_DIV
    with np.errstate(all="ignore"):
        if k == DBL:
            x, y = to_f64(ta, va), to_f64(tb, vb)
            return DBL, np.float64(x / y if div else x * y)
        if k == FLT:
            x, y = to_f32(ta, va), to_f32(tb, vb)
            return FLT, np.float32(x / y if div else x * y)
    if k == DEC or div:
        return _dec((dec_div if div else dec_mul)(to_dec(ta, va), to_dec(tb, vb)))
    p = va * vb
    lo, hi = (I32_MIN, I32_MAX) if k == INT else (I64_MIN, I64_MAX)
    return (k, p) if lo <= p <= hi else ERR


def unary(op, a):
    """NEG / PLUS / ABS (numeric.rs:20-38), ROUND / CEIL / FLOOR (round.rs:48-60, ceil.rs, floor.rs)"""
    t, v = a
    if t not in NUMERIC:
        return ERR
    if op == abi.EX_PLUS:
        return a
    if op in (abi.EX_NEG, abi.EX_ABS):
        if t in (FLT, DBL):
            return t, (-v if op == abi.EX_NEG else np.abs(v))
        r = -v if op == abi.EX_NEG else abs(v)
        lo, hi = {INT: (I32_MIN, I32_MAX), INTEGER: (I64_MIN, I64_MAX), DEC: (I128_MIN, I128_MAX)}[t]
        return (t, r) if lo <= r <= hi else ERR
    if t in (INT, INTEGER):
        return a
    if t in (FLT, DBL):
        return t, {abi.EX_ROUND: round_half_away, abi.EX_CEIL: np.ceil, abi.EX_FLOOR: np.floor}[op](v)
    return _dec({abi.EX_ROUND: dec_round, abi.EX_CEIL: dec_ceil, abi.EX_FLOOR: dec_floor}[op](v))


def cast(target, a, aux=0):
    """cast_{boolean,int,integer,decimal,float,double}.rs:48-62; `aux` = the language id of a string operand"""
    t, v = a
    if t == STR and aux == 0:
        raise CastFromString()
    if t == BOOL:
        t, v = INTEGER, int(v != 0)
    if t not in NUMERIC:
        return ERR
    if target == BOOL:
        if t in (FLT, DBL):
            return BOOL, int(v != 0 and not np.isnan(v))
        return BOOL, int(v != 0)
    if target == FLT:
        return FLT, to_f32(t, v)
    if target == DBL:
        return DBL, to_f64(t, v)
    d = dec_from_f64(to_f64(t, v)) if t in (FLT, DBL) else to_dec(t, v)
    if d is None:
        return ERR
    if target == DEC:
        return DEC, d
    q = trunc_div(d, E18)
    lo, hi = (I32_MIN, I32_MAX) if target == INT else (I64_MIN, I64_MAX)
    return (target, q) if lo <= q <= hi else ERR


def bits(value):
    """(tag, lo, hi) as the device writes the value (rdfgpu_agg_value / a typed literal); every NaN is one NaN"""
    t, v = value
    if t == abi.TV_NULL:
        return (t, 0, 0)
    if t == FLT:
        return (t, "nan", 0) if np.isnan(v) else (t, int(np.float32(v).view(np.uint32)), 0)
    if t == DBL:
        return (t, "nan", 0) if np.isnan(v) else (t, int(np.float64(v).view(np.int64)), 0)
    if t == DEC:
        u = v & ((1 << 128) - 1)
        s64 = lambda x: x - (1 << 64) if x >= 1 << 63 else x
        return (t, s64(u & ((1 << 64) - 1)), s64(u >> 64))
    return (t, int(v), 0)


def device_bits(tag, lo, hi):
    """A device value (tag, lo, hi) in the same form"""
    if tag == FLT and np.isnan(np.uint32(lo & 0xFFFFFFFF).view(np.float32)):
        return (tag, "nan", 0)
    if tag == DBL and np.isnan(np.int64(lo).view(np.float64)):
        return (tag, "nan", 0)
    if tag == abi.TV_NULL:
        return (tag, 0, 0)
    return (tag, int(lo) & 0xFFFFFFFF if tag == FLT else int(lo), int(hi) if tag == DEC else 0)
