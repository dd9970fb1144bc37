"""The lexical casts (RDFGPU_EX_CAST_LEX / RDFGPU_EX_CAST_STRING) restated in Python, and the case tables their tests share.

The reference parses a simple literal with Rust's FromStr impls (lib/model/src/xsd: boolean.rs:108-115, i32 / i64::from_str,
decimal.rs:496-568, f32 / f64::from_str).  Here: a hand-written recogniser per grammar, exact conversion of a float / double through
fractions.Fraction (the two neighbouring values of the exact rational, half to even, overflow beyond MAX + ulp/2, subnormals exact),
and `declines`: Eisel-Lemire as include/rdfgpu.h specifies it (the first 19 significant digits; w and w + 1 must agree when digits
were dropped), over the table that rdf-fusion_amd/csrc/gen_lex_pow5.py generates — which rows may fail the execute instead of answering.

A result is (status, bits): status "ok" / "error"; bits = the payload as the typed value carries it (float: 32 bits, double: 64 bits,
integers and decimals: Python ints)."""
import importlib.util
import os
import struct
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_lex_pow5", os.path.join(ROOT, "rdf-fusion_amd", "csrc", "gen_lex_pow5.py"))
gen_lex_pow5 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen_lex_pow5)

TARGETS = ("boolean", "int", "integer", "decimal", "float", "double")
DIGITS = "0123456789"


# ---- recognisers ----------------------------------------------------------------------------------------------------------------
def parse_boolean(s):
    return {"true": ("ok", 1), "1": ("ok", 1), "false": ("ok", 0), "0": ("ok", 0)}.get(s, ("error", None))


def parse_integer(s, bits):
    i, neg = 0, False
    if s[:1] in ("+", "-"):
        neg, i = s[0] == "-", 1
    body = s[i:]
    if not body or any(c not in DIGITS for c in body):
        return ("error", None)
    v = -int(body) if neg else int(body)
    return ("ok", v) if -(1 << (bits - 1)) <= v < (1 << (bits - 1)) else ("error", None)


def parse_decimal(s):
    """Decimal::from_str: (\\+|-)?([0-9]+(\\.[0-9]*)?|\\.[0-9]+); value * 10^18 in a checked i128; fraction digits beyond the 18th must be
    trailing zeros; every intermediate (the digits read so far, as a signed integer) must fit i128 too."""
    i, neg = 0, False
    if s[:1] in ("+", "-"):
        neg, i = s[0] == "-", 1
    rest = s[i:]
    whole, dot, frac = rest.partition(".")
    if any(c not in DIGITS for c in whole + frac) or (not whole and not frac):
        return ("error", None)
    frac = frac.rstrip("0")
    if len(frac) > 18:
        return ("error", None)
    digits = int(whole + frac) if whole + frac else 0
    v = (-digits if neg else digits) * 10 ** (18 - len(frac))
    return ("ok", v) if -(1 << 127) <= v < (1 << 127) else ("error", None)


def scan_float(s):
    """Rust std's float grammar.  -> None (not a float), ("inf", neg), ("nan", signed), or ("num", neg, digits, exp10): the value is
    int(digits) * 10^exp10, digits with its leading zeros."""
    i, neg, signed = 0, False, False
    if s[:1] in ("+", "-"):
        neg, signed, i = s[0] == "-", True, 1
    rest = s[i:]
    low = "".join(chr(ord(c) + 32) if "A" <= c <= "Z" else c for c in rest)
    if low in ("inf", "infinity"):
        return ("inf", neg)
    if low == "nan":
        return ("nan", signed)
    k = 0
    while k < len(rest) and rest[k] in DIGITS:
        k += 1
    whole, frac = rest[:k], ""
    if k < len(rest) and rest[k] == ".":
        k += 1
        j = k
        while k < len(rest) and rest[k] in DIGITS:
            k += 1
        frac = rest[j:k]
    if not whole and not frac:
        return None
    exp = 0
    if k < len(rest):
        if rest[k] not in "eE":
            return None
        k += 1
        eneg = False
        if k < len(rest) and rest[k] in "+-":
            eneg, k = rest[k] == "-", k + 1
        if k >= len(rest) or any(c not in DIGITS for c in rest[k:]):
            return None
        exp = -int(rest[k:]) if eneg else int(rest[k:])
    return ("num", neg, whole + frac, exp - len(frac))


FORMATS = {"float": (24, -126, 127), "double": (53, -1022, 1023)}   # precision, least normal exponent, greatest exponent


def round_fraction(x, target):
    """The bits (without the sign) of the float / double nearest to the non-negative rational x, half to even."""
    p, emin, emax = FORMATS[target]
    if x == 0:
        return 0
    e = x.numerator.bit_length() - x.denominator.bit_length()       # floor(log2 x) is e or e - 1
    if Fraction(2) ** e > x:
        e -= 1
    e = max(e, emin)
    quantum = Fraction(2) ** (e - (p - 1))
    n, rem = divmod(x, quantum)
    n = int(n)
    if rem * 2 > quantum or (rem * 2 == quantum and n & 1):
        n += 1
    if n == 1 << p:
        n, e = n >> 1, e + 1
    if e > emax:
        return (2 * emax + 1) << (p - 1)                              # beyond MAX + ulp/2: infinity
    if n < 1 << (p - 1):
        return n                                                      # subnormal (or zero)
    return ((e + emax) << (p - 1)) | (n - (1 << (p - 1)))


def parse_float(s, target):
    """-> (status, bits).  A signed NaN: ("ok", None) — the sign Rust leaves is not restated (the device declines it)."""
    p, _, emax = FORMATS[target]
    width = 32 if target == "float" else 64
    sc = scan_float(s)
    if sc is None:
        return ("error", None)
    if sc[0] == "inf":
        return ("ok", ((2 * emax + 1) << (p - 1)) | (int(sc[1]) << (width - 1)))
    if sc[0] == "nan":
        return ("ok", None if sc[1] else ((2 * emax + 1) << (p - 1)) | (1 << (p - 2)))
    _, neg, digits, exp = sc
    m = int(digits)
    if m == 0:
        return ("ok", int(neg) << (width - 1))
    if exp > 400:                                                     # (saturates: keeps the rationals small)
        x = Fraction(10) ** 400
    elif exp < -1200 - len(digits):
        x = Fraction(1, 10 ** 1200)
    else:
        x = Fraction(m) * Fraction(10) ** exp
    return ("ok", round_fraction(x, target) | (int(neg) << (width - 1)))


def parse(s, target):
    if target == "boolean":
        return parse_boolean(s)
    if target == "int":
        return parse_integer(s, 32)
    if target == "integer":
        return parse_integer(s, 64)
    if target == "decimal":
        return parse_decimal(s)
    return parse_float(s, target)


# ---- Eisel-Lemire as specified: may the device decline? -----------------------------------------------------------------------------
EL = {"float": (23, -127, 0xFF, -65, 38, -17, 10, 10, 1 << 24), "double": (52, -1023, 0x7FF, -342, 308, -4, 23, 22, 1 << 53)}
M64 = (1 << 64) - 1


def eisel_lemire(w, q, target):
    """w * 10^q -> bits, or None where the algorithm cannot decide."""
    mant, min_exp, inf_power, q_min, q_max, even_min, even_max, _, _ = EL[target]
    if q < q_min:
        return 0
    if q > q_max:
        return inf_power << mant
    lz = 64 - w.bit_length()
    w <<= lz
    five = gen_lex_pow5.entry(q)
    mask = M64 >> (mant + 3)
    first = w * (five >> 64)
    hi, lo = first >> 64, first & M64
    if hi & mask == mask:
        second_hi = (w * (five & M64)) >> 64
        lo = (lo + second_hi) & M64
        if second_hi > lo:
            hi += 1
    if lo == M64 and not -27 <= q <= 55:
        return None
    upper = hi >> 63
    shift = upper + 64 - mant - 3
    m = hi >> shift
    p2 = ((q * (152170 + 65536)) >> 16) + 63 + upper - lz - min_exp
    if p2 <= 0:
        if -p2 + 1 >= 64:
            return 0
        m >>= -p2 + 1
        m += m & 1
        return m >> 1
    if lo <= 1 and even_min <= q <= even_max and m & 3 == 1 and (m << shift) == hi:
        m &= ~1
    m += m & 1
    m >>= 1
    if m >= 2 << mant:
        m, p2 = 1 << mant, p2 + 1
    m &= ~(1 << mant)
    if p2 >= inf_power:
        return inf_power << mant
    return (p2 << mant) | m


def cut(digits, exp):
    """The first 19 significant digits: (w, q, dropped)."""
    sig = digits.lstrip("0")
    if len(sig) <= 19:
        return int(sig or "0"), exp, False
    return int(sig[:19]), exp + len(sig) - 19, any(c != "0" for c in sig[19:])     # (cut zeros leave the value exactly w)


def declines(s, target):
    """True where the device, as specified, fails the execute instead of answering: a signed NaN; Eisel-Lemire undecided; a cut mantissa
    whose ends w and w + 1 round differently."""
    sc = scan_float(s)
    if sc is None or sc[0] == "inf":
        return False
    if sc[0] == "nan":
        return sc[1]
    w, q, dropped = cut(sc[2], sc[3])
    fast_q, fast_m = EL[target][7], EL[target][8]
    if w == 0 or (not dropped and w <= fast_m and -fast_q <= q <= fast_q):
        return False
    a = eisel_lemire(w, q, target)
    if a is None:
        return True
    return dropped and eisel_lemire(w + 1, q, target) != a


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


# ---- the case tables ---------------------------------------------------------------------------------------------------------------
# float double-rounding: strictly between the f32 half-way point 1 + 2^-24 and the nearest f64 to it — through f64 the half-way
# point itself is reached and rounds to even (down)
DOUBLE_ROUNDING = ["1.0000000596046448", "3.0000001192092896", "16777217.000000001"]
assert parse_float(DOUBLE_ROUNDING[0], "float") == ("ok", 0x3F800001)
for _s in DOUBLE_ROUNDING:   # the two routes must really differ, or the case is stale
    assert parse_float(_s, "float")[1] != f32_bits(struct.unpack("<d", struct.pack("<Q", parse_float(_s, "double")[1]))[0]), _s

MAX_F32 = "340282346638528859811704183484516925440"
MAX_F64 = "17976931348623157" + "0" * 292
HALF_MIN_F64 = "2.4703282292062327208051355972539e-324"               # digits of 2^-1075
FLOAT_RANGE = [
    MAX_F32, "3.4028235e38", "340282356779733661637539395458142568447", "340282356779733661637539395458142568448", "3.4028236e38",
    MAX_F64, "1.7976931348623157e308", "1.7976931348623158e308", "1.797693134862315807e308", "1.7976931348623159e308", "1e309",
    "1e-45", "1.401298464324817e-45", "7.006492321624085e-46", "7.0064923216240853e-46", "7.0064923216240854e-46", "7.1e-46", "7e-46",
    "5e-324", "4.9406564584124654e-324", "2.4703282292062327e-324", "2.4703282292062328e-324", "2.5e-324", "2.4e-324", "1e-400",
    "2.2250738585072014e-308", "2.2250738585072011e-308", "1.1754943508222875e-38", "1.1754942e-38",
    "-0", "-0.0e5", "0", "+0.0", "0e999", "-0e-999",
    "1234567890123456789", "12345678901234567890", "1.234567890123456789e5", "1.2345678901234567890e5",      # 19 and 20 digits agree
    "1.234567890123456789012345e10",                                                                            # 25 digits, w and w + 1 agree
    "9007199254740993", "9007199254740992.5", "9007199254740993.0000000001",                                    # half-way neighbourhood of 2^53
    "16777217", "16777216.5", "16777217.0", "0.1", "0.3", "1e23", "8.5e22", "123456.78", "99999999", "4.35", "1e22", "1e-22", "1e10", "1e-10", "1e11",
]
# more than 19 digits, and the two ends of the cut mantissa round differently: the device must refuse it
DECLINING = "9007199254740994.9999999999"            # (as a double; as a float both ends agree)
DECLINING_FLOAT = "16777217.00000000000001"            # w is the half-way point 2^24 + 1 itself, w + 1 lies above it (as a double: fine)
FLOAT_ACCEPTED = ["INF", "+INF", "-INF", "NaN", "Infinity", "-infinity", "inf", "nan", "iNfInItY", "1.", ".5", "+.5e-3", "1e5", "1E5", "1e+5", "1e-5", "1.e5", "007",
                  "1" + "0" * 399, "1e999999999999", "1e-999999999999", "-1e999999999999",
                  "1e3000000000", "1e-3000000000", "1e4294967296", "1e2147483650", "1e-2147483650", "1e536870912", "1e5368709119", "0.1e2147483647", "1e00000000000000000005",
                  "12345678901234567890000", "1.2345678901234567890000e3", "0.000000000000000000000000000001", "5", "-5.25", "+7.125"]
FLOAT_REFUSED = [".", "", "+", "-", "1e", "1e+", " 1", "1 ", "0x10", "1_0", "1f", "e5", ".e5", "1e5.0", "1..0", "--1", "+-1", "infinit", "in", "na", "nane", "infinityy",
                 "1e+-5", "١", "1,5", "NaN ", "1e 5", "inf\0", "nan\0\0", "\0inf", "infinity\0"]
FLOAT_SIGNED_NAN = ["-nan", "+nan", "-NaN"]
INTEGER_CASES = ["9223372036854775807", "9223372036854775808", "-9223372036854775808", "-9223372036854775809", "-0", "+7", "007", "", "-", "1.0",
                 "2147483647", "2147483648", "-2147483648", "-2147483649", "+", "1e3", " 1", "12a", "0", "99999999999999999999"]
I128_MAX = (1 << 127) - 1
DECIMAL_CASES = ["0." + "1" * 18, "0." + "1" * 19, "1.5" + "0" * 30, "0." + "1" * 18 + "000", ".", "5.", ".5", "-.5", "+5.25", "", "-", "1e3", "1.2.3", "12a",
                 str(I128_MAX)[:-18] + "." + str(I128_MAX)[-18:], str(I128_MAX + 1)[:-18] + "." + str(I128_MAX + 1)[-18:],
                 "-" + str(I128_MAX + 1)[:-18] + "." + str(I128_MAX + 1)[-18:], "-" + str(I128_MAX + 2)[:-18] + "." + str(I128_MAX + 2)[-18:],
                 "170141183460469231731", "170141183460469231732", "-170141183460469231731.687303715884105728", "0", "-0.0", "007.70"]
BOOLEAN_CASES = ["true", "1", "false", "0", "TRUE", "01", "", "True", "false ", "2"]

FLOAT_CASES = DOUBLE_ROUNDING + FLOAT_RANGE + [DECLINING, DECLINING_FLOAT] + FLOAT_ACCEPTED + FLOAT_REFUSED + FLOAT_SIGNED_NAN
CASES = {"boolean": BOOLEAN_CASES + ["1.0", "-0"], "int": INTEGER_CASES, "integer": INTEGER_CASES, "decimal": DECIMAL_CASES + ["1", "-7"],
         "float": FLOAT_CASES + INTEGER_CASES, "double": FLOAT_CASES + INTEGER_CASES + DECIMAL_CASES}
ALL_STRINGS = sorted({s for v in CASES.values() for s in v})

assert declines(DECLINING, "double") and not declines(DECLINING, "float") and declines(DECLINING_FLOAT, "float") and not declines(DECLINING_FLOAT, "double")
assert not declines("1.234567890123456789012345e10", "double") and not declines("1.2345678901234567890e5", "float")
assert all(parse_float(s, t)[0] == "ok" for s in FLOAT_ACCEPTED for t in ("float", "double"))
assert all(parse_float(s, t)[0] == "error" for s in FLOAT_REFUSED for t in ("float", "double"))
assert parse_float("340282356779733661637539395458142568448", "float")[1] == 0x7F800000 and parse_float("340282356779733661637539395458142568447", "float")[1] == 0x7F7FFFFF
assert parse_float("2.4703282292062328e-324", "double")[1] == 1 and parse_float("2.4703282292062327e-324", "double")[1] == 0
for _s in FLOAT_RANGE + FLOAT_ACCEPTED:   # Python's own correctly rounded conversion as the second opinion, f64 only
    _sc = scan_float(_s)
    if _sc and _sc[0] == "num":
        assert parse_float(_s, "double")[1] == f64_bits(float(_s)), _s


def expected(s, target):
    """(status, bits, may_decline) — what a row of the table must give: the bits, the error value, or (may_decline) the failed execute."""
    st, bits = parse(s, target)
    may = target in ("float", "double") and declines(s, target)
    return st, bits, may
