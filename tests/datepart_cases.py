"""Shared cases of the date parts (RDFGPU_EX_YEAR .. RDFGPU_EX_SECONDS) and a Python reference that shares nothing with the device code.

The reference is integer arithmetic from the XSD definition: a Timestamp is `value` = seconds on the time line * 10^18 (UTC when there is
a timezone) and an offset in minutes; the local parts are those of t = trunc(value / 10^18) + 60 * offset (the library truncates toward
zero before it takes the euclidean day and second-of-day: Decimal::as_i128, then div_euclid / rem_euclid — stated in include/rdfgpu.h),
the calendar date of day number floor(t / 86400) counted from 0001-01-01 in the proleptic Gregorian calendar with a year 0, and
SECONDS = value mod 60 on the scaled value.  `civil_from_days` is the era-based conversion (400-year eras that begin on 1 March), not the
library's year descent.  check_reference() ties it to `datetime` (years 1..9999) and to rdf_fusion_amd.xsd.time_on_timeline (round trip).
"""
import datetime
import json
import os
from fractions import Fraction

import numpy as np

from rdf_fusion_amd import abi, xsd

SCALE = 10 ** 18
I128_MIN, I128_MAX = -(1 << 127), (1 << 127) - 1
PARTS = ("year", "month", "day", "hours", "minutes", "seconds")
OPS = {"year": abi.EX_YEAR, "month": abi.EX_MONTH, "day": abi.EX_DAY, "hours": abi.EX_HOURS, "minutes": abi.EX_MINUTES, "seconds": abi.EX_SECONDS}


def civil_from_days(days):
    """(year, month, day) of day number `days`, day 0 = 0001-01-01; year 0 precedes year 1"""
    z = days + 306                              # days since 0000-03-01
    era, doe = divmod(z, 146097)
    yoe = (doe - doe // 1460 + doe // 36524 - doe // 146096) // 365
    doy = doe - (365 * yoe + yoe // 4 - yoe // 100)
    mp = (5 * doy + 2) // 153
    day = doy - (153 * mp + 2) // 5 + 1
    month = mp + 3 if mp < 10 else mp - 9
    return yoe + era * 400 + (1 if month <= 2 else 0), month, day


def trunc_div(a, b):
    q = abs(a) // b
    return -q if a < 0 else q


def parts(value, has_tz, tz_minutes):
    """{'year': .., .., 'seconds': scaled decimal} of Timestamp(value, offset)"""
    t = trunc_div(value, SCALE) + 60 * (tz_minutes if has_tz else 0)
    days, sod = divmod(t, 86400)
    y, m, d = civil_from_days(days)
    return {"year": y, "month": m, "day": d, "hours": sod // 3600, "minutes": sod % 3600 // 60, "seconds": value % (60 * SCALE)}


def check_reference():
    """the reference against `datetime` for years 1..9999 (every 13th day, and every day around each century), and by round trip through
    xsd.time_on_timeline for years on both sides of 1, offsets and fractions"""
    last = datetime.date.max.toordinal()
    probe = set(range(1, last + 1, 13)) | {last}
    for y in range(100, 10000, 100):
        o = datetime.date(y, 3, 1).toordinal()
        probe |= set(range(o - 3, o + 2))
    for o in probe:
        dt = datetime.date.fromordinal(o)
        assert civil_from_days(o - 1) == (dt.year, dt.month, dt.day), o
    rng = np.random.default_rng(7)
    for _ in range(4000):
        y = int(rng.integers(-12000, 12000)); mo = int(rng.integers(1, 13)); d = int(rng.integers(1, xsd.days_in_month(y, mo) + 1))
        h, mi = int(rng.integers(0, 24)), int(rng.integers(0, 60))
        s = Fraction(int(rng.integers(0, 60 * 1000)), 1000)
        tz = None if rng.integers(0, 3) == 0 else int(rng.integers(-840, 841))
        v = xsd.time_on_timeline(y, mo, d, h, mi, s, tz) * SCALE
        assert v.denominator == 1
        p = parts(int(v), tz is not None, tz or 0)
        if int(v) >= 0 or s.denominator == 1:      # (a negative value with a fraction truncates toward zero first: the cases below)
            assert (p["year"], p["month"], p["day"], p["hours"], p["minutes"]) == (y, mo, d, h, mi), (y, mo, d, h, mi, s, tz, p)
        assert p["seconds"] == s * SCALE


def _offset(lexical):
    """the timezone offset a lexical form ends in, in minutes (none, or Z: 0)"""
    if len(lexical) > 6 and lexical[-6] in "+-" and lexical[-3] == ":":
        sign = -1 if lexical[-6] == "-" else 1
        return sign * (int(lexical[-5:-3]) * 60 + int(lexical[-2:]))
    return 0


def _dt(lexical):
    v, has = xsd.parse_date_time(lexical)
    return (lexical, v, has, _offset(lexical))


# (name, value * 10^18, has a timezone, offset in minutes)
CASES = [
    _dt("0001-01-01T00:00:00Z"),
    ("the second before 0001-01-01", -SCALE, True, 0),
    _dt("0000-12-31T23:59:59Z"), _dt("0000-02-29T00:00:00Z"), _dt("-0001-12-31T23:59:59Z"), _dt("-0001-03-01T00:00:00"),
    _dt("-0002-06-06T00:00:00"), _dt("-0400-02-29T12:30:30Z"), _dt("-0401-12-31T23:59:59Z"), _dt("-9999-01-01T00:00:00Z"),
    _dt("1900-02-28T23:59:59Z"), _dt("1900-03-01T00:00:00Z"), _dt("2000-02-29T12:00:00Z"), _dt("2000-03-01T00:00:00Z"),
    _dt("2100-02-28T23:59:59Z"), _dt("2100-03-01T00:00:00Z"), _dt("2024-02-29T23:59:59Z"), _dt("2023-02-28T23:59:59Z"),
    _dt("1999-12-31T23:59:59.999999999999999999Z"), _dt("1999-12-31T23:59:59.999999999999999999"), _dt("1999-12-31T24:00:00"),
    _dt("9999-12-31T23:59:59.999999999999999999Z"), _dt("10000-01-01T00:00:00Z"),
    # offsets that move the day, the month and the year across a boundary (the stored value is the UTC instant)
    _dt("2024-01-01T05:00:00+14:00"), _dt("2023-12-31T20:00:00-14:00"), _dt("2024-03-01T02:00:00+05:30"), _dt("2024-02-29T22:00:00-05:30"),
    _dt("2023-03-01T00:29:00+05:30"), _dt("0001-01-01T00:00:00+14:00"), _dt("0001-01-01T00:00:00-14:00"), _dt("1999-05-31T13:20:00-05:00"),
    _dt("1999-05-31T13:30:00+05:30"), _dt("2023-12-31T23:59:59-00:01"),
    # no timezone: the parts of the value as it stands
    _dt("2024-07-15T10:20:30"), _dt("2024-07-15T10:29:59.5"), _dt("1970-01-01T00:00:00"),
    # fractions, and negative values with a fraction: the whole seconds truncate TOWARD ZERO before the euclidean split
    ("+0.5 s", SCALE // 2, True, 0), ("-0.5 s", -(SCALE // 2), True, 0), ("-0.5 s, no timezone", -(SCALE // 2), False, 0),
    ("-1 s - 1e-18", -SCALE - 1, True, 0), ("-60 s - 1e-18", -60 * SCALE - 1, True, 0), ("-86400 s - 0.25", -86400 * SCALE - SCALE // 4, True, 0),
    ("-86399.75 s", -86400 * SCALE + SCALE // 4, True, 0), ("-0.5 s at +00:01", -(SCALE // 2), True, 1), ("-0.5 s at -00:01", -(SCALE // 2), True, -1),
    ("-1e-18", -1, True, 0), ("+1e-18", 1, False, 0),
    # the ends of the i128 range: 68-bit second counts, day counts beyond 2^50
    ("i128 max", I128_MAX, True, 840), ("i128 min", I128_MIN, True, -840), ("i128 max, no timezone", I128_MAX, False, 0), ("i128 min + 1", I128_MIN + 1, False, 0),
    ("2^64 s", (1 << 64) * SCALE, True, 0), ("-2^64 s", -(1 << 64) * SCALE, True, 0),
]

# a value of every kind that is not a dateTime: tag -> (lo, aux, scaled i128 or None).  Each must give the error value under all six ops.
NOT_DATE_TIME = {
    abi.TV_NULL: (0, 0, None), abi.TV_NAMED_NODE: (3, 0, None), abi.TV_BLANK_NODE: (4, 0, None), abi.TV_STRING: (5, 0, None),
    abi.TV_BOOLEAN: (1, 0, None), abi.TV_FLOAT: (0x40490FDB, 0, None), abi.TV_DOUBLE: (0x400921FB54442D18, 0, None),
    abi.TV_DECIMAL: (0, 0, 63_000_000_000 * SCALE), abi.TV_INT: (2024, 0, None), abi.TV_INTEGER: (63_000_000_000, 0, None),
    abi.TV_TIME: (0, 1, xsd.parse_time("13:20:10.5Z")[0]), abi.TV_DATE: (0, 1, xsd.parse_date("1999-05-31Z")[0]),
    abi.TV_DURATION: (7, 0, None), abi.TV_OTHER: (8, 9, None),
}


def fuzz_timestamps(n, seed):
    """n seeded (value, has_tz, tz): calendar years 1..9999, the neighbourhood of 0, the whole i128 range, at second and sub-second grain"""
    rng = np.random.default_rng(seed)
    out = []
    span = 9999 * 366 * 86400
    for i in range(n):
        k = i % 4
        if k == 0:
            v = int(rng.integers(0, span)) * SCALE + int(rng.integers(0, SCALE))
        elif k == 1:
            v = int(rng.integers(-span, span)) * SCALE + (int(rng.integers(-SCALE + 1, SCALE)) if rng.integers(0, 2) else 0)
        elif k == 2:
            v = int(rng.integers(-200000, 200000)) * SCALE // int(rng.integers(1, 1000))
        else:
            v = int.from_bytes(rng.bytes(16), "little", signed=True)
        has = bool(rng.integers(0, 4))
        out.append((v, has, int(rng.integers(-840, 841)) if has else 0))
    return out


def split_i128(v):
    """(lo, hi) as signed 64-bit integers"""
    u = v & ((1 << 128) - 1)
    s = lambda x: x - (1 << 64) if x >= (1 << 63) else x
    return s(u & ((1 << 64) - 1)), s(u >> 64)


def golden():
    """the known answers of the reference's own unit tests (date_time.rs `year` .. `second`), tests/golden/datepart_kats.json"""
    with open(os.path.join(os.path.dirname(__file__), "golden", "datepart_kats.json")) as f:
        return json.load(f)["cases"]


def golden_timestamp(case):
    """(value, has_tz, tz) of a golden case: its lexical form parsed by rdf_fusion_amd.xsd"""
    lex, kind = case["lexical"], case["type"]
    v, has = {"dateTime": xsd.parse_date_time, "date": xsd.parse_date, "time": xsd.parse_time}[kind](lex)
    return v, has, _offset(lex)
