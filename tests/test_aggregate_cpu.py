"""AggregateExec (GROUP BY with COUNT / COUNT DISTINCT / SUM / AVG) on the host side: the ABI constants, the plan builder's output
schema and display, and this file's own restatement of the reference's accumulators (lib/functions/src/aggregates/sum.rs:34-73,
avg.rs:43-134, lib/model/src/xsd/decimal.rs:131-162), checked against vectors worked by hand from reading them.  The GPU tests
(test_gpu_aggregate.py) take their expected values from this restatement.  No GPU needed."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from rdf_fusion_amd import abi
from rdf_fusion_amd.engine import agg_value
from rdf_fusion_amd.plan import PlanBuilder, explain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E18 = 10 ** 18
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I128_MIN, I128_MAX = -(1 << 127), (1 << 127) - 1


# ---------------------------------------------------------------------------------------------------
# the restatement: a value is (tag, payload) — int for TV_INT / TV_INTEGER, the i128 (value * 10^18) for TV_DECIMAL, a Python float
# for TV_FLOAT (already an f32 value) / TV_DOUBLE, anything for the other tags (not numeric)
# ---------------------------------------------------------------------------------------------------
NUMERIC = (abi.TV_INT, abi.TV_INTEGER, abi.TV_DECIMAL, abi.TV_FLOAT, abi.TV_DOUBLE)


def _trunc_div(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def dec_to_f64(v):
    """From<Decimal> for Double (decimal.rs:445-462): trailing zeros of the scaled value stripped, then one division."""
    mag, shift = abs(v), E18
    while mag and shift != 1 and mag % 10 == 0:
        mag //= 10
        shift //= 10
    d = float(mag) / float(shift)
    return -d if v < 0 else d


def f32(x):
    return float(np.float32(x))


def to_f64(tag, v):
    if tag in (abi.TV_INT, abi.TV_INTEGER):
        return float(v)
    return dec_to_f64(v) if tag == abi.TV_DECIMAL else float(v)


def to_f32(tag, v):
    if tag in (abi.TV_INT, abi.TV_INTEGER):
        return f32(v)
    return f32(dec_to_f64(v)) if tag == abi.TV_DECIMAL else f32(v)


def decimal_checked_div(left, right):
    """Decimal::checked_div on the scaled i128 values (decimal.rs:131-162); None = the error value."""
    shift_left = 0
    if left != 0:
        while I128_MIN <= left * 10 <= I128_MAX:
            left *= 10
            shift_left += 1
    shift_right = 0
    if right != 0:
        while right % 10 == 0:
            right = _trunc_div(right, 10)
            shift_right += 1
    shift = shift_left + shift_right - 18
    if shift < 0 or right == 0 or 10 ** shift > I128_MAX:
        return None
    return _trunc_div(_trunc_div(left, right), 10 ** shift)


class Approx:
    """A float / double result: the reference adds the cast values in row order; the device's order differs.  `terms` are the values as
    the reference casts them, `divisor` the AVG count (1 for SUM)."""

    def __init__(self, tag, terms, divisor=1):
        self.tag, self.terms, self.divisor = tag, list(terms), divisor

    def exact(self):
        t = self.terms
        if any(math.isnan(x) for x in t) or (math.inf in t and -math.inf in t):
            return math.nan
        if math.inf in t or -math.inf in t:
            return math.inf if math.inf in t else -math.inf
        return math.fsum(t)

    def check(self, got):
        """|got - exact| <= n * eps * sum|x| + eta (include/rdfgpu.h), on the sum; an AVG's division is one more correctly rounded step."""
        eps = 2.0 ** -24 if self.tag == abi.TV_FLOAT else 2.0 ** -53
        ex = self.exact()
        if math.isnan(ex):
            return math.isnan(got)
        if math.isinf(ex):
            return got == ex
        bound = len(self.terms) * eps * math.fsum(abs(x) for x in self.terms)
        top = 3.4028234663852886e38 if self.tag == abi.TV_FLOAT else 1.7976931348623157e308
        s = got * self.divisor if self.divisor != 1 else got
        if math.isinf(got):   # the rounded total left the format's range
            return abs(ex) + bound >= top and (got > 0) == (ex > 0)
        tiny = 2.0 ** -149 if self.tag == abi.TV_FLOAT else 2.0 ** -1074   # spacing of the subnormals: the absolute floor of a rounding
        slack = abs(s) * eps * 2 + self.divisor * tiny * 2 if self.divisor != 1 else tiny
        return abs(s - ex) <= bound + slack


def sum_agg(values):
    """SUM (sum.rs:34-73): starts as integer 0; not numeric / unbound values are skipped; the widest kind wins; overflow of the TOTAL
    (integer: i64, decimal: i128 x 10^-18) is the error value.  Returns (tag, payload) or (tag, Approx)."""
    nums = [(t, v) for t, v in values if t in NUMERIC]
    tags = {t for t, _ in nums}
    if abi.TV_DOUBLE in tags:
        return abi.TV_DOUBLE, Approx(abi.TV_DOUBLE, [to_f64(t, v) for t, v in nums])
    if abi.TV_FLOAT in tags:
        return abi.TV_FLOAT, Approx(abi.TV_FLOAT, [to_f32(t, v) for t, v in nums])
    if abi.TV_DECIMAL in tags:
        d = sum(v if t == abi.TV_DECIMAL else v * E18 for t, v in nums)
        return (abi.TV_DECIMAL, d) if I128_MIN <= d <= I128_MAX else (abi.TV_NULL, None)
    s = sum(v for _, v in nums)
    return (abi.TV_INTEGER, s) if I64_MIN <= s <= I64_MAX else (abi.TV_NULL, None)


def avg_agg(values):
    """AVG (avg.rs:43-134): starts as DECIMAL 0; every row counts; one not numeric / unbound value makes it the error value; count 0 =>
    integer 0; decimal results through Decimal::checked_div."""
    n = len(values)
    if n == 0:
        return abi.TV_INTEGER, 0
    if any(t not in NUMERIC for t, _ in values):
        return abi.TV_NULL, None
    tags = {t for t, _ in values}
    if abi.TV_DOUBLE in tags:
        return abi.TV_DOUBLE, Approx(abi.TV_DOUBLE, [to_f64(t, v) for t, v in values], n)
    if abi.TV_FLOAT in tags:
        return abi.TV_FLOAT, Approx(abi.TV_FLOAT, [to_f32(t, v) for t, v in values], n)
    d = sum(v if t == abi.TV_DECIMAL else v * E18 for t, v in values)
    if not I128_MIN <= d <= I128_MAX:
        return abi.TV_NULL, None
    q = decimal_checked_div(d, n * E18)
    return (abi.TV_DECIMAL, q) if q is not None else (abi.TV_NULL, None)


def count_agg(ids):
    return abi.TV_INTEGER, sum(1 for i in ids if i != 0)


def count_distinct_agg(ids):
    return abi.TV_INTEGER, len({i for i in ids if i != 0})


def same(expected, got):
    """expected (tag, payload | Approx) against a device value (tag, lo, hi)."""
    tag, payload = expected
    gtag, lo, hi = got
    if gtag != tag:
        return False
    if tag == abi.TV_NULL:
        return True
    if tag == abi.TV_INTEGER:
        return agg_value(gtag, lo, hi) == payload
    if tag == abi.TV_DECIMAL:
        return agg_value(gtag, lo, hi) == Fraction(payload, E18)
    return payload.check(agg_value(gtag, lo, hi))


# ---------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rdfgpu.h")).read(), flags=re.S)


def test_header_aggregate_constants_match_abi_py():
    h = _header()
    assert int(re.search(r"#define RDFGPU_ABI_VERSION (\d+)u", h).group(1)) == abi.ABI_VERSION == 4
    assert int(re.search(r"RDFGPU_NODE_AGGREGATE = (\d+)", h).group(1)) == abi.NODE_AGGREGATE == 11
    assert int(re.search(r"#define RDFGPU_MAX_AGGREGATES (\d+)u", h).group(1)) == abi.MAX_AGGREGATES == 8
    for name in ("COUNT_STAR", "COUNT", "COUNT_DISTINCT", "SUM", "AVG", "MIN", "MAX", "SAMPLE", "GROUP_CONCAT", "SUM_DISTINCT",
                 "AVG_DISTINCT", "COUNT_DISTINCT_STAR"):
        assert int(re.search(rf"RDFGPU_AGG_{name} = (\d+)", h).group(1)) == getattr(abi, "AGG_" + name), name
    opts = re.findall(r"RDFGPU_OPT_(\w+)", h[h.index("RDFGPU_OPT_FORCE_GENERIC_VM = 0"):h.index("RDFGPU_OPT__COUNT")])
    assert opts == abi.OPTION_NAMES and opts[-1] == "NO_AGG_LDS"


def test_agg_value_struct_and_symbols():
    assert abi.C.sizeof(abi.AggValue) == 24
    for f in ("rdfgpu_plan_agg_count", "rdfgpu_plan_agg_fetch", "rdfgpu_plan_agg_device"):
        assert f in abi.EXPORTED_SYMBOLS and f + "(" in _header()
    assert agg_value(abi.TV_INTEGER, -5) == -5
    assert agg_value(abi.TV_DECIMAL, 15 * E18 // 10) == Fraction(3, 2)
    assert agg_value(abi.TV_DECIMAL, -1, -1) == Fraction(-1, E18)
    assert agg_value(abi.TV_DOUBLE, int(np.array([2.5]).view(np.int64)[0])) == 2.5
    assert agg_value(abi.TV_FLOAT, int(np.array([1.5], np.float32).view(np.uint32)[0])) == 1.5
    assert agg_value(abi.TV_NULL, 7) is None


# ---------------------------------------------------------------------------------------------------
# plan builder and display
# ---------------------------------------------------------------------------------------------------
def test_builder_widths_names_and_encoding():
    pb = PlanBuilder()
    t = pb.table(0, 3, ["x", "y", "z"])
    a = pb.aggregate(t, [0], [(abi.AGG_COUNT, 1)])
    assert pb.width[a] == 2 and pb.names[a] == ["x", "COUNT(y)"]
    n = pb.nodes[a]
    assert n.kind == abi.NODE_AGGREGATE and n.n_keys == 1 and n.left_keys[0] == 0 and n.table_cols == 1
    assert n.n_proj == abi.NO_PROJECTION and pb.pool[n.table_slot:n.table_slot + 2] == [abi.AGG_COUNT, 1]
    b = pb.aggregate(t, [2, 0], [(abi.AGG_COUNT_STAR, None), (abi.AGG_SUM, 1), (abi.AGG_AVG, 1), (abi.AGG_COUNT_DISTINCT, 0)])
    assert pb.width[b] == 6
    assert pb.names[b] == ["z", "x", "COUNT(*)", "SUM(y)", "AVG(y)", "COUNT(DISTINCT x)"]
    d = pb.aggregate(t, [1])              # BI Q4: DISTINCT over a join column, no aggregates: an id column, usable as a join input
    assert pb.width[d] == 1 and pb.names[d] == ["y"]
    j = pb.hash_join(d, t, on=[(0, 1)])
    assert pb.width[j] == 4
    g = pb.aggregate(t, [], [(abi.AGG_COUNT_STAR, None)])
    assert pb.width[g] == 1 and pb.names[g] == ["COUNT(*)"] and pb.nodes[g].n_keys == 0


def test_explain_line():
    pb = PlanBuilder()
    t = pb.table(0, 2, ["x", "y"])
    a = pb.aggregate(t, [0], [(abi.AGG_COUNT, 1)])
    assert explain(pb, a)[0] == "AggregateExec: mode=Single, gby=[x@0 as x], aggr=[COUNT(y@1)]"
    b = pb.aggregate(t, [1], [(abi.AGG_COUNT_STAR, None), (abi.AGG_AVG, 0), (abi.AGG_COUNT_DISTINCT, 0)])
    assert explain(pb, b)[0] == "AggregateExec: mode=Single, gby=[y@1 as y], aggr=[COUNT(*), AVG(x@0), COUNT(DISTINCT x@0)]"
    c = pb.aggregate(t, [1])
    assert explain(pb, c) == ["AggregateExec: mode=Single, gby=[y@1 as y], aggr=[]", "  BoundTableExec: slot=0, columns=[x, y]"]


# ---------------------------------------------------------------------------------------------------
# the restatement against hand-worked vectors
# ---------------------------------------------------------------------------------------------------
INT, INTEGER, DEC, FLT, DBL, STR, NULL = abi.TV_INT, abi.TV_INTEGER, abi.TV_DECIMAL, abi.TV_FLOAT, abi.TV_DOUBLE, abi.TV_STRING, abi.TV_NULL


def test_avg_of_integers_is_a_decimal():
    assert avg_agg([(INTEGER, 1), (INTEGER, 2)]) == (DEC, 15 * E18 // 10)          # AVG(1, 2) = 1.5
    # AVG(1, 2, 2): 5 * 10^18 is scaled to 5 * 10^37 (19 steps), / 3 = 16666..6 (37 digits), / 10^19 => 1.666666666666666666
    assert avg_agg([(INT, 1), (INTEGER, 2), (INT, 2)]) == (DEC, 1666666666666666666)
    assert avg_agg([(INTEGER, -1), (INTEGER, -2), (INTEGER, -2)]) == (DEC, -1666666666666666666)   # truncation toward zero
    assert avg_agg([(DEC, 1), (DEC, 0), (DEC, 0)]) == (DEC, 0)      # 10^-18 / 3 truncates to 0
    # a divisor with trailing zeros adds to the scale: 10^-18 is scaled by 10^38, count 10 strips one zero => 10^39 does not fit: error
    assert avg_agg([(DEC, 1)] + [(DEC, 0)] * 9) == (NULL, None)
    assert decimal_checked_div(7 * E18, 2 * E18) == 35 * E18 // 10


def test_sum_skips_what_avg_refuses():
    assert sum_agg([(INTEGER, 4), (STR, 9), (NULL, None), (INT, 1)]) == (INTEGER, 5)   # sum.rs:52: no `else`
    assert avg_agg([(INTEGER, 4), (STR, 9)]) == (NULL, None)                           # avg.rs:63-78
    assert avg_agg([(INTEGER, 4), (NULL, None)]) == (NULL, None)
    assert count_agg([3, 0, 3, 5]) == (INTEGER, 3)
    assert count_distinct_agg([3, 0, 3, 5]) == (INTEGER, 2)


def test_overflow_is_the_error_value():
    assert sum_agg([(INTEGER, I64_MAX), (INTEGER, 1)]) == (NULL, None)
    assert sum_agg([(INTEGER, I64_MAX), (INTEGER, 1), (INTEGER, -1)]) == (INTEGER, I64_MAX)   # the total decides
    assert sum_agg([(DEC, I128_MAX), (DEC, 1)]) == (NULL, None)
    assert sum_agg([(DEC, I128_MAX), (INTEGER, -1)]) == (DEC, I128_MAX - E18)
    assert avg_agg([(DEC, I128_MAX), (DEC, I128_MAX)]) == (NULL, None)


def test_empty_global_group():
    assert count_agg([]) == (INTEGER, 0)
    assert sum_agg([]) == (INTEGER, 0)
    assert avg_agg([]) == (INTEGER, 0)


def test_promotion_to_double_and_float():
    tag, ap = sum_agg([(INTEGER, 1), (DEC, 5 * E18 // 10), (DBL, 0.25)])
    assert tag == DBL and ap.exact() == 1.75 and ap.check(1.75) and not ap.check(1.7500001)
    tag, ap = sum_agg([(INTEGER, 1), (FLT, 0.5), (DEC, E18)])
    assert tag == FLT and ap.exact() == 2.5
    tag, ap = avg_agg([(INTEGER, 1), (DBL, 2.0)])
    assert tag == DBL and ap.check(1.5)
    tag, ap = sum_agg([(DBL, math.inf), (DBL, -math.inf)])
    assert ap.check(math.nan) and not ap.check(0.0)
    assert sum_agg([(STR, 1), (DBL, 0.5)])[0] == DBL


def test_decimal_to_double_strips_trailing_zeros():
    assert dec_to_f64(15 * E18 // 10) == 1.5
    assert dec_to_f64(-1) == -1e-18
    assert to_f32(INTEGER, 16777217) == 16777216.0


def test_same_compares_device_values():
    assert same((INTEGER, 3), (INTEGER, 3, 0))
    assert same((DEC, -1), (DEC, -1, -1))
    assert not same((DEC, 1), (INTEGER, 1, 0))
    assert same((NULL, None), (NULL, 0, 0))
