"""Computed columns (abi.NODE_EXTEND, PlanBuilder.extend / sparql_bind): the tables, the plans and a Python reference, shared by
test_extend_cpu.py and test_gpu_extend.py.

The reference is built from what the suite already has: arithmetic is numeric_ref.binary / unary / cast over the typed-value table of
agg_cases.py (ids 1 .. 1000 are the xsd:integer of the same value, the named ids its edge values), relations are the lists of rows of
aggcol_cases.py (a cell is an object id, or in a value column the value as (tag, payload), UNBOUND for the error value).  A computed
value is ONE expression per row: there is no summation order, so every comparison is bit for bit (numeric_ref.bits against
numeric_ref.device_bits) and there is no tolerance anywhere."""
import numpy as np

from rdf_fusion_amd import abi
from rdf_fusion_amd.plan import (col, integer, float32, ENC_TV, MUL, DIV, CEIL, ROUND, GT, EBV, BOOLEAN_AS_TERM, xsd_int, xsd_decimal, xsd_float, xsd_double)
import agg_cases as ac
import aggcol_cases as cc
import numeric_ref as nr

IDS, val, tv = ac.IDS, ac.val, cc.tv
UNBOUND, ERR = cc.UNBOUND, nr.ERR
COUNT = abi.AGG_COUNT
INT, INTEGER, DEC, FLT, DBL, BOOL = abi.TV_INT, abi.TV_INTEGER, abi.TV_DECIMAL, abi.TV_FLOAT, abi.TV_DOUBLE, abi.TV_BOOLEAN
BLOCK = 256          # rows per workgroup of extend_kernel: kExtendBlock (rdf-fusion_amd/csrc/kernels.hpp)


class Bits:
    """A float / double / int / boolean payload that aggcol_cases.check_rows compares exactly: same bits, one NaN"""

    def __init__(self, tag, payload):
        self.key = nr.bits((tag, payload))

    def check(self, got):
        t = self.key[0]
        if t == FLT:
            return nr.bits((t, np.float32(got))) == self.key
        if t == DBL:
            return nr.bits((t, np.float64(got))) == self.key
        return got is not None and int(got) == self.key[1]

    def __repr__(self):
        return f"Bits{self.key}"


def cell(value):
    """a reference value as a value-column cell of aggcol_cases' rows"""
    t, p = value
    if t == abi.TV_NULL:
        return UNBOUND
    return value if t in (INTEGER, DEC) else (t, Bits(t, p))


def raw(c):
    """ENC_TV of a cell of such rows: an id's typed value, or the value of a value column (a Bits cell carries its tag and bits)"""
    if isinstance(c, int):
        return val(c)
    t, p = c
    if isinstance(p, Bits):
        lo = p.key[1]
        if t == FLT:
            return t, (np.float32("nan") if lo == "nan" else np.uint32(lo).view(np.float32))
        if t == DBL:
            return t, (np.float64("nan") if lo == "nan" else np.int64(lo).view(np.float64))
        return t, lo
    return c


def extend(rows, fns, keep=None):
    """PlanBuilder.extend on the reference's rows: the kept cells, then fn(row) -> (tag, payload) per computed column"""
    out = []
    for r in rows:
        kept = r if keep is None else tuple(r[c] for c in keep)
        out.append(tuple(kept) + tuple(cell(f(r)) for f in fns))
    return out


# ---------------------------------------------------------------------------------------------------
# expressions: (the program, the reference's function of a row)
# ---------------------------------------------------------------------------------------------------
def mul_cols(a, b):
    return MUL(ENC_TV(col(a)), ENC_TV(col(b))), lambda r: nr.binary(abi.EX_MUL, raw(r[a]), raw(r[b]))


def ratio(a, b):
    """BI Q3: DIV(xsd:float(count@a), count@b)"""
    return DIV(xsd_float(ENC_TV(col(a))), ENC_TV(col(b))), lambda r: nr.binary(abi.EX_DIV, cast(FLT, raw(r[a])), raw(r[b]))


def percent(a):
    """ROUND(x * 100)"""
    return ROUND(MUL(ENC_TV(col(a)), integer(100))), lambda r: nr.unary(abi.EX_ROUND, nr.binary(abi.EX_MUL, raw(r[a]), (INTEGER, 100)))


def cast(target, v):
    return ERR if v[0] == abi.TV_NULL else nr.cast(target, v)


def gt(a, b):
    x, y = cc.exact(a), cc.exact(b)
    return ERR if x is None or y is None else (BOOL, int(x > y))


# One plan with 8 computed columns over (a, b): every kind the record carries, and the error value
KINDS = [
    ("int", xsd_int(MUL(ENC_TV(col(0)), integer(1 << 30))), lambda r: cast(INT, nr.binary(abi.EX_MUL, raw(r[0]), (INTEGER, 1 << 30)))),
    ("integer", *mul_cols(0, 1)),
    ("decimal", DIV(ENC_TV(col(0)), ENC_TV(col(1))), lambda r: nr.binary(abi.EX_DIV, raw(r[0]), raw(r[1]))),
    ("float", CEIL(MUL(xsd_float(ENC_TV(col(0))), float32(-0.5))),
     lambda r: nr.unary(abi.EX_CEIL, nr.binary(abi.EX_MUL, cast(FLT, raw(r[0])), (FLT, np.float32(-0.5))))),
    ("double", DIV(xsd_double(ENC_TV(col(0))), xsd_double(ENC_TV(col(1)))), lambda r: nr.binary(abi.EX_DIV, cast(DBL, raw(r[0])), cast(DBL, raw(r[1])))),
    ("boolean", BOOLEAN_AS_TERM(EBV(GT(ENC_TV(col(0)), ENC_TV(col(1))))), lambda r: gt(raw(r[0]), raw(r[1]))),
    ("error", DIV(xsd_decimal(ENC_TV(col(0))), integer(0)), lambda r: nr.binary(abi.EX_DIV, cast(DEC, raw(r[0])), (INTEGER, 0))),
    ("as is", ENC_TV(col(1)), lambda r: raw(r[1])),
]


def kinds_rows():
    """(a, b) ids: small integers, zero divisors, negative values, the i64 / i128 edges, a float, a double, an unbound id"""
    n = IDS
    pairs = [(n["i5"], n["i3"]), (n["i1"], n["i0"]), (n["i0"], n["i0"]), (n["i-1"], 4), (2, n["i-1"]), (n["i2^32"], n["i2^32"]),
             (n["iMAX"], n["iMAX"]), (n["f0.75"], n["g0.5"]), (n["d-E18"], n["dMIN"]), (n["dMAX"], n["d-1"]), (n["unbound"], n["i1"]),
             (n["int-1"], n["int2^31-1"]), (3, n["f0.75"]), (n["i1"], n["unbound"])]
    return [np.asarray([p[0] for p in pairs], np.uint32), np.asarray([p[1] for p in pairs], np.uint32)]


# ---------------------------------------------------------------------------------------------------
# the tables and the plans
# ---------------------------------------------------------------------------------------------------
def mul_table(n, seed=4):
    """(a, b): n rows of small xsd:integer ids"""
    rng = np.random.default_rng(seed + n)
    return [rng.integers(1, 1001, n).astype(np.uint32), rng.integers(1, 1001, n).astype(np.uint32)]


def keyed_tables(n, seed=9):
    """(k, a) and (k, b): the same n unique keys in two orders: their inner join has n rows"""
    rng = np.random.default_rng(seed + n)
    k = np.arange(n, dtype=np.uint32) * 2 + 2001
    a, b = mul_table(n, seed)
    p = rng.permutation(n)
    return [k, a], [k[p], b[p]]


def q3_tables(products=300, seed=21):
    """(product, review) of this month and of the month before: 1 to 6 reviews per product; a third of the products (every third)
    have no review the month before"""
    rng = np.random.default_rng(seed)
    prod = np.arange(products, dtype=np.uint32) + 5000

    def month(keep):
        n = rng.integers(1, 7, products) * keep
        who = np.repeat(prod, n)
        perm = rng.permutation(len(who))
        return [who[perm], rng.integers(1, 1001, len(who)).astype(np.uint32)[perm]]
    return month(np.ones(products, np.int64)), month((np.arange(products) % 3 != 0).astype(np.int64))


def q3_plan(pb, now, before, join_type=abi.JOIN_LEFT):
    """BI Q3's shape: two COUNTs joined by product, then `DIV(xsd:float(monthCount@1), monthBeforeCount@2) as ratio`"""
    a = pb.aggregate(now, [0], [(COUNT, 1)])
    b = pb.aggregate(before, [0], [(COUNT, 1)])
    j = pb.hash_join(a, b, [(0, 0)], join_type=join_type, projection=[0, 1, 3])
    p = pb.projection(j, [0, 1, 2], names=["product", "monthCount", "monthBeforeCount"])
    return pb.extend(p, [ratio(1, 2)[0]], names=["ratio"])


def q3_reference(now, before, join_type=abi.JOIN_LEFT):
    a = cc.aggregate(cc.rows_of(now), [0], [(COUNT, 1)])
    b = cc.aggregate(cc.rows_of(before), [0], [(COUNT, 1)])
    j = [tuple(r[c] for c in (0, 1, 3)) for r in cc.join(a, b, [(0, 0)], join_type, right_width=2)]
    return extend(j, [ratio(1, 2)[1]])


def string_rows(with_string):
    """(x): integers, and (with_string) one string literal among them"""
    ids = [3, 7, IDS["str"] if with_string else 9, 11, 5]
    return [np.asarray(ids, np.uint32)]
