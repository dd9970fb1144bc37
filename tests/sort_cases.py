"""SortExec (abi.NODE_SORT, PlanBuilder.sort / sparql_order_by): the typed-value table, the sort key of a value restated in Python, the
reference order and the case tables, shared by test_sort_cpu.py and test_gpu_sort.py.

The contract (include/rdfgpu.h, RDFGPU_NODE_SORT): rows come out in lexicographic order of their keys, each ascending or descending;
rows equal on every key keep ascending input row order; a fetch keeps the first rows; nothing is de-duplicated.  A key by value is the
reference's sortable encoding (lib/encoding/src/sortable_term/builder.rs:24-39,113-140; term_type.rs:56-70; encoders/typed_value.rs:23-50;
lib/model/src/xsd/numeric.rs:52-60): the tuple (type, numeric, bytes).  The reference is `sorted` over those tuples: the device's row
sequence must equal it exactly, there is no tolerance anywhere.

The typed-value table is agg_cases.TV / DECIMALS with the edge values of the sortable encoding appended (the ids of agg_cases stay what
they are): a value column over it is `ENC_TV(col)` of an id column, computed by a ProjectionExec with expressions."""
import struct

import numpy as np

from rdf_fusion_amd import abi
from rdf_fusion_amd.plan import col, ENC_TV
import agg_cases as ac
import numeric_ref as nr

INT, INTEGER, DEC, FLT, DBL, BOOL = abi.TV_INT, abi.TV_INTEGER, abi.TV_DECIMAL, abi.TV_FLOAT, abi.TV_DOUBLE, abi.TV_BOOLEAN
STRING, IRI, BNODE = abi.TV_STRING, abi.TV_NAMED_NODE, abi.TV_BLANK_NODE
BY_ID, BY_TERM, BY_DOUBLE, BY_VALUE = abi.SORT_BY_ID, abi.SORT_BY_TERM, abi.SORT_BY_DOUBLE, abi.SORT_BY_VALUE
E18 = 10 ** 18
T = 1024                      # rows per tile of sort_tile_kernel: kSortTile (rdf-fusion_amd/csrc/kernels.hpp)
MAX_WORDS = 8                 # words of the widest key record: kSortMaxWords (a key by value takes 4, any other 1, the row index 1)
NAN = 0x7FF8000000000000      # the one NaN of the table (a quiet NaN; two NaNs of different bits would order by their bits)

# (name, tag, payload): a float / double payload is the value, a string's / IRI's its rank (the ENC_SORT order of its kind)
EXTRA = [
    ("g-0", DBL, -0.0), ("g+0", DBL, 0.0), ("g-inf", DBL, float("-inf")), ("g+inf", DBL, float("inf")), ("gNaN", DBL, float("nan")),
    ("g1.5", DBL, 1.5), ("g-1.5", DBL, -1.5),
    ("int2", INT, 2), ("f2", FLT, 2.0), ("g2", DBL, 2.0), ("d2", DEC, 2 * E18),                      # with id 2, the xsd:integer 2
    ("i2^53", INTEGER, 2 ** 53), ("i2^53+1", INTEGER, 2 ** 53 + 1),
    ("i-2", INTEGER, -2), ("int0", INT, 0), ("f+0", FLT, 0.0),
    ("bF", BOOL, 0), ("bT", BOOL, 1),
    ("sA", STRING, 10), ("sB", STRING, 11), ("sC", STRING, 12), ("iriA", IRI, 3), ("iriB", IRI, 4),
]


def typed_table():
    """agg_cases' table with EXTRA appended -> (tv, decimals, ids by name, values)"""
    first = len(ac.TV)
    tv = np.zeros(first + len(EXTRA), dtype=ac.TV.dtype)
    tv[:first] = ac.TV
    dec = [list(map(int, row)) for row in ac.DECIMALS.astype(np.uint64)]
    ids, values = dict(ac.IDS), list(ac.VALUES)
    for i, (name, tag, v) in enumerate(EXTRA, start=first):
        ids[name] = i
        tv["tag"][i] = tag
        if tag == DEC:
            raw = v & ((1 << 128) - 1)
            tv["lo"][i] = len(dec)
            dec.append([raw & ((1 << 64) - 1), raw >> 64])
        elif tag == FLT:
            tv["lo"][i] = int(np.float32(v).view(np.uint32))
        elif tag == DBL:
            tv["lo"][i] = NAN if v != v else int(np.float64(v).view(np.int64))
        else:
            tv["lo"][i] = v
        values.append((tag, np.float32(v) if tag == FLT else np.float64(v) if tag == DBL else v))
    return tv, np.array(dec, dtype=np.uint64).astype(np.int64).reshape(-1, 2), ids, values


TV, DECIMALS, IDS, VALUES = typed_table()


def val(i):
    """the typed value of object id i as (tag, payload); id 0 and ids past the table are unbound"""
    return VALUES[i] if 0 < i < len(VALUES) else (abi.TV_NULL, None)


# ---------------------------------------------------------------------------------------------------
# the sort keys
# ---------------------------------------------------------------------------------------------------
def ordered_double(x):
    """an f64 as the integer whose order is IEEE total order: -NaN < -inf < .. < -0 < +0 < .. < +inf < NaN"""
    b = NAN if x != x else int(np.float64(x).view(np.uint64))
    return b ^ ((1 << 64) - 1) if b >> 63 else b | (1 << 63)


def be_bytes(tag, v):
    """Numeric::to_be_bytes (numeric.rs:52-60) / Boolean::to_be_bytes"""
    if tag == INT:
        return struct.pack(">i", v)
    if tag == INTEGER:
        return struct.pack(">q", v)
    if tag == FLT:
        return struct.pack(">f", float(v))
    if tag == DBL:
        return struct.pack(">Q", NAN) if v != v else struct.pack(">d", float(v))
    if tag == DEC:
        return (v & ((1 << 128) - 1)).to_bytes(16, "big")
    return bytes([int(v != 0)])


def sort_key(value):
    """ENC_SORT of a typed value a 24-byte record can carry, as the tuple (type, ordered double, bytes): the error value / unbound is
    (0, 0, b"") (builder.rs:24-26: a valid struct of type Null), a boolean type 3 with numeric 0.0 / 1.0, a numeric type 4 with
    Double::from(Numeric).  Python compares bytes as byte strings, a prefix first."""
    tag, v = value
    if tag == abi.TV_NULL:
        return (0, 0, b"")
    if tag == BOOL:
        return (3, ordered_double(1.0 if v else 0.0), be_bytes(tag, v))
    assert tag in nr.NUMERIC, value
    return (4, ordered_double(nr.to_f64(tag, v)), be_bytes(tag, v))


def id_key(how, i):
    """the key of an object id as RDFGPU_NODE_TOPK defines it: the id; (tag, rank) of a string / IRI / blank node; the numeric value as
    a double in total order, unbound and everything else first"""
    if how == BY_ID:
        return i
    tag, v = val(i)
    if how == BY_DOUBLE:
        return ordered_double(nr.to_f64(tag, v)) if tag in nr.NUMERIC else 0
    assert tag in (abi.TV_NULL, STRING, IRI, BNODE), (i, tag)
    return 0 if tag == abi.TV_NULL else (tag << 56) | v


class Desc:
    """a key compared the other way round"""

    def __init__(self, k):
        self.k = k

    def __lt__(self, other):
        return other.k < self.k

    def __eq__(self, other):
        return self.k == other.k


def reference(rows, keys, fetch=None):
    """rows = one tuple of object ids per input row; keys = [(column, how, descending)], a BY_VALUE column's id standing for its typed
    value (the value column is ENC_TV of it).  -> the input row indexes in output order"""
    def key(r):
        parts = []
        for c, how, desc in keys:
            k = sort_key(val(rows[r][c])) if how == BY_VALUE else id_key(how, rows[r][c])
            parts.append(Desc(k) if desc else k)
        return (*parts, r)
    order = sorted(range(len(rows)), key=key)
    return order if not fetch else order[:fetch]


# ---------------------------------------------------------------------------------------------------
# the case tables
# ---------------------------------------------------------------------------------------------------
SIZES = [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 5, 5 * T + 3]
WIDE_SIZES = SIZES[-3:]
FETCH_N = 3 * T + 5
FETCHES = [1, 10, T - 1, T, T + 1, FETCH_N, FETCH_N + 7]

# the value edges: every id twice over, so that equal keys meet and keep their input order
EDGE_NAMES = ["g-0", "g+0", "g-inf", "g+inf", "gNaN", "g1.5", "g-1.5", "int2", "i2", "f2", "g2", "d2", "i2^53", "i2^53+1", "i-1", "i-2",
              "i1", "int0", "i0", "d0", "f+0", "bF", "bT", "unbound", "iMIN", "iMAX", "dMIN", "dMAX", "f0.75", "g0.5", "int-2^31"]


def edge_ids():
    ids = dict(IDS, i2=2)
    once = [ids[n] for n in EDGE_NAMES]
    return np.asarray(once + once[::-1], np.uint32)


def id_table(n, seed=3, hi=40):
    """(x, y, z): n rows of small xsd:integer ids, few distinct values per column: ties in every prefix of the keys"""
    rng = np.random.default_rng(seed + n)
    return [rng.integers(1, hi + 1, n).astype(np.uint32), rng.integers(1, 8, n).astype(np.uint32), rng.integers(0, 4, n).astype(np.uint32)]


def mixed_table(n, seed=5):
    """(v, x, d, s): v ids of numeric values of every kind (and unbound), x small ids, d ids for BY_DOUBLE, s strings / IRIs for BY_TERM"""
    rng = np.random.default_rng(seed + n)
    pick = lambda names: np.asarray([dict(IDS, i2=2)[m] for m in names], np.uint32)
    v = pick(["unbound", "g-0", "g+0", "int2", "i2", "f2", "g2", "d2", "i2^53", "i2^53+1", "i-1", "bT", "bF", "g+inf", "f0.75", "d-1", "dE18"])
    d = pick(["unbound", "i1", "i-1", "g0.5", "f0.75", "d1", "sA", "g-0", "g+0"])
    s = pick(["unbound", "sA", "sB", "sC", "iriA", "iriB"])
    return [v[rng.integers(0, len(v), n)], rng.integers(1, 6, n).astype(np.uint32), d[rng.integers(0, len(d), n)], s[rng.integers(0, len(s), n)]]


def rows_of(cols):
    return list(zip(*[c.tolist() for c in cols]))


def value_plan(pb, table, value_cols):
    """every column of `table`, then ENC_TV of each of `value_cols` as a value column -> (node, {id column: its value column})"""
    w = pb.width[table]
    e = pb.extend(table, [ENC_TV(col(c)) for c in value_cols], names=[f"v{c}" for c in value_cols])
    return e, {c: w + q for q, c in enumerate(value_cols)}
