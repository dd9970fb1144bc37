"""TopK (DISTINCT + ORDER BY keys LIMIT k per group) at its output order and its group-size edges: one typed-value table, the case
tables and a plain Python reference, shared by test_topk_order_cpu.py (oracle = reference, on a machine without a GPU) and
test_gpu_topk_edges.py (the device's rows, as a sequence, = reference).

The contract (include/rdfgpu.h, RDFGPU_NODE_TOPK): groups come out in ascending group id; inside a group the rows come out in
ascending key-tuple order, NULLS FIRST; rows equal on (group, keys) collapse to one; at most k rows per group.  The key of an id is
the id (SORT_BY_ID), (tag, rank) of its typed value (SORT_BY_TERM) or its value as a double in IEEE total order (SORT_BY_DOUBLE).

Geometry: the device gives every group one 64-lane wave, which scans the group's rows 64 at a time and reduces the lanes' candidates in
six shuffle steps, k times.  Hence groups of 1, 2, 63, 64, 65, 127, 128, 129 and 1000 rows, limits on either side of 64 and the largest
one the operator takes (1024), and sparse group ids (0 .. 70000) so that most groups between them are empty."""
import struct
from collections import namedtuple

import numpy as np

import numeric_ref as nr
from rdf_fusion_amd import abi
from rdf_fusion_amd.engine import TV_DTYPE
from rdf_fusion_amd.plan import PlanBuilder, col, lit_id, ID_EQ

BY_ID, BY_TERM, BY_DOUBLE = abi.SORT_BY_ID, abi.SORT_BY_TERM, abi.SORT_BY_DOUBLE
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
MAX_LIMIT, GROUP_ID_LIMIT = 1024, 1 << 24                 # what the compile step and exec_topk accept: limits 1 .. 1024, group ids below 2^24

# ---------------------------------------------------------------------------------------------------
# the typed-value table
# ---------------------------------------------------------------------------------------------------
N_STR, N_IRI, N_BNODE = 150, 40, 20
E18 = 10 ** 18
# (tag, payload) in the form of numeric_ref.py: a Python int for xsd:int / xsd:integer, the i128 of 10^-18 units for xsd:decimal, a numpy
# float for xsd:float / xsd:double.  NaNs with the sign bit set are left out: the all-ones pattern maps to key 0, the key of a null, and
# whether a store can hold such a NaN at all is a question for the loader, not for this operator.
NUMERICS = [
    (abi.TV_DOUBLE, np.float64("-inf")), (abi.TV_DOUBLE, np.float64(-1.5)), (abi.TV_DOUBLE, np.float64(-0.0)), (abi.TV_DOUBLE, np.float64(0.0)),
    (abi.TV_DOUBLE, np.float64(5e-324)), (abi.TV_DOUBLE, np.float64(1.5)), (abi.TV_DOUBLE, np.float64("inf")), (abi.TV_DOUBLE, np.float64("nan")),
    (abi.TV_INTEGER, 2 ** 53), (abi.TV_INTEGER, 2 ** 53 + 1), (abi.TV_INTEGER, I64_MIN), (abi.TV_INTEGER, I64_MAX),
    (abi.TV_INTEGER, 0), (abi.TV_INTEGER, -7), (abi.TV_INTEGER, 2),
    (abi.TV_INT, -2 ** 31), (abi.TV_INT, 2 ** 31 - 1), (abi.TV_INT, 2), (abi.TV_INT, -7),
    (abi.TV_FLOAT, np.float32(1.5)), (abi.TV_FLOAT, np.float32(-0.0)), (abi.TV_FLOAT, np.float32(0.1)), (abi.TV_FLOAT, np.float32("inf")),
    (abi.TV_FLOAT, np.float32("nan")), (abi.TV_FLOAT, np.float32(1e-45)), (abi.TV_FLOAT, np.float32(-3.25)),
    (abi.TV_DECIMAL, 3 * E18 // 2), (abi.TV_DECIMAL, -13 * E18 // 4), (abi.TV_DECIMAL, 2 * E18), (abi.TV_DECIMAL, 0), (abi.TV_DECIMAL, -E18 // 8),
    (abi.TV_DECIMAL, 1234567890123456789), (abi.TV_DECIMAL, -(2 ** 100)), (abi.TV_DECIMAL, 2 ** 126),
]


def typed_table():
    """-> (tv, decimals, ids): ids 1 .. of plain and language-tagged strings, IRIs, blank nodes and numerics.  Ranks are a permutation of
    their kind's ids, spread over all 56 bits (the key packs tag << 56 | rank, and a rank has a high and a low word), so neither the id nor
    one word of the rank orders like the term.  Every tenth string shares its rank with the string before it (the same lexical form under
    another language tag): only a later key by id separates the two."""
    rng = np.random.default_rng(77)
    n_ids = 1 + N_STR + N_IRI + N_BNODE + len(NUMERICS)
    tv = np.zeros(n_ids, dtype=TV_DTYPE)
    ids = {}
    at = 1
    for kind, tag, n in (("str", abi.TV_STRING, N_STR), ("iri", abi.TV_NAMED_NODE, N_IRI), ("bnode", abi.TV_BLANK_NODE, N_BNODE)):
        rank = rng.permutation(n).astype(np.int64)
        rank[rank % 3 == 1] += 1 << 33                                   # equal low words, different high words
        rank[rank % 3 == 2] <<= 40
        rank[int(np.argmax(rank))] = (1 << 56) - 1
        assert len(set(rank.tolist())) == n and rank.max() < 1 << 56
        ids[kind] = list(range(at, at + n))
        tv["tag"][at:at + n] = tag
        tv["lo"][at:at + n] = rank
        at += n
    s0 = ids["str"][0]
    tv["aux"][s0:s0 + N_STR:7] = 3                                       # language-tagged
    ids["twins"] = []
    for i in range(s0 + 9, s0 + N_STR, 10):
        tv["lo"][i] = tv["lo"][i - 1]
        tv["aux"][i] = 5
        ids["twins"].append((i - 1, i))
    ids["num"] = list(range(at, at + len(NUMERICS)))
    dec = []
    for i, (tag, v) in zip(ids["num"], NUMERICS):
        tv["tag"][i] = tag
        if tag == abi.TV_DECIMAL:
            raw = v & ((1 << 128) - 1)
            tv["lo"][i] = len(dec)
            dec.append([raw & ((1 << 64) - 1), raw >> 64])
        elif tag == abi.TV_FLOAT:
            tv["lo"][i] = int(np.float32(v).view(np.uint32))
        elif tag == abi.TV_DOUBLE:
            tv["lo"][i] = int(np.float64(v).view(np.int64))
        else:
            tv["lo"][i] = v
    ids["beyond"] = n_ids + 3                                            # an id the table does not reach: a null for TERM and DOUBLE keys
    return tv, np.array(dec, dtype=np.uint64).astype(np.int64).reshape(-1, 2), ids


TV, DECIMALS, IDS = typed_table()

# ---------------------------------------------------------------------------------------------------
# the reference: Python ints and tuples, sorted(set(..))[:k] per group
# ---------------------------------------------------------------------------------------------------
def total_order_key(v):
    """a double as an unsigned integer that orders like IEEE total order; None (unbound / not a number) first"""
    if v is None:
        return 0
    bits = struct.unpack("<Q", struct.pack("<d", v))[0]
    return (~bits) & ((1 << 64) - 1) if bits >> 63 else bits | (1 << 63)


def numeric_value(i, tv, decimals):
    """(tag, payload) of id i as numeric_ref.py wants it, or None where the id has no number"""
    if not 0 < i < len(tv):
        return None
    tag, lo = int(tv["tag"][i]), int(tv["lo"][i])
    if tag in (abi.TV_INT, abi.TV_INTEGER):
        return tag, lo
    if tag == abi.TV_FLOAT:
        return tag, np.uint32(lo & 0xFFFFFFFF).view(np.float32)
    if tag == abi.TV_DOUBLE:
        return tag, np.int64(lo).view(np.float64)
    if tag == abi.TV_DECIMAL:
        low, high = (int(x) & ((1 << 64) - 1) for x in decimals[lo])
        raw = (high << 64) | low
        return tag, raw - (1 << 128) if raw >> 127 else raw
    return None


def sort_key(i, how, tv, decimals):
    if how == BY_ID:
        return i
    if how == BY_TERM:
        return (int(tv["tag"][i]), int(tv["lo"][i])) if 0 < i < len(tv) else (0, 0)
    v = numeric_value(i, tv, decimals)
    return 0 if v is None else total_order_key(float(nr.to_f64(*v)))


def reference(cols, keys, limit, group, projection, tv, decimals):
    """The rows TopK gives, as a list of tuples in output order.  `keys` as PlanBuilder.topk takes them; like the builder, every output
    column that is not the group column also orders by its id after the keys (a column that is a key by id already decides nothing twice)."""
    out_cols = list(range(len(cols))) if projection is None else [int(c) for c in projection]
    groups = {}
    for row in zip(*[np.asarray(c).tolist() for c in cols]):
        g = row[group] if group is not None else 0
        k = tuple(sort_key(row[c], how, tv, decimals) for c, how in keys) + tuple(row[c] for c in out_cols if c != group)
        groups.setdefault(g, set()).add((k, tuple(row[c] for c in out_cols)))
    rows = []
    for g in sorted(groups):
        rows += [out for _, out in sorted(groups[g])[:limit]]
    return rows


# ---------------------------------------------------------------------------------------------------
# the case tables
# ---------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name cols keys limit group projection")

LADDER_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 1000, 7)
LADDER_GROUPS = (3, 70000, 5, 0, 4000, 1, 10, 9, 4, 69999)              # sparse, unordered against the sizes; 0 is a group like any other
LADDER_LIMITS = (1, 5, 63, 64, 65, MAX_LIMIT)
TERM_KEYS = ((1, BY_TERM), (2, BY_ID))
PRODUCTS = list(range(1000, 1040))


def _u32(*cols):
    return [np.asarray(c, dtype=np.uint32) for c in cols]


def _shuffled(rng, rows):
    """rows (a list of tuples) in a seeded random order -> u32 columns"""
    rows = [rows[i] for i in rng.permutation(len(rows))]
    return _u32(*zip(*rows))


def term_pool():
    return IDS["str"] + IDS["iri"] + IDS["bnode"] + [0, IDS["beyond"]]


def ladder_table(sizes=LADDER_SIZES, groups=LADDER_GROUPS, seed=5):
    """(g, label, product): group groups[i] holds sizes[i] rows, no two of them alike - so a group of n rows gives exactly min(n, k) rows and the
    limits 63, 64 and 65 cut the groups of 63, 64 and 65 rows on either side"""
    rng = np.random.default_rng(seed)
    pool = term_pool()
    rows = []
    for g, size in zip(groups, sizes):
        picks = rng.choice(len(pool) * len(PRODUCTS), size, replace=False)
        rows += [(g, pool[p // len(PRODUCTS)], PRODUCTS[p % len(PRODUCTS)]) for p in picks.tolist()]
    return _shuffled(rng, rows)


def duplicates_table():
    """group 1: 50 times one row; group 2: 100 rows, three distinct; group 3: 90 rows, its fifth and sixth tuple equal up to the last key (the
    product); group 6: 70 rows, its fifth and sixth tuple two strings of one rank, which only the label's id - the key the builder appends -
    separates"""
    rng = np.random.default_rng(6)
    by_rank = sorted(IDS["str"], key=lambda i: (int(TV["lo"][i]), i))
    twin_a, twin_b = IDS["twins"][2]
    low = [i for i in by_rank if int(TV["lo"][i]) < int(TV["lo"][twin_a])][:2]
    assert len(low) == 2 and twin_a < twin_b
    a, b, c = by_rank[0], by_rank[1], by_rank[-1]
    rows = [(1, b, 1003)] * 50
    rows += [(2, (a, b, 0)[i % 3], 1001) for i in range(100)]
    g3 = [(3, a, p) for p in (1000, 1001, 1002, 1003)] + [(3, b, 1010), (3, b, 1011), (3, b, 1030), (3, c, 1000), (3, c, 1001)]
    rows += [g3[i % len(g3)] for i in range(90)]
    g6 = [(6, low[0], 1000), (6, low[0], 1001), (6, low[1], 1000), (6, low[1], 1005), (6, twin_a, 1007), (6, twin_b, 1007), (6, twin_b, 1008)]
    rows += [g6[i % len(g6)] for i in range(70)]
    return _shuffled(rng, rows)


def nulls_table():
    """(g, x, y): x over the null id, an id beyond the table and a few terms; y over few ids, the null id and an id beyond the table among them"""
    rng = np.random.default_rng(7)
    xs = [0, IDS["beyond"], IDS["beyond"] + 9] + IDS["str"][:4] + IDS["iri"][:2] + IDS["bnode"][:1]
    ys = [0, 1000, 1001, IDS["beyond"]]
    rows = [(int(g), xs[int(x)], ys[int(y)]) for g, x, y in zip(rng.choice([0, 2, 7], 260, p=[0.1, 0.3, 0.6]), rng.integers(0, len(xs), 260), rng.integers(0, len(ys), 260))]
    return _shuffled(rng, rows)


def nulls_double_table():
    """(g, value, offer): numerics among strings, IRIs, the null id and an id beyond the table - the last four kinds all carry key 0, so among them
    the offer decides, then the value's id"""
    rng = np.random.default_rng(8)
    vs = IDS["num"][:12] + IDS["str"][:3] + IDS["iri"][:3] + [0, IDS["beyond"]]
    rows = [(int(g), vs[int(v)], int(o)) for g, v, o in zip(rng.choice([1, 4], 300), rng.integers(0, len(vs), 300), rng.integers(1, 6, 300))]
    return _shuffled(rng, rows)


def four_key_table():
    """(g, a, b, c, d) for the keys (a BY_TERM, b BY_DOUBLE, c BY_ID, d BY_ID), output (g, c, d): a over two strings of one rank, one other string
    and the null id; b over 2^53 and 2^53 + 1 (one double), -0.0, +0.0 and a string; c over three ids, d over six.  Rows that differ only in
    which twin or which of the two integers they hold collapse, since neither column is in the output; a good many tuples differ in d alone."""
    rng = np.random.default_rng(9)
    twin_a, twin_b = IDS["twins"][0]
    num = IDS["num"]
    a_s = [twin_a, twin_b, IDS["str"][0], 0]
    b_s = [num[8], num[9], num[2], num[3], IDS["str"][1]]
    sizes = {0: 65, 2: 200, 11: 335}
    rows = []
    for g, n in sizes.items():
        rows += [(g, a_s[int(a)], b_s[int(b)], int(c), int(d)) for a, b, c, d in
                 zip(rng.integers(0, 4, n), rng.integers(0, 5, n), rng.integers(500, 503, n), rng.integers(600, 606, n))]
    return _shuffled(rng, rows)


def numeric_table():
    """(price, offer): every numeric of the table, two strings, an IRI, the null id and an id beyond the table, five offers each"""
    rng = np.random.default_rng(10)
    vs = IDS["num"] + IDS["str"][:2] + IDS["iri"][:1] + [0, IDS["beyond"]]
    return _shuffled(rng, [(v, o) for v in vs for o in range(1, 6)])


def _cases():
    out = []
    ladder, dup, nulls, nd, four, num = ladder_table(), duplicates_table(), nulls_table(), nulls_double_table(), four_key_table(), numeric_table()
    for limit in LADDER_LIMITS:
        out.append(Case(f"ladder-k{limit}-grouped", ladder, TERM_KEYS, limit, 0, None))
        out.append(Case(f"ladder-k{limit}-one-group", ladder, TERM_KEYS, limit, None, [1, 2]))
    out.append(Case("duplicates-k5", dup, TERM_KEYS, 5, 0, None))
    out.append(Case("duplicates-k1", dup, TERM_KEYS, 1, 0, None))
    out.append(Case("duplicates-k5-projection-201", dup, TERM_KEYS, 5, 0, [2, 0, 1]))
    out.append(Case("duplicates-k5-no-group-column", dup, TERM_KEYS, 5, 0, [1, 2]))
    out.append(Case("duplicates-k5-one-group", dup, TERM_KEYS, 5, None, [2, 1]))
    out.append(Case("nulls-first-key", nulls, TERM_KEYS, 6, 0, None))
    out.append(Case("nulls-later-key", nulls, ((2, BY_ID), (1, BY_TERM)), 9, 0, None))
    out.append(Case("nulls-one-group", nulls, TERM_KEYS, 64, None, [1, 2]))
    out.append(Case("nulls-under-double", nd, ((1, BY_DOUBLE), (2, BY_ID)), 30, 0, None))
    out.append(Case("nulls-under-double-one-group", nd, ((1, BY_DOUBLE), (2, BY_ID)), 65, None, [2, 1]))
    four_keys = ((1, BY_TERM), (2, BY_DOUBLE), (3, BY_ID), (4, BY_ID))
    out.append(Case("four-keys-grouped", four, four_keys, 40, 0, [0, 3, 4]))
    out.append(Case("four-keys-one-group", four, four_keys, MAX_LIMIT, None, [4, 3]))
    out.append(Case("numeric-order", num, ((0, BY_DOUBLE), (1, BY_ID)), 500, None, None))
    out.append(Case("numeric-order-k7", num, ((0, BY_DOUBLE),), 7, None, [1, 0]))
    return out


CASES = _cases()
CASE_IDS = [c.name for c in CASES]
_REFS = {}


def case_named(name):
    return CASES[CASE_IDS.index(name)]


def expected(c):
    """reference(..) of a case: computed once, shared by the tests that need it and left unchanged"""
    if c.name not in _REFS:
        _REFS[c.name] = reference(c.cols, c.keys, c.limit, c.group, c.projection, TV, DECIMALS)
    return _REFS[c.name]


def as_matrix(rows, width):
    """a list of row tuples as an (n, width) u32 array - what np.stack(columns, 1) gives"""
    return np.array(rows, dtype=np.uint32).reshape(len(rows), width)


def out_width(c):
    return len(c.cols) if c.projection is None else len(c.projection)


def topk_plan(c, limit=None):
    pb = PlanBuilder()
    return pb.build(pb.topk(pb.table(0, len(c.cols)), keys=list(c.keys), limit=c.limit if limit is None else limit, group=c.group, projection=c.projection))


# ---------------------------------------------------------------------------------------------------
# TopK above a FilterExec: the input's row count is known on the device only
# ---------------------------------------------------------------------------------------------------
KEEP_ID, NEVER_ID = 7, 11


def with_flag_column(c, seed=12):
    """the case's columns and one more, drawn from 1 .. 10: about one row in ten carries KEEP_ID, none carries NEVER_ID"""
    flag = np.random.default_rng(seed).integers(1, 11, len(c.cols[0])).astype(np.uint32)
    return list(c.cols) + [flag]


def filtered_topk_plan(c, flag_id):
    """TopK over  FilterExec(flag = flag_id)  of the case's table with its flag column (projected away by the filter)"""
    w = len(c.cols)
    pb = PlanBuilder()
    f = pb.filter(pb.table(0, w + 1), ID_EQ(col(w), lit_id(flag_id)), projection=list(range(w)))
    return pb.build(pb.topk(f, keys=list(c.keys), limit=c.limit, group=c.group, projection=c.projection))


def surviving(cols_with_flag, flag_id):
    keep = cols_with_flag[-1] == flag_id
    return [col_[keep] for col_ in cols_with_flag[:-1]]


# ---------------------------------------------------------------------------------------------------
# re-execution of one plan over tables of other sizes, and the largest group id
# ---------------------------------------------------------------------------------------------------
def small_table():
    """(g, label, product): 40 rows in groups 0 .. 3"""
    return ladder_table(sizes=(3, 20, 9, 8), groups=(2, 0, 3, 1), seed=13)


def group_bound_table(max_group):
    """three rows, in groups 0, 5 and max_group"""
    s = IDS["str"]
    return _u32([5, max_group, 0], [s[4], s[2], s[9]], [1002, 1001, 1000])
