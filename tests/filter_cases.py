"""FILTER's streamed and run-copy forms at their tile and run edges: the typed-value table, the literals, the per-id answer in plain
Python, the row layouts of one predicate partition and what each layout must contain, shared by test_filter_cases_cpu.py (the Python answer
= the oracle's, the edges are in the data; on a machine without a GPU) and test_gpu_filter_edges.py (the device = the Python answer).

Geometry (kernels.hip, plan_filter.cpp).  A typed comparison `EBV(cmp(ENC_TV(col), literal))` is shape 2.  Below 2^20 rows, with three
output columns, or with an output column in another 16-byte phase than the predicate column it runs in one pass (filter_kernel<2>, no
order promised).  From 2^20 rows it is streamed: one verdict bit per row and a count per 4096-row tile (filter_bits_kernel<2>), a scan,
an ordered write (filter_write_kernel).  Over the sorted column of a store slice whose id range [first, last] has span = last - first + 1
ids: span * 4 <= rows answers the comparison once per id (value_verdict_kernel, 64 ids per ballot) and the rows read one bit
(filter_bits_kernel<4>: the first and the last id of a 16-byte group bring their 32-id verdict words, an id in between that shares
neither loads its own); span * 1024 <= rows copies the qualifying runs instead (value_runs_kernel or the slice's cached starts,
run_scan_kernel: 1024 lanes with ceil(span / 1024) ids each, run_copy_kernel: 4096 output rows per workgroup, 16-byte stores from the
first output row that is a multiple of 4)."""
import math
from collections import namedtuple
from functools import lru_cache

import numpy as np

from rdf_fusion_amd import abi
from rdf_fusion_amd.engine import TV_DTYPE
from rdf_fusion_amd.plan import (PlanBuilder, quad_pattern, col, integer, int32, decimal, float32, double, ENC_TV, EBV,
                                 GT, LT, GEQ, LEQ, EQ, NEQ)
import minmax_cases as mc

E18, HI5 = mc.E18, mc.HI5
ROWS = 1 << 20                                        # the smallest input that is streamed or run-copied at all
RUN_CHUNK = 4096                                      # kRunChunk: output rows per workgroup of run_copy_kernel; also one tile of the streamed form

# ---------------------------------------------------------------------------------------------------
# the typed-value table: minmax_cases' ids unchanged (1 .. 1000 the xsd:integer of the same value, then the edge values of the five
# numeric kinds, a plain string and a boolean), a few more ids that are not numeric, then 2^18 xsd:integer ids whose value is a simple
# function of the id (the layouts that need many ids)
# ---------------------------------------------------------------------------------------------------
BASE = len(mc.VALUES)
NON_NUMERIC = [("lang", abi.TV_STRING, 5, 1), ("iri", abi.TV_NAMED_NODE, 2, 0), ("str9", abi.TV_STRING, 9, 0)]   # (name, tag, lo, aux)
EXT0 = BASE + len(NON_NUMERIC)                        # the first computed id
N_EXT = 1 << 18
N_TABLE = EXT0 + N_EXT
BEYOND = N_TABLE                                      # an id the table does not hold: the error value
IDS = dict(mc.IDS)
for _k, (_name, _tag, _lo, _aux) in enumerate(NON_NUMERIC):
    IDS[_name] = BASE + _k
NOT_NUMERIC_IDS = [i for i in range(1, BASE) if mc.VALUES[i][0] not in mc.KINDS] + [BASE + k for k in range(len(NON_NUMERIC))]


def ext_value(i):
    """the value of computed id i (int or array): -500 .. 499, the sign changing with the id's parity, 0 at ids = 500 mod 1000"""
    i = np.asarray(i, np.int64)
    m = i % 1000
    return np.where(i % 2 == 0, m - 500, 500 - m)


def typed_table():
    tv = np.zeros(N_TABLE, dtype=TV_DTYPE)
    tv[:BASE] = mc.TV
    for k, (_, tag, lo, aux) in enumerate(NON_NUMERIC):
        tv["tag"][BASE + k], tv["lo"][BASE + k], tv["aux"][BASE + k] = tag, lo, aux
    tv["tag"][EXT0:] = abi.TV_INTEGER
    tv["lo"][EXT0:] = ext_value(np.arange(EXT0, N_TABLE))
    return tv, mc.DECIMALS


TV, DECIMALS = typed_table()


def value(i):
    """id -> (tag, payload) as minmax_cases takes it; mc.ERR for the null id and an id beyond the table; payload None where not numeric"""
    i = int(i)
    if i <= 0 or i >= N_TABLE:
        return mc.ERR
    if i < BASE:
        return mc.VALUES[i]
    if i < EXT0:
        return NON_NUMERIC[i - BASE][1], None
    return mc.INTEGER, int(ext_value(i))


# ---------------------------------------------------------------------------------------------------
# literals and operators
# ---------------------------------------------------------------------------------------------------
Lit = namedtuple("Lit", "name kind payload")
_LIT_TAG = {"integer": mc.INTEGER, "int32": mc.INT, "decimal": mc.DEC, "float32": mc.FLOAT, "double": mc.DOUBLE}
_LIT_EXPR = {"integer": integer, "int32": int32, "decimal": decimal, "float32": float32, "double": double}
# every one but the last two has ids below it, equal to it (i5, i0, g2^53 / nothing exact for the integer 2^53: i2^53+1 is above it as an
# integer and equal to it as a double, iMIN, iMAX, i7 / int7, id 990, dE18 / i1, dHI+1, f0.75, f2^24 / i2^24 / i2^24+1, g0.5) and above it
LITERALS = [
    Lit("integer 5", "integer", 5), Lit("integer 0", "integer", 0), Lit("integer 2^53", "integer", 2 ** 53),
    Lit("integer -2^63", "integer", -2 ** 63), Lit("integer 2^63-1", "integer", 2 ** 63 - 1),
    Lit("int 7", "int32", 7), Lit("int 990", "int32", 990),
    Lit("decimal 1.0", "decimal", E18), Lit("decimal HI5+1", "decimal", HI5 + 1),
    Lit("float 0.75", "float32", 0.75), Lit("float 2^24", "float32", 2.0 ** 24),
    Lit("double 0.5", "double", 0.5), Lit("double 2^53", "double", 2.0 ** 53),
    Lit("double 0.3", "double", 0.3),                 # equal to no id: EQ keeps nothing, NEQ every value that has an order
    Lit("double NaN", "double", math.nan),            # no order with any number: no numeric id is kept under any operator
]
LIT = {l.name: l for l in LITERALS}
OPS = {"GT": GT, "LT": LT, "GEQ": GEQ, "LEQ": LEQ, "EQ": EQ, "NEQ": NEQ}
TRUTH = {"GT": lambda o: o > 0, "LT": lambda o: o < 0, "GEQ": lambda o: o >= 0, "LEQ": lambda o: o <= 0, "EQ": lambda o: o == 0, "NEQ": lambda o: o != 0}


def lit_expr(lit):
    return _LIT_EXPR[lit.kind](lit.payload)


def lit_value(lit):
    return _LIT_TAG[lit.kind], lit.payload


def predicate(column, op, lit):
    """shape 2: the column on the left, the literal on the right"""
    return EBV(OPS[op](ENC_TV(col(column)), lit_expr(lit)))


# ---------------------------------------------------------------------------------------------------
# the per-id answer
# ---------------------------------------------------------------------------------------------------
_ORACLE = []


def oracle_store():
    """an OracleStore holding the typed table and no quads (the answers for ids that are not numeric, and what test_filter_cases_cpu.py
    holds this file to)"""
    if not _ORACLE:
        from oracle import oracle as orc
        os_ = orc.OracleStore()
        os_.set_typed_values(TV, DECIMALS)
        _ORACLE.append(os_)
    return _ORACLE[0]


@lru_cache(maxsize=None)
def _not_numeric_answers(op, lit_name):
    ids = np.asarray(NOT_NUMERIC_IDS, np.uint32)
    kept = oracle_store().eval_bool(predicate(0, op, LIT[lit_name]), [ids]) == 1
    return dict(zip(ids.tolist(), kept.tolist()))


def _numeric_verdict(v, op, lit):
    o = mc.partial_cmp(v, lit_value(lit))
    return o is not None and TRUTH[op](o)             # None: no order (a NaN), not kept under any of the six operators


def verdict(i, op, lit):
    """does FILTER(id `op` literal) keep a row that carries id i"""
    v = value(i)
    if v == mc.ERR:
        return False                                  # the null id, an unknown id
    if v[0] in mc.KINDS:
        return _numeric_verdict(v, op, lit)
    return bool(_not_numeric_answers(op, lit.name)[int(i)])


@lru_cache(maxsize=None)
def _verdict_table(op, lit_name):
    lit = LIT[lit_name]
    t = np.zeros(N_TABLE + 1, bool)                   # index N_TABLE: every id beyond the table
    t[:EXT0] = [verdict(i, op, lit) for i in range(EXT0)]
    per_value = np.array([_numeric_verdict((mc.INTEGER, v), op, lit) for v in range(-500, 500)])
    t[EXT0:N_TABLE] = per_value[ext_value(np.arange(EXT0, N_TABLE)) + 500]
    t.setflags(write=False)
    return t


def verdict_table(op, lit):
    """verdict for every id at once: entry i for id i < N_TABLE, entry N_TABLE (False) for every other id"""
    return _verdict_table(op, lit.name)


def keep_mask(ids, op, lit):
    return verdict_table(op, lit)[np.minimum(np.asarray(ids, np.uint32), N_TABLE)]


def expected(cols, pred_col, op, lit, projection):
    """the surviving rows in input order: (projected columns, row count)"""
    mask = keep_mask(cols[pred_col], op, lit)
    return [np.asarray(cols[c])[mask] for c in projection], int(mask.sum())


# ---------------------------------------------------------------------------------------------------
# layouts: the (subject, object) quads of one predicate partition in graph 0, distinct subjects, `head` quads of a smaller predicate in
# front of it in GPOS order, so that the slice's first row sits at 4-byte phase `head` of its 16-byte group
# ---------------------------------------------------------------------------------------------------
PRED_SMALL, PRED_BIG = N_TABLE + 2, N_TABLE + 3
SUBJECT0 = N_TABLE + 16
HEADS = (0, 1, 2, 3)
Layout = namedtuple("Layout", "name head ids counts")   # the runs in id order: ids ascending, counts > 0


def _layout(name, head, ids, counts):
    ids, counts = np.asarray(ids, np.int64), np.asarray(counts, np.int64)
    present = counts > 0
    ids, counts = ids[present], counts[present]
    assert np.all(np.diff(ids) > 0) and head in HEADS
    return Layout(name, head, ids.astype(np.uint32), counts)


def rows_of(layout):
    return int(layout.counts.sum())


def span_of(layout):
    return int(layout.ids[-1]) - int(layout.ids[0]) + 1


def columns(layout):
    """the partition's (s, o), in no particular order of the subjects"""
    n = rows_of(layout)
    o = np.repeat(layout.ids, layout.counts)
    s = (SUBJECT0 + np.random.default_rng(n + layout.head).permutation(n)).astype(np.uint32)
    return s, o


def store_quads(layout):
    """(g, s, p, o) of the whole store: the head quads and the partition"""
    s, o = columns(layout)
    h = layout.head
    s = np.concatenate([np.arange(1, h + 1, dtype=np.uint32), s])
    o = np.concatenate([np.full(h, 1, np.uint32), o])
    p = np.full(len(s), PRED_BIG, np.uint32)
    p[:h] = PRED_SMALL
    return np.zeros(len(s), np.uint32), s, p, o


def slice_rows(layout):
    """[s, o] of the pattern (?s, PRED_BIG, ?o) in graph 0 in index order: GPOS, by object, then subject"""
    s, o = columns(layout)
    order = np.lexsort((s, o))
    return [s[order], o[order]]


def slice_plan(op, lit, projection):
    pb = PlanBuilder()
    return pb.build(pb.filter(pb.data_source(quad_pattern("s", PRED_BIG, "o")), predicate(1, op, lit), projection=projection))


def with_one_more_id(layout):
    """the same partition and one quad that carries id max + 1"""
    return _layout(layout.name + "+1", layout.head, np.append(layout.ids, int(layout.ids[-1]) + 1), np.append(layout.counts, 1))


def _zero_sum_jitter(n, width):
    """n run length offsets in [-width, width] that total 0: the runs start at every phase"""
    d = (np.arange(n) * 5) % (2 * width + 1) - width
    d[-1] -= d.sum()
    return d


A_IDS = [i for i in range(1, EXT0) if value(i)[0] in mc.KINDS and not mc.is_nan(value(i))]
A_IDS = A_IDS[-64:]                                   # 15 small integers (986 .. 1000) and every edge value that has an order with any number


def long_runs(head):
    """A: 2^20 rows, 64 ids of the edge table (every numeric id but the NaNs: some literal keeps every row), every run about 16384 rows"""
    counts = ROWS // 64 + _zero_sum_jitter(64, 3)
    counts[-1] += ROWS - counts.sum()
    return _layout("long_runs", head, A_IDS, counts)


B_FIRST = EXT0 + 512 - 1024                           # span 1024 exactly: ids B_FIRST .. EXT0 + 511


def short_runs(head):
    """B: 2^20 rows, span 1024 (span * 1024 == rows, the inclusive bound of the run copy).  Ids B_FIRST .. 1000 (small integers): long runs,
    every tenth id absent, the first run exactly 4096 rows (an output that ends on a chunk boundary).  The edge ids, the NaNs and the ids
    that are not numeric among them: 2000 rows each.  512 computed ids: runs of 1, 2, 3, 4, 5 rows and absent ids in turn; their values
    change sign with every id, so under `> 0` every other run qualifies."""
    ids = np.arange(B_FIRST, EXT0 + 512)
    counts = np.zeros(1024, np.int64)
    small = ids <= 1000
    edge = (ids > 1000) & (ids < EXT0)
    ext = ids >= EXT0
    counts[edge] = 2000
    counts[ext] = np.resize([1, 2, 3, 4, 5, 0, 5, 1, 0, 0, 3], int(ext.sum()))
    counts[-1] = 2                                    # the last id of the span is there
    n_small = int(small.sum())
    there = (np.arange(n_small) % 10) != 9
    there[0] = True
    rest = ROWS - counts.sum() - RUN_CHUNK            # the first run has RUN_CHUNK rows, the other long runs share the rest
    n_long = int(there.sum()) - 1
    long_counts = rest // n_long + _zero_sum_jitter(n_long, 3)
    long_counts[-1] += rest - long_counts.sum()
    c_small = np.zeros(n_small, np.int64)
    c_small[0] = RUN_CHUNK
    c_small[np.flatnonzero(there)[1:]] = long_counts
    counts[small] = c_small
    assert counts.sum() == ROWS and counts[0] > 0 and counts[-1] > 0
    return _layout("short_runs", head, ids, counts)


def span_1025(head):
    """C: 1025 * 1024 rows over the 1025 computed ids from EXT0 on: span * 1024 == rows with two ids per lane of run_scan_kernel"""
    counts = 1024 + _zero_sum_jitter(1025, 3)
    return _layout("span_1025", head, np.arange(EXT0, EXT0 + 1025), counts)


D_LAST = 4400                                         # span 4400 = 68 * 64 + 48


def sparse_singles(head):
    """D: 2^20 rows over ids 1 .. 4400 (span % 64 == 48).  Single rows at ids 1, 34, .. 991 and at 1090, 1123, .. 4357 (33 apart: four
    neighbours touch four verdict words), every id of the edge table in between as a long run, one long run at the last id."""
    singles = np.concatenate([np.arange(1, 1000, 33), np.arange(1090, 4360, 33)])
    edge = np.arange(1001, EXT0)
    ids = np.concatenate([singles[singles < 1001], edge, singles[singles > 1001], [D_LAST]])
    counts = np.ones(len(ids), np.int64)
    long_ = np.isin(ids, edge) | (ids == D_LAST)
    n_long = int(long_.sum())
    rest = ROWS - int((~long_).sum())
    lc = rest // n_long + _zero_sum_jitter(n_long, 3)
    lc[-1] += rest - lc.sum()
    counts[long_] = lc
    return _layout("sparse_singles", head, ids, counts)


def wide_span(head):
    """E: 2^20 rows over all 2^18 computed ids (span * 4 == rows, the inclusive bound of the verdict bits): 7, 1, 4, 8, 0, 4, 3, 5 rows in turn"""
    return _layout("wide_span", head, np.arange(EXT0, N_TABLE), np.resize([7, 1, 4, 8, 0, 4, 3, 5], N_EXT))


def one_run(head):
    """F: 2^20 + 1 rows of the id i5 (span 1)"""
    return _layout("one_run", head, [IDS["i5"]], [ROWS + 1])


LAYOUTS = {"long_runs": long_runs, "short_runs": short_runs, "span_1025": span_1025, "sparse_singles": sparse_singles,
           "wide_span": wide_span, "one_run": one_run}

# the (operator, literal) pairs the GPU test runs over a layout; test_filter_cases_cpu.py holds layout_facts over them
A_KIND_LITERALS = ["integer 0", "int 990", "decimal 1.0", "float 0.75", "double 0.5"]      # each equal to an id of A
A_MORE_INTEGERS = ["integer 2^53", "integer -2^63", "integer 2^63-1"]
A_ENDS = [("EQ", "double 0.3"), ("NEQ", "double 0.3"), ("NEQ", "double NaN")]               # no survivor, every row, no survivor
B_CASES = [("GT", "integer 0"), ("LEQ", "integer 0"), ("NEQ", "double 0.5"), ("EQ", "double NaN"), ("GEQ", "decimal 1.0"), ("LT", "float 0.75")]
C_CASES = [("GT", "integer 0"), ("LEQ", "integer 0"), ("EQ", "integer 0"), ("NEQ", "double NaN"), ("GEQ", "integer -2^63")]
F_CASES = [("GT", "integer 5"), ("GEQ", "integer 5"), ("EQ", "double 0.5"), ("LEQ", "decimal HI5+1")]
D_CASES = [(op, name) for op in OPS for name in ("integer 0", "double 0.5")]
E_CASES = [("GT", "integer 0"), ("GEQ", "integer 0"), ("LT", "integer 0"), ("LEQ", "int 7"), ("EQ", "integer 0"), ("NEQ", "integer 0"), ("LEQ", "double 0.5")]
CASES = {"long_runs": [(op, name) for op in OPS for name in A_KIND_LITERALS + A_MORE_INTEGERS] + A_ENDS,
         "short_runs": B_CASES, "span_1025": C_CASES, "sparse_singles": D_CASES, "wide_span": E_CASES, "one_run": F_CASES}


def groups_of_three_words(layout):
    """how many 16-byte groups of the slice's sorted column hold ids of three or more 32-id verdict words (row r of the slice sits at
    phase (head + r) % 4)"""
    o = np.repeat(layout.ids, layout.counts).astype(np.int64)
    first = (-layout.head) % 4
    n = (len(o) - first) // 4
    w = ((o[first:first + 4 * n] - int(layout.ids[0])) >> 5).reshape(n, 4)
    return int(((np.diff(w, axis=1) != 0).sum(axis=1) >= 2).sum())


def places_33_apart(layout):
    """how many times four consecutive rows of the slice carry ids at least 33 apart from each other"""
    o = np.repeat(layout.ids, layout.counts).astype(np.int64)
    far = np.diff(o) >= 33
    return int((far[:-2] & far[1:-1] & far[2:]).sum())


def layout_facts(layout, op, lit):
    """what a case holds, from the reference alone"""
    q = verdict_table(op, lit)[np.minimum(layout.ids, N_TABLE)]
    cnt = layout.counts[q]
    end = np.cumsum(cnt)
    off = end - cnt                                   # where each qualifying run's output starts
    inner = end[:-1]                                  # (the last run ends where the output ends)
    return {
        "rows": rows_of(layout), "survivors": int(cnt.sum()), "span": span_of(layout),
        "qualifying_runs": int(q.sum()),
        "alternations": int((q[1:] != q[:-1]).sum()),                       # neighbours in the slice of which one qualifies
        "start_phases": set((off % 4).tolist()),
        "short_qualifying_runs": int((cnt <= 5).sum()),
        "ends_on_chunk": bool(np.any(inner % RUN_CHUNK == 0)),
        "crosses_chunk": bool(np.any(off // RUN_CHUNK != (end - 1) // RUN_CHUNK)),
        "absent_ids": span_of(layout) - len(layout.ids),
        "groups_of_three_words": groups_of_three_words(layout), "places_33_apart": places_33_apart(layout),
        "last_id_kept": bool(q[-1]),
    }


# ---------------------------------------------------------------------------------------------------
# bound tables
# ---------------------------------------------------------------------------------------------------
def every_id_table(n=4097, seed=3):
    """(ids, payload): every id below EXT0 + 64 (the null id among them) and the id beyond the table, shuffled; payload = row number + 1"""
    pool = np.concatenate([np.arange(EXT0 + 64), [BEYOND]]).astype(np.uint32)
    ids = np.resize(pool, n)
    np.random.default_rng(seed).shuffle(ids)
    return [ids, np.arange(1, n + 1, dtype=np.uint32)]


def unsorted_table(n, seed=11):
    """(ids, payload, second payload) for the streamed form over a bound table: ids of the whole small part of the table, unsorted, the
    null id and the id beyond the table among them"""
    rng = np.random.default_rng(seed + n)
    pool = np.concatenate([np.arange(EXT0 + 64), [BEYOND]]).astype(np.uint32)
    ids = pool[rng.integers(0, len(pool), n)]
    return [ids, np.arange(1, n + 1, dtype=np.uint32), rng.integers(1, 1 << 30, n).astype(np.uint32)]


PATTERN_IDS = {"first": 11, "last": 12, "tile": 13, "other": 14, "nowhere": 15}


def pattern_column(n, skip, tile=129):
    """n ids for the survivor patterns of a streamed filter whose column starts `skip` words into a 16-byte group: PATTERN_IDS["first"] in
    the first row, ["last"] in the last, ["tile"] in every row of the 4096-row tile `tile` (tiles count from the group's start: its
    neighbours hold no such row), ["other"] elsewhere"""
    ids = np.full(n, PATTERN_IDS["other"], np.uint32)
    t = (np.arange(n) + skip) // RUN_CHUNK
    ids[t == tile] = PATTERN_IDS["tile"]
    ids[0], ids[-1] = PATTERN_IDS["first"], PATTERN_IDS["last"]
    return ids
