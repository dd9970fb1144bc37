"""SUM / AVG accumulators at their limb, run, form and tile edges: one typed-value table, the total cases with their results worked by
hand, the run layout, the group counts on either side of the LDS / HBM switch and the expectation, shared by
test_aggregate_edges_cpu.py (the hand-written results = the restatement of test_aggregate_cpu.py, on a machine without a GPU) and
test_gpu_aggregate_edges.py (the device = the restatement).

Geometry (aggregate.hip): SUM and AVG add the two (integer) or four (decimal) 32-bit limbs of every value into u64 words and count the
negative values; agg_final_kernel rebuilds the total in 256 bits and decides whether it fits i64 / i128.  Rows of a 64-lane wave that are
neighbours in one group are summed in the wave first (runs).  The words live in LDS while n_words * groups * 8 <= 65536 bytes.  The
group pass walks 1024-row tiles, at most 16384 workgroups; the accumulate pass 256 rows per workgroup, at most 512 (LDS) or 16384 (HBM)
workgroups."""
from collections import defaultdict, namedtuple
from fractions import Fraction

import numpy as np

from rdf_fusion_amd import abi
from rdf_fusion_amd.engine import TV_DTYPE
from rdf_fusion_amd.plan import PlanBuilder, col, lit_id, integer, ID_EQ, ADD, ENC_TV
from test_aggregate_cpu import sum_agg, avg_agg, count_agg, count_distinct_agg

E18 = 10 ** 18
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I128_MIN, I128_MAX = -(1 << 127), (1 << 127) - 1
STAR, COUNT, DISTINCT, SUM, AVG = abi.AGG_COUNT_STAR, abi.AGG_COUNT, abi.AGG_COUNT_DISTINCT, abi.AGG_SUM, abi.AGG_AVG

# ---------------------------------------------------------------------------------------------------
# the typed-value table
# ---------------------------------------------------------------------------------------------------
N_SMALL = 1000                                   # ids 1 .. 1000 are the xsd:integer of the same value (fillers, the strides' values)
INT_TOP = I128_MAX // E18                        # 170141183460469231731: the largest integer total that is still a decimal
TOP_FILL = INT_TOP - 18 * I64_MAX                # 4120486797083267205: 18 x I64_MAX and this one total INT_TOP
TOP_REST = I128_MAX - INT_TOP * E18              # 687303715884105727: INT_TOP x 10^18 and this decimal total I128_MAX
NAMED = [
    ("i0", abi.TV_INTEGER, 0), ("i-1", abi.TV_INTEGER, -1), ("i2^32-1", abi.TV_INTEGER, 2 ** 32 - 1), ("i2^32", abi.TV_INTEGER, 2 ** 32),
    ("i2^62", abi.TV_INTEGER, 2 ** 62), ("i-2^62", abi.TV_INTEGER, -2 ** 62), ("i2^62-1", abi.TV_INTEGER, 2 ** 62 - 1),
    ("iMAX", abi.TV_INTEGER, I64_MAX), ("iMIN", abi.TV_INTEGER, I64_MIN), ("iFILL", abi.TV_INTEGER, TOP_FILL),
    ("int-1", abi.TV_INT, -1), ("int2^31-1", abi.TV_INT, 2 ** 31 - 1), ("int-2^31", abi.TV_INT, -2 ** 31),
    ("d0", abi.TV_DECIMAL, 0), ("d1", abi.TV_DECIMAL, 1), ("d-1", abi.TV_DECIMAL, -1), ("d2^32-1", abi.TV_DECIMAL, 2 ** 32 - 1),
    ("d2^64-1", abi.TV_DECIMAL, 2 ** 64 - 1), ("d2^96-1", abi.TV_DECIMAL, 2 ** 96 - 1), ("dE18", abi.TV_DECIMAL, E18), ("d-E18", abi.TV_DECIMAL, -E18),
    ("dMAX", abi.TV_DECIMAL, I128_MAX), ("dMIN", abi.TV_DECIMAL, I128_MIN), ("dREST", abi.TV_DECIMAL, TOP_REST), ("dREST+1", abi.TV_DECIMAL, TOP_REST + 1),
    ("f0.75", abi.TV_FLOAT, 0.75), ("g0.5", abi.TV_DOUBLE, 0.5), ("str", abi.TV_STRING, 5),
]


def typed_table():
    """-> (tv, decimals, ids by name, values): `values[i]` is id i as the restatement takes it, (tag, payload); id 0 is unbound"""
    tv = np.zeros(1 + N_SMALL + len(NAMED), dtype=TV_DTYPE)
    values = [(abi.TV_NULL, None)]
    tv["tag"][1:N_SMALL + 1] = abi.TV_INTEGER
    tv["lo"][1:N_SMALL + 1] = np.arange(1, N_SMALL + 1)
    values += [(abi.TV_INTEGER, v) for v in range(1, N_SMALL + 1)]
    ids, dec = {"unbound": 0, "i1": 1, "i3": 3, "i5": 5}, []
    for i, (name, tag, v) in enumerate(NAMED, start=N_SMALL + 1):
        ids[name] = i
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
        values.append((tag, v))
    return tv, np.array(dec, dtype=np.uint64).astype(np.int64).reshape(-1, 2), ids, values


TV, DECIMALS, IDS, VALUES = typed_table()


def val(i):
    return VALUES[i] if 0 < i < len(VALUES) else (abi.TV_NULL, None)


# ---------------------------------------------------------------------------------------------------
# the total cases: SUM and AVG worked by hand.  int = an xsd:integer, Fraction = an xsd:decimal, float = an xsd:float / xsd:double (the
# exact value: the inputs are dyadic and few), None = the error value.
# AVG is Decimal::checked_div(total, count): the dividend is scaled by 10 while it stays in i128, so a quotient keeps 18 fractional digits,
# truncated toward zero, unless the total is so large that it cannot be scaled at all (then it keeps what the two divisions leave).
# ---------------------------------------------------------------------------------------------------
TotalCase = namedtuple("TotalCase", "name ids sum avg")
D = lambda raw: Fraction(raw, E18)


def _total_cases():
    n = IDS
    MAX, MIN, one, five = n["iMAX"], n["iMIN"], n["i1"], n["i5"]
    top = [MAX] * 18 + [n["iFILL"]]                                # integers totalling INT_TOP
    C = TotalCase
    out = [
        # integer fit
        C("int-max", [MAX], 9223372036854775807, Fraction(9223372036854775807)),
        C("int-max+1", [MAX, one], None, Fraction(4611686018427387904)),                                       # 2^63 / 2
        C("int-max+1-1", [MAX, one, n["i-1"]], 9223372036854775807, D(3074457345618258602333333333333333333)),   # the total decides; MAX / 3
        C("int-min", [MIN], -9223372036854775808, Fraction(-9223372036854775808)),
        C("int-min-1", [MIN, n["i-1"]], None, Fraction(-9223372036854775809, 2)),
        C("int-min+max", [MIN, MAX], -1, Fraction(-1, 2)),
        C("int-2^62+2^62-1", [n["i2^62"], n["i2^62-1"]], 9223372036854775807, Fraction(9223372036854775807, 2)),
        C("int-2^62+2^62", [n["i2^62"], n["i2^62"]], None, Fraction(4611686018427387904)),
        C("int--2^62-2^62", [n["i-2^62"], n["i-2^62"]], -9223372036854775808, Fraction(-4611686018427387904)),
        C("int--2^62-2^62-1", [n["i-2^62"], n["i-2^62"], n["i-1"]], None, Fraction(-3074457345618258603)),      # -(2^63 + 1) / 3, exact
        C("int-zero-total", [MIN, MAX, one, n["i0"]], 0, Fraction(0)),
        C("xsd-int", [n["int-1"], n["int2^31-1"], n["int-2^31"]], -2, D(-666666666666666666)),                  # -2 / 3 truncated toward zero
        # AVG of integers past i64
        C("avg-18-max", [MAX] * 18, None, Fraction(9223372036854775807)),
        C("avg-19-max", [MAX] * 19, None, None),
        # 170141183460469231731 = 19 * 8954799129498380617 + 8, and 8 / 19 = 0.421052631578947368 421..
        C("avg-int-top", top, None, D(8954799129498380617421052631578947368)),
        C("avg-int-top+1", top + [one], None, None),
        # decimal fit
        C("dec-max", [n["dMAX"]], D(170141183460469231731687303715884105727), D(170141183460469231731687303715884105727)),
        C("dec-max+1", [n["dMAX"], n["d1"]], None, None),
        C("dec-max+1-1", [n["dMAX"], n["d1"], n["d-1"]], D(170141183460469231731687303715884105727), D(56713727820156410577229101238628035242)),
        C("dec-min", [n["dMIN"]], D(-170141183460469231731687303715884105728), D(-170141183460469231731687303715884105728)),
        C("dec-min-1", [n["dMIN"], n["d-1"]], None, None),
        C("dec-min+max", [n["dMIN"], n["dMAX"]], D(-1), D(0)),                                                 # -10^-18 / 2 truncates to 0
        C("dec-max+max", [n["dMAX"], n["dMAX"]], None, None),
        C("dec-min+min", [n["dMIN"], n["dMIN"]], None, None),
        C("dec-257-max", [n["dMAX"]] * 257, None, None),                                                       # a total of 136 bits
        C("dec-257-min", [n["dMIN"]] * 257, None, None),
        # 10^-18 scales by 10^38; the count 10 strips one zero more: a scale of 10^39 is the error value (decimal.rs:154-158)
        C("dec-count-10", [n["d1"]] + [n["d0"]] * 9, D(1), None),
        # mixed: integers x 10^18 + decimals
        C("mixed-max", top + [n["dREST"]], D(170141183460469231731687303715884105727), D(8507059173023461586584365185794205286)),   # (MAX / 2) / 10
        C("mixed-max+1", top + [n["dREST+1"]], None, None),
        # fits only because I * 10^18 + D cancels: (INT_TOP + 1) * 10^18 is past i128, -1.0 brings it back; 170141183460469231731 = 21 * 8101961117165201511
        C("mixed-cancels", top + [one, n["d-E18"]], Fraction(170141183460469231731), Fraction(8101961117165201511)),
        # limb carries: 257 rows each
        C("limb-int-2^32-1", [n["i2^32-1"]] * 257, 1103806594815, Fraction(4294967295)),
        C("limb-int-2^32", [n["i2^32"]] * 257, 1103806595072, Fraction(4294967296)),
        C("limb-dec-2^32-1", [n["d2^32-1"]] * 257, D(1103806594815), D(4294967295)),
        C("limb-dec-2^64-1", [n["d2^64-1"]] * 257, D(4740813226943354765055), D(18446744073709551615)),
        C("limb-dec-2^96-1", [n["d2^96-1"]] * 257, D(20361637766165934761540795236095), D(79228162514264337593543950335)),
        C("limb-dec--1", [n["d-1"]] * 257, D(-257), D(-1)),
        C("limb-int--1", [n["i-1"]] * 257, -257, Fraction(-1)),
        # cancelling: limb sums near 2^47, 20000 negatives; 19995 * 10^18 = 40001 * 499862503437414064 + 25936
        C("cancelling", [MAX, MIN] * 20000 + [five], -19995, D(-499862503437414064)),
        # typing
        C("unbound-among-integers", [five, 0, one], 6, None),
        C("string-among-integers", [five, n["str"], one], 6, None),
        C("float-wins", [n["f0.75"], one], 1.75, 0.875),
        C("double-wins", [n["g0.5"], one, n["dE18"]], 2.5, 2.5 / 3),
    ]
    return out


TOTAL_CASES = _total_cases()
KEEP_ID, DROP_ID = 7, 11


def python_value(result):
    """(tag, payload | Approx) of the restatement as the hand-written results are given: int, Fraction, float or None"""
    tag, payload = result
    if tag == abi.TV_NULL:
        return None
    if tag == abi.TV_INTEGER:
        return int(payload)
    if tag == abi.TV_DECIMAL:
        return Fraction(payload, E18)
    return payload.exact() / payload.divisor


def literal_result(v):
    """a hand-written result as same() of test_aggregate_cpu.py takes an expectation; a float result has no such form (None)"""
    if v is None:
        return abi.TV_NULL, None
    if isinstance(v, int):
        return abi.TV_INTEGER, v
    if isinstance(v, Fraction):
        raw = v * E18
        assert raw.denominator == 1
        return abi.TV_DECIMAL, int(raw)
    return None


def totals_table(order):
    """(group, value) columns with one group per total case (group id = the case's index: id 0 is a group like any other).
    order: "sorted" by group; "shuffled"; "filtered": a third column of KEEP_ID / DROP_ID, the shuffled rows interleaved with and followed
    by rows a FilterExec is to drop - they carry the cases' groups and I64_MAX / I128_MAX, so one of them counted shows"""
    key = np.concatenate([np.full(len(c.ids), g, np.uint32) for g, c in enumerate(TOTAL_CASES)])
    value = np.concatenate([np.asarray(c.ids, np.uint32) for c in TOTAL_CASES])
    if order == "sorted":
        return [key, value]
    rng = np.random.default_rng(21)
    perm = rng.permutation(len(key))
    key, value = key[perm], value[perm]
    if order == "shuffled":
        return [key, value]
    assert order == "filtered"
    n, extra = len(key), 1000
    drop = rng.random(n) < 0.3                                      # a dropped row before about every third live one
    at = np.arange(n) + np.cumsum(drop)                             # where the live rows go
    total = n + int(drop.sum()) + extra
    k = rng.integers(0, len(TOTAL_CASES), total).astype(np.uint32)
    v = rng.choice([IDS["iMAX"], IDS["dMAX"]], total).astype(np.uint32)
    flag = np.full(total, DROP_ID, np.uint32)
    k[at], v[at], flag[at] = key, value, KEEP_ID
    return [k, v, flag]


def expression_input(c):
    """the column as an expression of the same value: ADD(ENC_TV(col), integer 0)"""
    return ADD(ENC_TV(col(c)), integer(0))


def aggregate_plan(n_cols, keys, aggs, filtered=False):
    """AggregateExec over bound table 0; filtered: over FilterExec(last column = KEEP_ID), which projects that column away"""
    pb = PlanBuilder()
    t = pb.table(0, n_cols)
    if filtered:
        t = pb.filter(t, ID_EQ(col(n_cols - 1), lit_id(KEEP_ID)), projection=list(range(n_cols - 1)))
    return pb.build(pb.aggregate(t, keys, aggs))


# ---------------------------------------------------------------------------------------------------
# runs of equal neighbouring groups
# ---------------------------------------------------------------------------------------------------
RUN_LENGTHS = (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
RUN_GROUPS = 12
RUN_SEED = 1
INT_CYCLE = ("iMAX", "iMIN", "i-1", "i2^32-1")
DEC_CYCLE = ("dMAX", "dMIN", "d-1", "d2^96-1")
FLOAT_CYCLE = ("f0.75", "i-1", "f0.75", "i3")                   # small values, a float among them: a float total wherever a group holds one


def run_starts(keys):
    """row numbers at which a run of equal neighbouring keys starts, and the row count as the last entry"""
    keys = np.asarray(keys)
    return np.concatenate([[0], np.flatnonzero(keys[1:] != keys[:-1]) + 1, [len(keys)]])


def run_layout(seed=RUN_SEED):
    """A key column as a concatenation of runs: 400 runs with lengths drawn from RUN_LENGTHS, 130 runs of one row in their middle (a wave of
    heads only takes the path without the shuffle reduction), groups drawn from RUN_GROUPS ids (never the neighbour's: each group returns in
    many separate runs).  Asserts what the layout is for."""
    rng = np.random.default_rng(seed)
    lengths = rng.choice(RUN_LENGTHS, 400).tolist()
    lengths[200:200] = [1] * 130
    groups = []
    for _ in lengths:
        g = int(rng.integers(0, RUN_GROUPS))
        while groups and g == groups[-1]:
            g = int(rng.integers(0, RUN_GROUPS))
        groups.append(g)
    keys = np.repeat(np.asarray(groups, np.uint32) * 5 + 2, lengths)
    check_run_layout(keys)
    return keys


def check_run_layout(keys):
    st = run_starts(keys)
    n, first, last = int(st[-1]), st[:-1], st[1:] - 1                # each run's first and last row
    assert n % 64 != 0, "the last run ends where a wave ends"
    assert set((first % 64).tolist()) == set(range(64)), "no run starts at some lane"
    assert (first // 64 != last // 64).any(), "no run crosses a wave boundary"
    assert (first // 256 != last // 256).any(), "no run crosses a workgroup boundary"
    assert set((last - first + 1).tolist()) == set(RUN_LENGTHS), "a run length is missing"
    is_start = np.zeros(n + 1, bool)
    is_start[st] = True
    heads_only = [w for w in range(n // 64) if is_start[w * 64:(w + 1) * 64 + 1].all()]
    assert heads_only, "no wave holds only runs of one row"
    per_group = defaultdict(int)
    for g in keys[first].tolist():
        per_group[g] += 1
    assert len(per_group) == RUN_GROUPS and min(per_group.values()) >= 5, "a group does not return in separate runs"


def cycle_column(names, n):
    return np.resize(np.asarray([IDS[x] for x in names], np.uint32), n)


def run_table(seed=RUN_SEED):
    """(group, integer, decimal, float): the run layout's keys, the value columns cycling by row number"""
    keys = run_layout(seed)
    return [keys] + [cycle_column(c, len(keys)) for c in (INT_CYCLE, DEC_CYCLE, FLOAT_CYCLE)]


RUN_AGGS = [(STAR, None), (SUM, 1), (AVG, 1), (SUM, 2), (DISTINCT, 1), (SUM, 3)]

# ---------------------------------------------------------------------------------------------------
# the LDS / HBM switch
# ---------------------------------------------------------------------------------------------------
LDS_BYTES, SUM_WORDS = 65536, 11                                  # kAggLdsBytes, kAggSumWords (kernels.hpp)


def n_words(aggs):
    """accumulator words per group: the row count, 11 per SUM / AVG, 1 per COUNT / COUNT DISTINCT"""
    return 1 + sum(0 if fn == STAR else SUM_WORDS if fn in (SUM, AVG) else 1 for fn, _ in aggs)


def form_edges():
    """[(aggregates over (group, value), the largest group count whose words fit LDS, the smallest that does not)]"""
    out = []
    for aggs in ([(STAR, None)], [(STAR, None), (SUM, 1)], [(SUM, 1), (AVG, 1)]):
        fit = LDS_BYTES // (8 * n_words(aggs))
        out.append((aggs, fit, fit + 1))
    return out


LIMB_SET = ("i2^32-1", "d2^64-1", "d2^96-1", "d-1", "i-1")


def form_table(groups):
    """(group, value): three rows per group, shuffled; group g holds LIMB_SET[g], [g + 1] and [g + 3] (indices modulo 5)"""
    ids = [IDS[x] for x in LIMB_SET]
    key = np.repeat(np.arange(groups, dtype=np.uint32), 3)
    value = np.asarray([ids[(g + j) % 5] for g in range(groups) for j in (0, 1, 3)], np.uint32)
    perm = np.random.default_rng(groups).permutation(len(key))
    return [key[perm], value[perm]]


# ---------------------------------------------------------------------------------------------------
# the group pass: every row a group of its own
# ---------------------------------------------------------------------------------------------------
GROUP_ROWS = (1023, 1024, 1025, 4097)
GROUP_KEYS = (1, 2, 4)


def distinct_tuples(rows, n_keys):
    """`rows` distinct key tuples as n_keys columns, and a value column.  The ids come from the smallest pool [0, 0xFFFFFFFF, 1, 2, ..]
    whose tuples suffice, so with several columns the table holds tuples that differ in their last column only and tuples that are
    permutations of each other; a seeded choice among all tuples of the pool, in a seeded order."""
    m = 2
    while m ** n_keys < rows:
        m += 1
    pool = np.asarray([0, 0xFFFFFFFF] + list(range(1, m - 1)), np.uint32)
    pick = np.random.default_rng(rows * 10 + n_keys).permutation(m ** n_keys)[:rows]
    cols = [pool[(pick // m ** (n_keys - 1 - q)) % m] for q in range(n_keys)]
    tuples = set(zip(*[c.tolist() for c in cols]))
    assert len(tuples) == rows
    assert any(0 in t for t in tuples) and any(0xFFFFFFFF in t for t in tuples)
    if n_keys > 1:
        assert any(t[:-1] + (x,) in tuples for t in tuples for x in pool.tolist() if x != t[-1]), "no two tuples differ in the last column only"
        assert any(t[::-1] in tuples for t in tuples if t[::-1] != t), "no tuple is a permutation of another"
    return cols + [cycle_column(INT_CYCLE + ("d2^64-1", "i2^32"), rows)]


# ---------------------------------------------------------------------------------------------------
# the strides: a workgroup's second trip through its loop
# ---------------------------------------------------------------------------------------------------
GROUP_TILE, GROUP_GRID = 1024, 16384                              # agg_groups_kernel: rows per tile, the launcher's cap on workgroups
ACCUM_BLOCK, ACCUM_LDS_GRID, ACCUM_HBM_GRID = 256, 512, 16384     # agg_accum_kernel: rows per sweep and workgroup, the caps of its two forms
# tile 16384 exists and is partial; so is the HBM form's second sweep (its first covers 16384 x 256 = 2^22 rows: this is its fifth)
BIG_ROWS, BIG_GROUPS = GROUP_TILE * GROUP_GRID + 1500, 1000      # (COUNT(*) and SUM over 1000 groups: 96000 bytes of words, the HBM form)
BIG_GROUPS_LDS = 600                                              # .. over 600 groups: 57600 bytes, the LDS form, 33 sweeps per workgroup
# the LDS form's second sweep, partial and ending in mid-wave
SWEEP_ROWS, SWEEP_GROUPS = ACCUM_BLOCK * ACCUM_LDS_GRID + 257, 64


def big_table(groups=BIG_GROUPS):
    """(group, value): BIG_ROWS rows in `groups` groups, value id v = the integer v in 1 .. 1000"""
    rng = np.random.default_rng(16384)
    return [(rng.integers(0, groups, BIG_ROWS) * 7 + 3).astype(np.uint32), rng.integers(1, N_SMALL + 1, BIG_ROWS).astype(np.uint32)]


def sweep_table():
    """(group, integer): SWEEP_ROWS rows with the integer cycle of the run table.  Every four rows (one turn of the cycle: I64_MAX + I64_MIN
    - 1 + 2^32 - 1) go to one of SWEEP_GROUPS groups drawn at random, so a group's total fits i64 while its limb sums pass 2^40 and
    its negatives run into the hundreds; the one row left over (I64_MAX) takes its group past i64."""
    rng = np.random.default_rng(512)
    key = np.repeat(rng.integers(0, SWEEP_GROUPS, SWEEP_ROWS // 4 + 1), 4)[:SWEEP_ROWS].astype(np.uint32)
    return [key, cycle_column(INT_CYCLE, SWEEP_ROWS)]


# ---------------------------------------------------------------------------------------------------
# the expectation
# ---------------------------------------------------------------------------------------------------
def expected(cols, keys, aggs, value=val):
    """{key tuple: [(tag, payload | Approx) per aggregate]} by the restatement of test_aggregate_cpu.py over host columns"""
    kc = [np.asarray(cols[k]).tolist() for k in keys]
    vc = {c: np.asarray(cols[c]).tolist() for _, c in aggs if c is not None}
    rows = defaultdict(list)
    for r in range(len(cols[0])):
        rows[tuple(c[r] for c in kc)].append(r)
    out = {}
    for key, members in rows.items():
        res = []
        for fn, c in aggs:
            ids = [vc[c][r] for r in members] if c is not None else []
            if fn == STAR:
                res.append((abi.TV_INTEGER, len(members)))
            elif fn == COUNT:
                res.append(count_agg(ids))
            elif fn == DISTINCT:
                res.append(count_distinct_agg(ids))
            elif fn == SUM:
                res.append(sum_agg([value(i) for i in ids]))
            else:
                res.append(avg_agg([value(i) for i in ids]))
        out[key] = res
    return out
