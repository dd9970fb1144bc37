"""Aggregate values as columns (abi.PLAN_AGG_COLUMNS): the tables and a Python reference for plans that continue above an AggregateExec —
HAVING, joins of aggregates, a cross join with a global aggregate, aggregates over aggregates — shared by test_agg_columns_cpu.py and
test_gpu_agg_columns.py.

The reference is built from what the suite already has: an aggregate's value per group is sum_agg / avg_agg / count_agg of
test_aggregate_cpu.py, arithmetic in a predicate is numeric_ref.binary, over the typed-value table of agg_cases.py (ids 1 .. 1000 are the
xsd:integer of the same value, the named ids its edge values).  A relation is a list of rows; a cell is an object id (int) or, in a value
column, the value itself as (tag, payload) — UNBOUND where the aggregate was the error value or a LEFT join padded the row.

Values that a predicate compares are int / integer / decimal (or small dyadic floats): their comparison after the reference's promotion
equals the comparison of the exact rationals, which is what `compare` does, and no verdict depends on a summation order.  Float and double
aggregates are only carried and compared with same() / Approx."""
from collections import defaultdict
from fractions import Fraction

import numpy as np

from rdf_fusion_amd import abi
import agg_cases as ac
import numeric_ref as nr
from test_aggregate_cpu import sum_agg, avg_agg, count_agg, same

E18 = 10 ** 18
STAR, COUNT, DISTINCT, SUM, AVG = abi.AGG_COUNT_STAR, abi.AGG_COUNT, abi.AGG_COUNT_DISTINCT, abi.AGG_SUM, abi.AGG_AVG
UNBOUND = (abi.TV_NULL, None)
val = ac.val                                  # object id -> (tag, payload); id 0 and ids beyond the table are unbound
IDS = ac.IDS


# ---------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------
def rows_of(cols):
    return list(zip(*[np.asarray(c).tolist() for c in cols]))


def tv(cell):
    """ENC_TV of a cell: the typed value of an object id, or a value column's value"""
    return val(cell) if isinstance(cell, int) else cell


def bound(cell):
    return cell != 0 if isinstance(cell, int) else cell[0] != abi.TV_NULL


def exact(v):
    """a numeric value as the exact rational (None: not numeric, the error value)"""
    t, p = v
    if t in (abi.TV_INT, abi.TV_INTEGER):
        return Fraction(p)
    if t == abi.TV_DECIMAL:
        return Fraction(p, E18)
    if t in (abi.TV_FLOAT, abi.TV_DOUBLE):
        return Fraction(float(p))
    return None


def compare(op, a, b):
    """EBV(op(a, b)) for numeric operands: True / False, None = the error value (the row is dropped)"""
    x, y = exact(a), exact(b)
    if x is None or y is None:
        return None
    return {"gt": x > y, "geq": x >= y, "lt": x < y, "leq": x <= y, "eq": x == y}[op]


def mul(a, b):
    return nr.binary(abi.EX_MUL, a, b)


def aggregate(rows, keys, aggs):
    """AggregateExec: aggs = [(fn, input)], input = None (COUNT(*)), a column, or a function row -> value (an input expression).
    -> rows of the key ids followed by one value cell per aggregate; zero keys: one row, even over no rows."""
    groups = defaultdict(list)
    for r in rows:
        groups[tuple(r[k] for k in keys)].append(r)
    if not keys and not groups:
        groups[()] = []
    out = []
    for key, members in groups.items():
        cells = []
        for fn, c in aggs:
            if fn == STAR:
                res = (abi.TV_INTEGER, len(members))
            elif fn == COUNT:
                res = (abi.TV_INTEGER, sum(1 for r in members if bound(r[c])))
            else:
                values = [c(r) if callable(c) else tv(r[c]) for r in members]
                res = sum_agg(values) if fn == SUM else avg_agg(values)
            cells.append(UNBOUND if res[0] == abi.TV_NULL else res)
        out.append(key + tuple(cells))
    return out


def having(rows, pred, projection=None):
    """FilterExec: rows whose predicate is exactly True"""
    kept = [r for r in rows if pred(r) is True]
    return kept if projection is None else [tuple(r[c] for c in projection) for r in kept]


def join(left, right, on, join_type=abi.JOIN_INNER, pred=None, right_width=None):
    """HashJoinExec (on) / NestedLoopJoinExec / CrossJoinExec (on = []): NullEqualsNothing keys, the filter part of the match"""
    out = []
    for l in left:
        matches = [r for r in right if all(l[a] != 0 and l[a] == r[b] for a, b in on) and (pred is None or pred(l + r) is True)]
        if join_type == abi.JOIN_LEFT_SEMI:
            out += [l] if matches else []
        elif join_type == abi.JOIN_LEFT_ANTI:
            out += [] if matches else [l]
        else:
            out += [l + r for r in matches]
            if join_type == abi.JOIN_LEFT and not matches:
                out.append(l + tuple([0] * right_width))    # padding: id 0 in an id column, entry 0 = unbound in a value column
    return out


# ---------------------------------------------------------------------------------------------------
# device rows against reference rows
# ---------------------------------------------------------------------------------------------------
def device_rows(plan):
    """the executed result as rows: ids, and (tag, lo, hi) in the value columns; an entry of 0 must be the null value and nothing else"""
    n, c = plan.result_info()
    ids = plan.fetch()
    vcols = plan.value_columns()
    values = {q: plan.fetch_column_values(q) for q in vcols}
    for q in vcols:
        assert np.array_equal(ids[q] == 0, values[q]["tag"] == 0), f"column {q}: entry 0 and the null value do not coincide"
    rows = []
    for r in range(n):
        rows.append(tuple((int(values[q]["tag"][r]), int(values[q]["lo"][r]), int(values[q]["hi"][r])) if q in values else int(ids[q][r])
                          for q in range(c)))
    return rows, vcols


def cell_matches(expected, got):
    if isinstance(got, tuple):                      # a value column: a padded row of the reference carries 0 in every padded column
        return (expected == 0 and got[0] == abi.TV_NULL) if isinstance(expected, int) else same(expected, got)
    return isinstance(expected, int) and expected == got


def check_rows(expected, plan, value_cols):
    """the device's rows are the reference's, as multisets; `value_cols`: which result columns must be value columns"""
    got, vcols = device_rows(plan)
    assert vcols == list(value_cols), (vcols, value_cols)
    assert len(got) == len(expected), (len(got), len(expected))
    id_cols = [q for q in range(len(got[0])) if q not in vcols] if got else []
    by_key = defaultdict(list)
    for g in got:
        by_key[tuple(g[q] for q in id_cols)].append(g)
    for e in expected:
        cands = by_key[tuple(e[q] for q in id_cols)]
        hit = next((i for i, g in enumerate(cands) if all(cell_matches(x, y) for x, y in zip(e, g))), None)
        assert hit is not None, (e, cands[:4])
        cands.pop(hit)


# ---------------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------------
def sized_groups(groups, seed=3):
    """(group, x, y): group g (id g * 3 + 1) has g % 5 + 1 rows, shuffled; x, y are small xsd:integer ids"""
    key = np.repeat(np.arange(groups, dtype=np.uint32) * 3 + 1, np.arange(groups) % 5 + 1)
    rng = np.random.default_rng(seed + groups)
    perm = rng.permutation(len(key))
    return [key[perm], rng.integers(1, 40, len(key)).astype(np.uint32), rng.integers(1, 40, len(key)).astype(np.uint32)]


def review_table(reviewers=300, seed=8):
    """(reviewer, rating): 1 to 5 ratings each, ids 1 .. 10 = the xsd:integer ratings; one rating in fifty is unbound"""
    rng = np.random.default_rng(seed)
    n = rng.integers(1, 6, reviewers)
    who = np.repeat(np.arange(reviewers, dtype=np.uint32) + 2000, n)
    rating = rng.integers(1, 11, len(who)).astype(np.uint32)
    rating[rng.random(len(who)) < 0.02] = 0
    perm = rng.permutation(len(who))
    return [who[perm], rating[perm]]


def two_level_table(seed=12):
    """(country, product, price): 12 countries x up to 30 products, 1 to 6 rows per pair; prices are xsd:integer ids"""
    rng = np.random.default_rng(seed)
    pairs = [(c + 100, p + 500) for c in range(12) for p in range(30) if rng.random() < 0.7]
    n = rng.integers(1, 7, len(pairs))
    country = np.repeat(np.asarray([c for c, _ in pairs], np.uint32), n)
    product = np.repeat(np.asarray([p for _, p in pairs], np.uint32), n)
    price = rng.integers(1, 1001, len(country)).astype(np.uint32)
    perm = rng.permutation(len(country))
    return [country[perm], product[perm], price[perm]]


def kinds_table():
    """(group, value): one group per kind of result, and the error value: integer; decimal with a negative high word; float; double;
    an integer SUM past i64"""
    groups = [[IDS["i5"], IDS["i-1"], IDS["i2^32"]], [IDS["d-1"], IDS["d-E18"], IDS["i-1"]], [IDS["f0.75"], IDS["i1"], IDS["f0.75"]],
              [IDS["g0.5"], IDS["i1"], IDS["dE18"]], [IDS["iMAX"], IDS["iMAX"]], [IDS["i3"], IDS["i5"]]]
    key = np.concatenate([np.full(len(g), 10 + 7 * i, np.uint32) for i, g in enumerate(groups)])
    return [key, np.concatenate([np.asarray(g, np.uint32) for g in groups])]


def overflow_table(groups=40):
    """(group, value): every fifth group's integer SUM overflows i64 (two I64_MAX among its rows); the others sum small integers"""
    rng = np.random.default_rng(5)
    key, value = [], []
    for g in range(groups):
        n = int(rng.integers(2, 6))
        key += [g + 50] * n
        value += [IDS["iMAX"], IDS["iMAX"]] + [3] * (n - 2) if g % 5 == 0 else rng.integers(1, 100, n).tolist()
    perm = rng.permutation(len(key))
    return [np.asarray(key, np.uint32)[perm], np.asarray(value, np.uint32)[perm]]
