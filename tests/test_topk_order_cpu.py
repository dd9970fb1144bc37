"""The TopK cases of topk_cases.py on the CPU: the oracle's rows, in the order it gives them, must be the Python reference's on every case
the device tests run (test_gpu_topk_edges.py), so that a wrong reference cannot hide a device bug, and the tables must be worth running:
the group sizes, limits and values the cases are there for are in them."""
import numpy as np
import pytest

from rdf_fusion_amd import abi
from oracle import oracle as orc
import topk_cases as tc


@pytest.fixture(scope="module")
def oracle_store():
    os_ = orc.OracleStore()
    os_.set_typed_values(tc.TV, tc.DECIMALS)
    return os_


def rows_of(cols, n):
    return [tuple(int(c[r]) for c in cols) for r in range(n)]


@pytest.mark.parametrize("c", tc.CASES, ids=tc.CASE_IDS)
def test_oracle_equals_reference_in_order(oracle_store, c):
    cols, n, _ = oracle_store.execute(tc.topk_plan(c), [c.cols])
    assert len(cols) == tc.out_width(c)
    assert rows_of(cols, n) == tc.expected(c), c.name


def test_the_comparison_sees_the_order(oracle_store):
    """the reversed expectation is the same multiset and must not pass"""
    c = tc.case_named("ladder-k5-grouped")
    want = tc.expected(c)
    cols, n, _ = oracle_store.execute(tc.topk_plan(c), [c.cols])
    got = rows_of(cols, n)
    assert len(want) > 1 and sorted(got) == sorted(want[::-1])
    assert got != want[::-1]
    assert not np.array_equal(np.stack(cols, 1)[:n], tc.as_matrix(want[::-1], tc.out_width(c)))
    assert np.array_equal(np.stack(cols, 1)[:n], tc.as_matrix(want, tc.out_width(c)))


@pytest.mark.parametrize("flag_id", [tc.KEEP_ID, tc.NEVER_ID])
def test_oracle_equals_reference_above_a_filter(oracle_store, flag_id):
    c = tc.case_named("ladder-k5-grouped")
    table = tc.with_flag_column(c)
    live = tc.surviving(table, flag_id)
    cols, n, _ = oracle_store.execute(tc.filtered_topk_plan(c, flag_id), [table])
    assert rows_of(cols, n) == tc.reference(live, c.keys, c.limit, c.group, c.projection, tc.TV, tc.DECIMALS)
    assert (n == 0) == (flag_id == tc.NEVER_ID)
    if flag_id == tc.KEEP_ID:
        assert 0.05 < len(live[0]) / len(table[0]) < 0.2


def test_reference_known_answers():
    tv, dec, ids = tc.TV, tc.DECIMALS, tc.IDS
    key = lambda i, how: tc.sort_key(i, how, tv, dec)
    num = dict(zip([(t, repr(v)) for t, v in tc.NUMERICS], ids["num"]))
    d = lambda v: num[(abi.TV_DOUBLE, repr(np.float64(v)))]
    order = [d("-inf"), d(-1.5), d(-0.0), d(0.0), d(5e-324), d(1.5), d("inf"), d("nan")]
    keys = [key(i, tc.BY_DOUBLE) for i in order]
    assert keys == sorted(keys) and len(set(keys)) == len(keys) and keys[0] > 0           # -inf still sorts after every null
    i53, i53p = num[(abi.TV_INTEGER, repr(2 ** 53))], num[(abi.TV_INTEGER, repr(2 ** 53 + 1))]
    assert key(i53, tc.BY_DOUBLE) == key(i53p, tc.BY_DOUBLE)                              # one double: the id key separates them
    assert key(num[(abi.TV_INTEGER, repr(tc.I64_MIN))], tc.BY_DOUBLE) < key(d(-1.5), tc.BY_DOUBLE) < key(num[(abi.TV_INTEGER, repr(tc.I64_MAX))], tc.BY_DOUBLE)
    assert key(num[(abi.TV_DECIMAL, repr(3 * tc.E18 // 2))], tc.BY_DOUBLE) == key(d(1.5), tc.BY_DOUBLE) == key(num[(abi.TV_FLOAT, repr(np.float32(1.5)))], tc.BY_DOUBLE)
    # 18 fractional digits: the conversion divides two rounded doubles, so it may sit one ulp off the nearest double
    assert abs(key(num[(abi.TV_DECIMAL, repr(1234567890123456789))], tc.BY_DOUBLE) - tc.total_order_key(1.234567890123456789)) <= 1
    for null in (0, ids["beyond"], ids["str"][0], ids["iri"][0]):
        assert key(null, tc.BY_DOUBLE) == 0
    assert key(0, tc.BY_TERM) == key(ids["beyond"], tc.BY_TERM) == (0, 0)
    a, b = ids["twins"][0]
    assert key(a, tc.BY_TERM) == key(b, tc.BY_TERM) and a != b
    assert key(ids["iri"][0], tc.BY_TERM)[0] < key(ids["bnode"][0], tc.BY_TERM)[0] < key(ids["str"][0], tc.BY_TERM)[0]
    # three rows by hand: groups ascending, nulls first, duplicates once, at most k
    s = ids["str"]
    lo, hi = sorted(s[:2], key=lambda i: int(tv["lo"][i]))
    cols = [np.array(x, np.uint32) for x in ([4, 4, 0, 4, 4, 4], [hi, lo, hi, 0, lo, hi], [9, 9, 9, 9, 9, 8])]
    assert tc.reference(cols, tc.TERM_KEYS, 3, 0, None, tv, dec) == [(0, hi, 9), (4, 0, 9), (4, lo, 9), (4, hi, 8)]
    assert tc.reference(cols, tc.TERM_KEYS, 2, None, [2, 1], tv, dec) == [(9, 0), (9, lo)]


def test_tables_hold_what_the_cases_are_for():
    g = tc.case_named("ladder-k1-grouped").cols[0]
    sizes = dict(zip(*[x.tolist() for x in np.unique(g, return_counts=True)]))
    assert sizes == dict(zip(tc.LADDER_GROUPS, tc.LADDER_SIZES))
    assert {1, 2, 63, 64, 65, 127, 128, 129, 1000} <= set(sizes.values()) and {0, 1, 3, 4, 5, 9, 10, 4000, 70000} <= set(sizes)
    assert set(tc.LADDER_LIMITS) == {1, 5, 63, 64, 65, 1024}
    for limit in tc.LADDER_LIMITS:                                   # no two rows of a group alike: a group of n rows gives min(n, k)
        want = tc.expected(tc.case_named(f"ladder-k{limit}-grouped"))
        per_group = {}
        for row in want:
            per_group[row[0]] = per_group.get(row[0], 0) + 1
        assert per_group == {grp: min(n, limit) for grp, n in sizes.items()}
        assert [row[0] for row in want] == sorted(row[0] for row in want)
    labels = set(tc.case_named("ladder-k1-grouped").cols[1].tolist())
    assert {0, tc.IDS["beyond"]} <= labels and any(a in labels and b in labels for a, b in tc.IDS["twins"])
    # duplicates: one row out of fifty; three out of a hundred under a limit of five; the limit falls between two tuples that share all but the last key
    dup = tc.expected(tc.case_named("duplicates-k5"))
    per_group = {grp: [r for r in dup if r[0] == grp] for grp in (1, 2, 3, 6)}
    assert [len(v) for v in per_group.values()] == [1, 3, 5, 5]
    full = tc.reference(tc.case_named("duplicates-k5").cols, tc.TERM_KEYS, 1024, 0, None, tc.TV, tc.DECIMALS)
    sixth = {grp: [r for r in full if r[0] == grp][5] for grp in (3, 6)}
    assert per_group[3][4][1] == sixth[3][1] and per_group[3][4][2] != sixth[3][2]
    assert per_group[6][4][2] == sixth[6][2] and (per_group[6][4][1], sixth[6][1]) in tc.IDS["twins"]
    # four keys: every key decides between two neighbours of the output somewhere
    c = tc.case_named("four-keys-one-group")
    assert len(c.keys) == 4 and [how for _, how in c.keys] == [tc.BY_TERM, tc.BY_DOUBLE, tc.BY_ID, tc.BY_ID]
    tuples = sorted({tuple(tc.sort_key(row[col_], how, tc.TV, tc.DECIMALS) for col_, how in c.keys) for row in zip(*[x.tolist() for x in c.cols])})
    first_difference = {next(i for i in range(4) if x[i] != y[i]) for x, y in zip(tuples, tuples[1:])}
    assert first_difference == {0, 1, 2, 3}
    assert len(tuples) < len(set(zip(*[x.tolist() for x in c.cols[1:]])))            # rows collapse on keys that are not ids
    # numeric order: every numeric of the table, limit above the row count
    c = tc.case_named("numeric-order")
    assert set(tc.IDS["num"]) <= set(c.cols[0].tolist()) and c.limit > len(c.cols[0]) == len(tc.expected(c))
