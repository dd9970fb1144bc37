"""The aggregate edge cases of agg_cases.py on the CPU: every total case's SUM and AVG, worked by hand there, must be what the
restatement of the reference's accumulators (test_aggregate_cpu.py) returns for it, so that neither a slip of the hand nor a wrong
restatement can hide a device bug; and the tables must be worth running: the limb sums, runs, group counts and row counts the device
tests (test_gpu_aggregate_edges.py) are there for are in them.  No GPU needed."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from rdf_fusion_amd import abi
import agg_cases as ac
from test_aggregate_cpu import sum_agg, avg_agg, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rdf-fusion_amd", "csrc")


def typed(v):
    return type(v), v            # Fraction(5) == 5 in Python: an xsd:decimal 5 is not an xsd:integer 5


@pytest.mark.parametrize("c", ac.TOTAL_CASES, ids=[c.name for c in ac.TOTAL_CASES])
def test_hand_written_totals_equal_the_restatement(c):
    values = [ac.val(i) for i in c.ids]
    assert typed(ac.python_value(sum_agg(values))) == typed(c.sum), c.name
    assert typed(ac.python_value(avg_agg(values))) == typed(c.avg), c.name


def test_total_cases_hold_what_the_issue_lists():
    by_name = {c.name: c for c in ac.TOTAL_CASES}
    assert len(by_name) == len(ac.TOTAL_CASES)
    n, MAX, MIN = ac.IDS, ac.IDS["iMAX"], ac.IDS["iMIN"]
    assert by_name["int-max+1-1"].ids == [MAX, n["i1"], n["i-1"]] and by_name["int-min+max"].ids == [MIN, MAX]
    assert by_name["avg-18-max"].ids == [MAX] * 18 and by_name["avg-19-max"].ids == [MAX] * 19
    top = sum(ac.val(i)[1] for i in by_name["avg-int-top"].ids)
    assert top == ac.I128_MAX // ac.E18 == 170141183460469231731 and ac.TOP_FILL == 4120486797083267205
    assert sum(ac.val(i)[1] for i in by_name["avg-int-top+1"].ids) == top + 1
    mixed = by_name["mixed-max"].ids
    assert sum(ac.val(i)[1] * (ac.E18 if ac.val(i)[0] == abi.TV_INTEGER else 1) for i in mixed) == ac.I128_MAX
    assert {ac.val(i)[0] for i in mixed} == {abi.TV_INTEGER, abi.TV_DECIMAL}
    for name in ("limb-int-2^32-1", "limb-dec-2^64-1", "limb-dec-2^96-1", "limb-dec--1", "limb-int--1"):
        assert len(by_name[name].ids) == 257 and len(set(by_name[name].ids)) == 1
    c = by_name["cancelling"]
    assert c.ids.count(MAX) == c.ids.count(MIN) == 20000 and len(c.ids) == 40001 and c.ids[:4] == [MAX, MIN, MAX, MIN]
    assert 2 ** 46 < 20000 * (2 ** 32 - 1) < 2 ** 47                       # the low limb's sum
    # every value of the table is in some case or column
    used = {i for c in ac.TOTAL_CASES for i in c.ids} | {n[x] for x in ac.INT_CYCLE + ac.DEC_CYCLE + ac.FLOAT_CYCLE + ac.LIMB_SET}
    assert used >= set(range(ac.N_SMALL + 1, len(ac.TV))) and 0 in used


def test_the_edge_set_is_not_dull():
    sums, avgs = [c.sum for c in ac.TOTAL_CASES], [c.avg for c in ac.TOTAL_CASES]
    for results in (sums, avgs):
        assert sum(r is not None for r in results) >= 12 and sum(r is None for r in results) >= 8
    assert sum(isinstance(r, int) for r in sums) >= 8 and sum(isinstance(r, Fraction) for r in sums) >= 8
    assert any(s is None and a is not None for s, a in zip(sums, avgs)) and any(s is not None and a is None for s, a in zip(sums, avgs))


def test_typed_table_round_trips():
    """the table's encoding, read back the way the device reads it, gives the values the restatement is fed"""
    tv, dec = ac.TV, ac.DECIMALS
    assert tv.dtype == ac.TV_DTYPE and dec.dtype == np.int64 and dec.shape[1] == 2
    for i in range(1, len(tv)):
        tag, lo = int(tv["tag"][i]), int(tv["lo"][i])
        want_tag, want = ac.val(i)
        assert tag == want_tag
        if tag == abi.TV_DECIMAL:
            raw = ((int(dec[lo][1]) & (2 ** 64 - 1)) << 64) | (int(dec[lo][0]) & (2 ** 64 - 1))
            assert (raw - 2 ** 128 if raw >> 127 else raw) == want
        elif tag == abi.TV_FLOAT:
            assert float(np.uint32(lo).view(np.float32)) == want
        elif tag == abi.TV_DOUBLE:
            assert float(np.int64(lo).view(np.float64)) == want
        else:
            assert lo == want
    assert ac.val(0) == ac.val(len(tv)) == (abi.TV_NULL, None)
    assert [ac.val(i) for i in (1, 5, 1000)] == [(abi.TV_INTEGER, 1), (abi.TV_INTEGER, 5), (abi.TV_INTEGER, 1000)]


def test_totals_tables():
    exp = None
    for order in ("sorted", "shuffled", "filtered"):
        cols = ac.totals_table(order)
        if order == "filtered":
            live = cols[2] == ac.KEEP_ID
            assert set(cols[2].tolist()) == {ac.KEEP_ID, ac.DROP_ID}
            assert not live[-1000:].any() and 0.2 < 1 - live[:-1000].mean() < 0.3       # dropped rows after and among the live ones
            assert live.sum() % 64 != 0 and live.sum() < len(live)
            cols = [c[live] for c in cols[:2]]
        assert (np.diff(cols[0].astype(np.int64)) >= 0).all() == (order == "sorted")
        got = ac.expected(cols, [0], [(ac.SUM, 1), (ac.AVG, 1), (ac.STAR, None)])
        assert len(got) == len(ac.TOTAL_CASES)
        for g, c in enumerate(ac.TOTAL_CASES):
            s, a, star = got[(g,)]
            assert star == (abi.TV_INTEGER, len(c.ids))
            for res, lit in ((s, c.sum), (a, c.avg)):
                assert typed(ac.python_value(res)) == typed(lit), (order, c.name)
        exp = exp or got
        assert all(ac.python_value(got[k][j]) == ac.python_value(exp[k][j]) for k in exp for j in range(3))


def test_literal_result_and_same():
    assert ac.literal_result(None) == (abi.TV_NULL, None) and ac.literal_result(-2) == (abi.TV_INTEGER, -2)
    assert ac.literal_result(Fraction(-1, 2)) == (abi.TV_DECIMAL, -5 * 10 ** 17) and ac.literal_result(0.5) is None
    assert same(ac.literal_result(Fraction(5)), (abi.TV_DECIMAL, 5 * ac.E18, 0)) and not same(ac.literal_result(5), (abi.TV_DECIMAL, 5 * ac.E18, 0))


def test_run_layout_meets_its_conditions():
    keys = ac.run_layout()
    ac.check_run_layout(keys)                                             # (run_layout asserts them itself; once more, on what it returned)
    assert np.array_equal(keys, ac.run_layout(ac.RUN_SEED))
    with pytest.raises(AssertionError):
        ac.check_run_layout(keys[:len(keys) // 64 * 64])                  # the conditions can fail: cut at a wave's end
    with pytest.raises(AssertionError):
        ac.check_run_layout(np.repeat(np.arange(50, dtype=np.uint32), 65))
    st = ac.run_starts(np.array([4, 4, 9, 4, 4, 4], np.uint32))
    assert st.tolist() == [0, 2, 3, 6]


def test_run_table_has_totals_on_both_sides():
    cols = ac.run_table()
    exp = ac.expected(cols, [0], ac.RUN_AGGS)
    assert len(exp) == ac.RUN_GROUPS
    for a, tag in ((1, abi.TV_INTEGER), (3, abi.TV_DECIMAL)):             # SUM(integer), SUM(decimal): groups that fit and groups that do not
        tags = [r[a][0] for r in exp.values()]
        assert tags.count(tag) >= 3 and tags.count(abi.TV_NULL) >= 3 and set(tags) == {tag, abi.TV_NULL}, tags
    assert all(r[5][0] == abi.TV_FLOAT and len(r[5][1].terms) == r[0][1] for r in exp.values())
    assert {r[4] for r in exp.values()} == {(abi.TV_INTEGER, 4)}


def _constant(text, name):
    return int(re.search(rf"\b{name}\s*=\s*(?:\(\w+\))?(\d+)", text).group(1))


def test_geometry_matches_the_sources():
    hpp = open(os.path.join(CSRC, "kernels.hpp")).read()
    assert _constant(hpp, "kAggLdsBytes") == ac.LDS_BYTES == 65536 and _constant(hpp, "kAggSumWords") == ac.SUM_WORDS == 11
    edges = ac.form_edges()
    assert [(lo, hi) for _, lo, hi in edges] == [(8192, 8193), (682, 683), (356, 357)]
    for aggs, lo, hi in edges:
        assert ac.n_words(aggs) * lo * 8 <= ac.LDS_BYTES < ac.n_words(aggs) * hi * 8
    hip = open(os.path.join(CSRC, "aggregate.hip")).read()
    assert _constant(hip, "kAggBlock") == ac.ACCUM_BLOCK and _constant(hip, "kAggBlock") * _constant(hip, "kAggItems") == ac.GROUP_TILE
    assert _constant(hip, "kAggGroupGrid") == ac.GROUP_GRID
    assert [_constant(hip, "kAggAccumLdsGrid"), _constant(hip, "kAggAccumHbmGrid")] == [ac.ACCUM_LDS_GRID, ac.ACCUM_HBM_GRID]
    # the smallest row counts at which the second trips exist, and partial ones
    assert ac.BIG_ROWS > ac.GROUP_TILE * ac.GROUP_GRID and ac.BIG_ROWS % ac.GROUP_TILE not in (0,) and ac.BIG_ROWS % 64 != 0
    assert ac.BIG_ROWS > ac.ACCUM_BLOCK * ac.ACCUM_HBM_GRID and ac.BIG_ROWS < 2 * ac.GROUP_TILE * ac.GROUP_GRID
    assert ac.ACCUM_BLOCK * ac.ACCUM_LDS_GRID < ac.SWEEP_ROWS < 2 * ac.ACCUM_BLOCK * ac.ACCUM_LDS_GRID and ac.SWEEP_ROWS % 64 != 0
    assert ac.n_words([(ac.STAR, None), (ac.SUM, 1), (ac.AVG, 1)]) * ac.SWEEP_GROUPS * 8 <= ac.LDS_BYTES


def test_form_and_group_tables():
    for _, lo, hi in ac.form_edges():
        for groups in (lo, hi):
            key, value = ac.form_table(groups)
            assert len(key) == 3 * groups and len(set(key.tolist())) == groups
    assert {ac.IDS[x] for x in ac.LIMB_SET} == set(ac.form_table(357)[1].tolist())
    for rows in ac.GROUP_ROWS:
        for n_keys in ac.GROUP_KEYS:
            cols = ac.distinct_tuples(rows, n_keys)                       # (asserts its own conditions)
            assert len(cols) == n_keys + 1 and all(len(c) == rows and c.dtype == np.uint32 for c in cols)


def test_sweep_table_totals():
    cols = ac.sweep_table()
    exp = ac.expected(cols, [0], [(ac.STAR, None), (ac.SUM, 1), (ac.AVG, 1)])
    assert len(exp) == ac.SWEEP_GROUPS
    sums = [r[1] for r in exp.values()]
    assert sum(t == abi.TV_NULL for t, _ in sums) == 1                    # the group of the last row
    assert all(t == abi.TV_NULL or v == r[0][1] // 4 * (2 ** 32 - 3) for (t, v), r in zip(sums, exp.values()))
    assert min(r[0][1] for r in exp.values()) > 1024                      # limb sums past 2^40
