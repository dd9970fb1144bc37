"""MIN / MAX of AggregateExec on the MI355X (plans with abi.PLAN_AGG_COLUMNS): the hand-written cases, order independence, the row and
form edges of the accumulate pass, the decimal refinement, the error rules, zero keys, a row count known on the device only and the BI
Q5 / Q6 shapes.  Every expectation is minmax_cases.device_rule; results are compared as (tag, lo, hi) bit for bit, except the payload of
an all-NaN group."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rdf_fusion_amd import abi
from rdf_fusion_amd.engine import RdfGpuError
from rdf_fusion_amd.plan import PlanBuilder, col, integer, EBV, GT, DIV, NOT, BOUND, ENC_TV
from test_gpu_parity import both_stores, table_on_device
from test_aggregate_cpu import avg_agg, same
import agg_cases as ac
import aggcol_cases as cc
import numeric_ref as nr
import minmax_cases as mc
from minmax_cases import MIN, MAX, COUNT, AVG, SUM, ERR, IDS

EMPTY = (np.zeros(0, np.uint32),) * 4
ACCUM, ACCUM_EXPR, REFINE = "void rdfgpu::agg_accum_minmax_kernel<", "void rdfgpu::agg_accum_minmax_expr_kernel<", "void rdfgpu::agg_minmax_refine_kernel"
FORMS = [None, "NO_AGG_LDS"]


@pytest.fixture(scope="module")
def gs(torch_cuda):
    return both_stores(EMPTY, typed=mc.TV, decimals=mc.DECIMALS)[0]


def compiled(gs, widths, root_of, option=None):
    pb = PlanBuilder()
    plan = gs.plan(pb.build(root_of(pb, [pb.table(slot, w) for slot, w in enumerate(widths)]), agg_columns=True))
    if option:
        plan.set_option(option)
    plan.enable_kernel_timing(True)
    return plan


def bind(torch, plan, tables):
    plan._keep_cols = []
    for slot, cols in enumerate(tables):
        keep, ptrs = table_on_device(torch, cols)
        plan._keep_cols.append(keep)
        plan.bind_table(slot, ptrs, len(cols[0]))


def run(torch, gs, tables, root_of, option=None):
    plan = compiled(gs, [len(t) for t in tables], root_of, option)
    bind(torch, plan, tables)
    return plan.execute()


def kernels(plan):
    return [s[0] for s in plan.kernel_stats()]


def matches(want, got):
    """a result of device_rule against a device record (tag, lo, hi)"""
    if mc.is_nan(want):
        bits = got[1] & 0xFFFFFFFF if want[0] == abi.TV_FLOAT else got[1]
        return got[0] == want[0] and math.isnan(mc._unrecord(got[0], (bits, 0))[1])
    return mc.record(want) == got


def results(plan, n_keys):
    rows, vcols = cc.device_rows(plan)                                # (asserts: an entry of 0 <=> the null value)
    assert vcols == list(range(n_keys, len(rows[0]) if rows else n_keys))
    out = {r[:n_keys]: r[n_keys:] for r in rows}
    assert len(out) == len(rows)
    return out


def check(plan, cols, keys, aggs, value=mc.val):
    want, got = mc.expected(cols, keys, aggs, value), results(plan, len(keys))
    assert set(got) == set(want)
    for k, res in want.items():
        for a, (w, g) in enumerate(zip(res, got[k])):
            assert matches(w, g), (k, aggs[a], w, g)
    return got


def aggregate(torch, gs, cols, keys, aggs, option=None):
    return run(torch, gs, [cols], lambda pb, t: pb.aggregate(t[0], keys, aggs), option)


def ran(plan, lds, prefix=ACCUM, only=True):
    """which accumulate kernel the MIN / MAX node launched; only: no other AggregateExec is in the plan"""
    names = kernels(plan)
    assert any(n.startswith(f"{prefix}{'true' if lds else 'false'}>") for n in names), names
    assert any(n.startswith(REFINE) for n in names), names
    assert not only or not any(n.startswith("void rdfgpu::agg_accum_kernel<") or n.startswith("void rdfgpu::agg_accum_expr_kernel<") for n in names), names


# ---------------------------------------------------------------------------------------------------
# the hand-written cases, order independence
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option", FORMS)
def test_hand_written_cases(torch_cuda, gs, option):
    """every answered case as one group among filler groups, MIN and MAX in one node, in both forms of the accumulate pass"""
    cols = mc.case_table(mc.ANSWERED, "shuffled")
    plan = aggregate(torch_cuda, gs, cols, [0], [(MIN, 1), (MAX, 1)], option)
    got = check(plan, cols, [0], [(MIN, 1), (MAX, 1)])
    for g, c in enumerate(mc.ANSWERED):                               # .. and against the results worked by hand
        assert matches(c.min, got[(10 + g,)][0]) and matches(c.max, got[(10 + g,)][1]), c.name
    ran(plan, lds=option is None)


def test_a_node_without_min_max_launches_what_it_did(torch_cuda, gs):
    cols = mc.case_table(mc.ANSWERED)
    names = kernels(aggregate(torch_cuda, gs, cols, [0], [(SUM, 1), (AVG, 1)]))
    assert any(n.startswith("void rdfgpu::agg_accum_kernel<true>") for n in names) and not any("minmax" in n for n in names), names


def test_row_order_does_not_matter(torch_cuda, gs):
    key, value = mc.case_table(mc.ANSWERED * 3)                       # (every case three times: runs and repeats)
    key = np.concatenate([key, key[:len(key) // 2]])
    value = np.concatenate([value, value[:len(value) // 2]])
    asc = np.lexsort((value, key))
    seen = []
    for order in (asc, asc[::-1], np.random.default_rng(4).permutation(len(key))):
        cols = [key[order], value[order]]
        seen.append(check(aggregate(torch_cuda, gs, cols, [0], [(MIN, 1), (MAX, 1)]), cols, [0], [(MIN, 1), (MAX, 1)]))
    assert seen[0] == seen[1] == seen[2]


# ---------------------------------------------------------------------------------------------------
# row edges
# ---------------------------------------------------------------------------------------------------
ROWS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)


@pytest.mark.parametrize("option", FORMS)
@pytest.mark.parametrize("n", ROWS)
def test_row_edges(torch_cuda, gs, n, option):
    """one group holds all n rows (the integer 500); the winner — the integer 1 for MIN, 1000 for MAX, a float -inf / +inf in a third
    column — sits at the first row, the last row, the last lane of the first wave and the first row of the second workgroup"""
    plan = compiled(gs, [4], lambda pb, t: pb.aggregate(t[0], [0], [(MIN, 1), (MAX, 2), (MIN, 3), (MAX, 3)]), option)
    for at in sorted({0, n - 1, min(63, n - 1), min(256, n - 1)}):
        lo, hi, f = np.full(n, 500, np.uint32), np.full(n, 500, np.uint32), np.full(n, IDS["f0.75"], np.uint32)
        lo[at], hi[at] = 1, 1000
        f[at] = IDS["f-inf"]
        f[(at + 1) % n] = IDS["g+inf"] if n > 1 else f[at]
        cols = [np.full(n, 9, np.uint32), lo, hi, f]
        bind(torch_cuda, plan, [cols])
        plan.execute()
        got = check(plan, cols, [0], [(MIN, 1), (MAX, 2), (MIN, 3), (MAX, 3)])
        assert got[(9,)][:2] == ((abi.TV_INTEGER, 1, 0), (abi.TV_INTEGER, 1000, 0))
    ran(plan, lds=option is None)


@pytest.mark.parametrize("option", FORMS)
def test_runs_of_equal_neighbouring_groups(torch_cuda, gs, option):
    """agg_cases' run layout (runs of 1 to 257 rows that start at every lane and cross wave and workgroup boundaries, waves of heads only)
    with values of every numeric kind drawn at random, NaNs included"""
    key = ac.run_layout()
    rng = np.random.default_rng(9)
    pool = np.asarray([i for i in mc.NUMERIC_IDS if i != 0], np.uint32)
    cols = [key, rng.choice(pool, len(key)), rng.integers(1, 1001, len(key)).astype(np.uint32)]
    aggs = [(MIN, 1), (MAX, 1), (MAX, 2)]
    check(aggregate(torch_cuda, gs, cols, [0], aggs, option), cols, [0], aggs)


# ---------------------------------------------------------------------------------------------------
# the LDS / HBM switch
# ---------------------------------------------------------------------------------------------------
FORM_SET = ("i2^32-1", "d2^64-1", "dHI+1", "f-0", "g2.5", "int-1", "dHI+2")


def form_table(groups):
    """(group, value): three rows per group, shuffled; group g holds FORM_SET[g], [g + 1] and [g + 3] (indices modulo 7)"""
    ids = [IDS[x] for x in FORM_SET]
    key = np.repeat(np.arange(groups, dtype=np.uint32), 3)
    value = np.asarray([ids[(g + j) % 7] for g in range(groups) for j in (0, 1, 3)], np.uint32)
    perm = np.random.default_rng(groups).permutation(len(key))
    return [key[perm], value[perm]]


@pytest.mark.parametrize("option", FORMS)
@pytest.mark.parametrize("aggs", [[(MIN, 1)], [(MIN, 1), (AVG, 1)]], ids=["min", "min+avg"])
def test_form_switch(torch_cuda, gs, aggs, option):
    """the group counts on either side of 65536 / (8 * words): one MIN alone (1 + 7 words), one MIN beside one AVG (Q6's node: 1 + 7 + 11)"""
    words = 1 + sum(mc.MINMAX_WORDS if fn == MIN else ac.SUM_WORDS for fn, _ in aggs)
    fit = ac.LDS_BYTES // (8 * words)
    assert fit == (1024 if len(aggs) == 1 else 431)
    for groups in (fit, fit + 1):
        cols = form_table(groups)
        plan = aggregate(torch_cuda, gs, cols, [0], aggs, option)
        got = results(plan, 1)
        want = mc.expected(cols, [0], aggs[:1])
        assert set(got) == set(want) and all(matches(want[k][0], got[k][0]) for k in want)
        if len(aggs) == 2:                                            # the AVG beside it, by the restatement of test_aggregate_cpu.py
            members = {}
            for k, v in cc.rows_of(cols):
                members.setdefault((k,), []).append(mc.val(v))
            assert all(same(avg_agg(members[k]), got[k][1]) for k in members)
        ran(plan, lds=option is None and groups == fit)


# ---------------------------------------------------------------------------------------------------
# the decimal refinement
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option", FORMS)
def test_decimal_refinement(torch_cuda, gs, option):
    """group 1: 700 rows that share the high word 5, the smallest and the largest low word more than 256 rows apart, among decimals of
    lower high words whose low words are larger (2^64 - 1: high 0, every low bit set); group 2: the same within one wave's run; group 3:
    negative against positive, -(5 * 2^64 + 1) and 5 * 2^64 + 1; group 4: dMIN and dMAX among integers"""
    n = IDS
    g1 = np.resize(np.asarray([n["dHI+1"], n["dHI+2"]], np.uint32), 700)
    g1[5], g1[650], g1[300], g1[301] = n["dHI+top"], n["dHI+0"], n["d2^64-1"], n["d-1"]
    g2 = np.resize(np.asarray([n["dHI+2"], n["dHI+1"]], np.uint32), 40)
    g2[7], g2[31] = n["dHI+0"], n["dHI+top"]
    g3 = np.asarray([n["dHI+1"], n["d-HI-1"], n["dHI+2"], n["d0"], n["d2^64-1"]] * 20, np.uint32)
    g4 = np.asarray([n["dMAX"], n["i5"], n["dMIN"], n["iMAX"], n["d2^96-1"]] * 70, np.uint32)
    key = np.concatenate([np.full(len(g), 1 + i, np.uint32) for i, g in enumerate((g1, g2, g3, g4))])
    cols = [key, np.concatenate([g1, g2, g3, g4])]
    assert np.flatnonzero(cols[1] == n["dHI+0"])[0] - np.flatnonzero(cols[1] == n["dHI+top"])[0] > 256
    aggs = [(MIN, 1), (MAX, 1)]
    got = check(aggregate(torch_cuda, gs, cols, [0], aggs, option), cols, [0], aggs)
    D = lambda raw: mc.record((abi.TV_DECIMAL, raw))
    assert got[(1,)] == (D(-1), D(mc.HI5 + 2 ** 64 - 1)) and got[(2,)] == (D(mc.HI5), D(mc.HI5 + 2 ** 64 - 1))
    assert got[(3,)] == (D(-(mc.HI5 + 1)), D(mc.HI5 + 2)) and got[(4,)] == (D(ac.I128_MIN), D(ac.I128_MAX))
    shuffled = [c[np.random.default_rng(2).permutation(len(key))] for c in cols]
    assert check(aggregate(torch_cuda, gs, shuffled, [0], aggs, option), shuffled, [0], aggs) == got


def test_a_node_without_decimals_is_untouched_by_the_refinement(torch_cuda, gs):
    """the same groups without a decimal anywhere (the refinement leaves on its device word) and beside one group of decimals (it runs
    over every row): the same records"""
    rng = np.random.default_rng(6)
    pool = np.asarray([i for i in mc.NUMERIC_IDS if i != 0 and mc.val(i)[0] != abi.TV_DECIMAL], np.uint32)
    plain = [rng.integers(1, 60, 3000).astype(np.uint32), rng.choice(pool, 3000)]
    extra = [np.full(3, 77, np.uint32), np.asarray([IDS["dHI+1"], IDS["dHI+0"], IDS["d-1"]], np.uint32)]
    with_dec = [np.concatenate([a, b]) for a, b in zip(plain, extra)]
    aggs = [(MIN, 1), (MAX, 1)]
    a, b = aggregate(torch_cuda, gs, plain, [0], aggs), aggregate(torch_cuda, gs, with_dec, [0], aggs)
    ga, gb = check(a, plain, [0], aggs), check(b, with_dec, [0], aggs)
    assert all(gb[k] == v for k, v in ga.items()) and set(gb) - set(ga) == {(77,)}
    assert any(n.startswith(REFINE) for n in kernels(a)) and any(n.startswith(REFINE) for n in kernels(b))


# ---------------------------------------------------------------------------------------------------
# rules 2 and 3, zero keys
# ---------------------------------------------------------------------------------------------------
def test_an_unbound_id_makes_its_own_group_null(torch_cuda, gs):
    rng = np.random.default_rng(3)
    cols = [rng.integers(1, 40, 900).astype(np.uint32), rng.integers(1, 1001, 900).astype(np.uint32)]
    hit = sorted(set(cols[0][[5, 450, 899]].tolist()))
    cols[1][[5, 450, 899]] = 0
    aggs = [(MIN, 1), (MAX, 1)]
    plan = aggregate(torch_cuda, gs, cols, [0], aggs)
    got = check(plan, cols, [0], aggs)
    assert sorted(k[0] for k, v in got.items() if v[0][0] == abi.TV_NULL) == hit and all(v[0][0] == v[1][0] for v in got.values())
    # BOUND is false above it, and the export delivers a null
    above = run(torch_cuda, gs, [cols], lambda pb, t: pb.filter(pb.aggregate(t[0], [0], aggs), NOT(BOUND(col(1)))))
    assert sorted(above.fetch()[0].tolist()) == hit
    arrow = list(plan.batches())
    valid = np.concatenate([np.asarray(b.field(1).is_valid()) for b in arrow])
    ids = np.concatenate([b.field(0).to_numpy(zero_copy_only=False) for b in arrow])
    assert sorted(ids[~valid].tolist()) == hit


def test_an_error_entry_of_a_value_column_makes_its_own_group_null(torch_cuda, gs):
    """(outer, inner, value): SUM per (outer, inner), one of which overflows i64 (entry 0 in its value column); MAX / MIN of the sums per
    outer: the outer group that holds it is NULL, the others are answered"""
    inner, value = cc.overflow_table()
    outer = ((inner - 50) % 10 + 1).astype(np.uint32)                  # (groups 50, 55, 60 .. overflow: the outer groups 1 and 6 hold them)
    cols = [outer, inner, value]
    plan = run(torch_cuda, gs, [cols], lambda pb, t: pb.aggregate(pb.aggregate(t[0], [0, 1], [(SUM, 2)]), [0], [(MAX, 2), (MIN, 2)]))
    sums = cc.aggregate(cc.rows_of(cols), [0, 1], [(SUM, 2)])
    by_outer = {}
    for o, _, s in sums:
        by_outer.setdefault((o,), []).append(ERR if s == cc.UNBOUND else s)
    want = {k: [mc.device_rule(v, MAX), mc.device_rule(v, MIN)] for k, v in by_outer.items()}
    got = results(plan, 1)
    assert set(got) == set(want) and all(matches(w, g) for k in want for w, g in zip(want[k], got[k]))
    nulls = [k for k, v in want.items() if v[0] == ERR]
    assert 0 < len(nulls) < len(want)
    ran(plan, lds=True, prefix=ACCUM_EXPR, only=False)


def test_a_division_by_zero_makes_its_own_group_null(torch_cuda, gs):
    rng = np.random.default_rng(8)
    cols = [rng.integers(1, 30, 600).astype(np.uint32), rng.integers(1, 1001, 600).astype(np.uint32), rng.integers(1, 50, 600).astype(np.uint32)]
    cols[2][[17, 400]] = IDS["i0"]
    expr = DIV(ENC_TV(col(1)), ENC_TV(col(2)))
    plan = aggregate(torch_cuda, gs, cols, [0], [(MIN, expr), (MAX, expr)])
    rows = {}
    for k, x, y in cc.rows_of(cols):
        rows.setdefault((k,), []).append(nr.binary(abi.EX_DIV, mc.val(x), mc.val(y)))
    want = {k: [mc.device_rule(v, MIN), mc.device_rule(v, MAX)] for k, v in rows.items()}
    got = results(plan, 1)
    assert set(got) == set(want) and all(matches(w, g) for k in want for w, g in zip(want[k], got[k]))
    assert sorted(k[0] for k, v in want.items() if v[0] == ERR) == sorted(set(cols[0][[17, 400]].tolist()))
    ran(plan, lds=True, prefix=ACCUM_EXPR)


@pytest.mark.parametrize("bad", ["str", "bool"])
def test_a_value_that_is_not_numeric_fails_the_execute(torch_cuda, gs, bad):
    rng = np.random.default_rng(1)
    cols = [rng.integers(1, 20, 500).astype(np.uint32), rng.integers(1, 1001, 500).astype(np.uint32)]
    broken = [cols[0], cols[1].copy()]
    broken[1][333] = IDS[bad]
    aggs = [(MAX, 1), (MIN, 1)]
    plan = compiled(gs, [2], lambda pb, t: pb.aggregate(t[0], [0], aggs))
    bind(torch_cuda, plan, [broken])
    with pytest.raises(RdfGpuError) as err:
        plan.execute()
    assert err.value.status == abi.ERR_UNSUPPORTED and "MIN / MAX" in str(err.value), err.value
    bind(torch_cuda, plan, [cols])                                    # the plan stays usable
    plan.execute()
    check(plan, cols, [0], aggs)


def test_zero_keys(torch_cuda, gs):
    aggs = [(MIN, 1), (MAX, 1)]
    plan = compiled(gs, [2], lambda pb, t: pb.aggregate(t[0], [], aggs))
    cols = [np.zeros(300, np.uint32), np.random.default_rng(5).integers(3, 1001, 300).astype(np.uint32)]
    cols[1][299] = IDS["g-3.5"]
    bind(torch_cuda, plan, [cols])
    plan.bind_table(0, [t.data_ptr() for t in plan._keep_cols[0]], 0)      # an empty input: one row, the error value
    plan.execute()
    assert results(plan, 0) == {(): ((0, 0, 0), (0, 0, 0))} and plan.fetch()[0].tolist() == [0]
    bind(torch_cuda, plan, [cols])
    plan.execute()
    got = check(plan, cols, [], aggs)
    assert got[()][0] == mc.record((abi.TV_DOUBLE, -3.5)) and plan.result_info()[0] == 1


# ---------------------------------------------------------------------------------------------------
# a row count known on the device only
# ---------------------------------------------------------------------------------------------------
def test_row_count_known_on_the_device_only(torch_cuda, gs):
    """MIN / MAX above an inner join, whose output is counted on the device: one compiled plan over tables of other sizes"""
    plan = compiled(gs, [2, 2], lambda pb, t: pb.aggregate(pb.hash_join(t[0], t[1], [(0, 0)], projection=[1, 3]), [0], [(MIN, 1), (MAX, 1)]))
    pool = np.asarray([i for i in mc.NUMERIC_IDS if i != 0], np.uint32)
    for n in (65, 1500, 300):
        rng = np.random.default_rng(n)
        left = [np.arange(1, n + 1, dtype=np.uint32), rng.integers(1, 12, n).astype(np.uint32)]             # key, group
        right = [rng.permutation(np.arange(1, n + 1, dtype=np.uint32))[: n - 7], rng.choice(pool, n - 7)]    # key, value
        bind(torch_cuda, plan, [left, right])
        plan.execute()
        joined = [(r[1], r[3]) for r in cc.join(cc.rows_of(left), cc.rows_of(right), [(0, 0)])]
        assert len(joined) == n - 7
        check(plan, [np.asarray(c, np.uint32) for c in zip(*joined)], [0], [(MIN, 1), (MAX, 1)])


# ---------------------------------------------------------------------------------------------------
# BI Q5 and Q6
# ---------------------------------------------------------------------------------------------------
def test_q5_shape(torch_cuda, gs):
    """COUNT per (country, product); MAX of it per country; the join back with count = max; ORDER BY count DESC, country, product"""
    country, product, _ = cc.two_level_table()
    review = np.arange(1, len(country) + 1, dtype=np.uint32)
    review[::37] = 0                                                    # (an unbound review is not counted)
    cols = [country, product, review]
    plan = run(torch_cuda, gs, [cols], lambda pb, t: mc.q5_plan(pb, t[0]))
    counts = {}
    for c, p, r in cc.rows_of(cols):
        counts[(c, p)] = counts.get((c, p), 0) + (r != 0)
    best = {}
    for (c, p), k in counts.items():
        best[c] = max(best.get(c, 0), k)
    want = sorted(((c, p, k) for (c, p), k in counts.items() if k == best[c]), key=lambda r: (-r[2], r[0], r[1]))
    assert 12 <= len(want) < len(counts)
    rows, vcols = cc.device_rows(plan)
    assert vcols == [2] and [(c, p, v) for c, p, v in rows] == [(c, p, (abi.TV_INTEGER, k, 0)) for c, p, k in want]
    ran(plan, lds=True, prefix=ACCUM_EXPR, only=False)


def q6_table(reviewers=200, seed=8):
    """(reviewer, score): four scores each (ids 1 .. 10 = the xsd:integer scores), their sum a multiple of 8: the global average has two
    fractional digits, so `min * 1.5` is a value (Decimal::checked_mul is the error value when its operands' trailing zeros are fewer than 18)"""
    rng = np.random.default_rng(seed)
    who = np.repeat(np.arange(reviewers, dtype=np.uint32) + 2000, 4)
    score = rng.integers(1, 11, len(who)).astype(np.uint32)
    while int(score.sum()) % 8:
        score[-1] = score[-1] % 10 + 1
    perm = rng.permutation(len(who))
    return [who[perm], score[perm]]


def test_q6_shape(torch_cuda, gs):
    """the global AVG(score); cross join; AVG(score) and MIN(global average) per reviewer; HAVING avg > min * 1.5"""
    cols = q6_table()
    plan = run(torch_cuda, gs, [cols], lambda pb, t: mc.q6_plan(pb, t[0]))
    overall = cc.aggregate(cc.rows_of(cols), [], [(AVG, 1)])[0][0]
    per = cc.aggregate([r + (overall,) for r in cc.rows_of(cols)], [0], [(AVG, 1)])
    low = mc.device_rule([overall], MIN)
    assert low == overall and overall[0] == abi.TV_DECIMAL
    want = cc.having([r + (low,) for r in per], lambda r: cc.compare("gt", r[1], cc.mul(r[2], (abi.TV_DECIMAL, 15 * mc.E18 // 10))))
    assert 0 < len(want) < len(per)
    cc.check_rows(want, plan, [1, 2])
    ran(plan, lds=True, prefix=ACCUM_EXPR, only=False)
