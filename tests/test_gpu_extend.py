"""Computed columns (abi.NODE_EXTEND: ProjectionExec with expressions, SPARQL BIND) on the MI355X: the BI Q3 ratio, every kind of value
the 24-byte record carries and the error value, the row-count edges of extend_kernel, a row count known on the device only, the computed
column downstream (FILTER, join payload, two parents, a further aggregate, EXTEND over EXTEND), the run-time refusal of a string value
and the export — each against the Python reference of extend_cases.py, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from rdf_fusion_amd import abi
from rdf_fusion_amd.engine import RdfGpuError
from rdf_fusion_amd.plan import PlanBuilder, col, decimal, integer, EBV, GT, ENC_TV, MUL
from test_gpu_parity import both_stores, table_on_device
import agg_cases as ac
import aggcol_cases as cc
import extend_cases as ec
import numeric_ref as nr
from extend_cases import IDS, UNBOUND, INTEGER, DEC, FLT

EMPTY = (np.zeros(0, np.uint32),) * 4
INNER, LEFT, SEMI, ANTI = abi.JOIN_INNER, abi.JOIN_LEFT, abi.JOIN_LEFT_SEMI, abi.JOIN_LEFT_ANTI
COUNT, SUM, AVG = abi.AGG_COUNT, abi.AGG_SUM, abi.AGG_AVG
E18 = 10 ** 18
B = 256                       # rows per workgroup of extend_kernel: kExtendBlock (rdf-fusion_amd/csrc/kernels.hpp); one workgroup per B rows, the grid is not capped
GUARD = 0xA5A5A5A5            # the element behind each array of an EXTEND (Plan::exec_extend, kExtendGuard)


@pytest.fixture(scope="module")
def gs(torch_cuda):
    return both_stores(EMPTY, typed=ac.TV, decimals=ac.DECIMALS)[0]


def bind(torch, plan, tables):
    plan._keep_cols = []
    for slot, cols in enumerate(tables):
        keep, ptrs = table_on_device(torch, cols)
        plan._keep_cols.append(keep)
        plan.bind_table(slot, ptrs, len(cols[0]))


def compiled(gs, n_cols, root_of):
    pb = PlanBuilder()
    nodes = [pb.table(slot, w) for slot, w in enumerate(n_cols)]
    return gs.plan(pb.build(root_of(pb, nodes), agg_columns=True))


def run(torch, gs, tables, root_of, timing=False):
    plan = compiled(gs, [len(t) for t in tables], root_of)
    if timing:
        plan.enable_kernel_timing(True)
    bind(torch, plan, tables)
    return plan.execute()


def device_words(gs, ptr, n):
    """`n` u32 words at device address `ptr`, read by the library itself (a plan whose root is a bound table fetches it as it is)"""
    pb = PlanBuilder()
    reader = gs.plan(pb.build(pb.table(0, 1)))
    reader.bind_table(0, [ptr], n)
    return reader.execute().fetch()[0]


def column_bits(plan, q):
    """value column q of the result, one (tag, lo, hi) per row as numeric_ref.device_bits spells it"""
    return [nr.device_bits(int(v["tag"]), int(v["lo"]), int(v["hi"])) for v in plan.fetch_column_values(q)]


def check_in_row_order(plan, rows, fns, first):
    """an EXTEND over a bound table keeps the rows' order: row r carries r + 1 (or 0), its value is the reference's, bit for bit"""
    ids = plan.fetch()
    for q, fn in enumerate(fns, start=first):
        want = [nr.bits(fn(r)) for r in rows]
        got = column_bits(plan, q)
        assert got == want, (q, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:4])
        entries = ids[q].tolist()
        assert entries == [0 if w[0] == abi.TV_NULL else r + 1 for r, w in enumerate(want)], q      # entry 0 coincides exactly with tag 0


# ---------------------------------------------------------------------------------------------------
# the Q3 shape, every kind
# ---------------------------------------------------------------------------------------------------
def test_q3_ratio_of_two_counts(torch_cuda, gs):
    """300 products, two COUNTs joined LEFT by product, DIV(xsd:float(c1), c2): a third of the products have no partner, their ratio is
    unbound (entry 0)"""
    now, before = ec.q3_tables(300)
    plan = run(torch_cuda, gs, [now, before], lambda pb, t: ec.q3_plan(pb, t[0], t[1]), timing=True)
    ref = ec.q3_reference(now, before)
    assert sum(1 for r in ref if r[3] == UNBOUND) == 100 and len(ref) == 300
    cc.check_rows(ref, plan, [1, 2, 3])
    ids = plan.fetch()
    assert (ids[3] == 0).sum() == 100 and np.array_equal(ids[3] == 0, ids[2] == 0)
    assert set(plan.fetch_column_values(3)["tag"].tolist()) == {abi.TV_NULL, FLT}
    assert any(s[0].startswith("rdfgpu::extend_kernel") for s in plan.kernel_stats()), plan.kernel_stats()


def test_every_kind_and_the_error_value(torch_cuda, gs):
    """one plan with 8 computed columns: INT, INTEGER, DECIMAL (a negative high word), FLOAT (-0.0), DOUBLE (NaN, INF), BOOLEAN, the
    error value, and values passed through as they are — payloads bit for bit"""
    cols = ec.kinds_rows()
    plan = run(torch_cuda, gs, [cols], lambda pb, t: pb.extend(t[0], [e for _, e, _ in ec.KINDS], keep=[1, 0]))
    n, c = plan.result_info()
    assert (n, c) == (len(cols[0]), 10) and plan.value_columns() == list(range(2, 10))
    ids = plan.fetch()
    assert np.array_equal(ids[0], cols[1]) and np.array_equal(ids[1], cols[0])                    # the kept columns, in the order asked for
    check_in_row_order(plan, cc.rows_of(cols), [fn for _, _, fn in ec.KINDS], first=2)
    tags = lambda q: set(plan.fetch_column_values(q)["tag"].tolist())
    assert abi.TV_INT in tags(2) and abi.TV_BOOLEAN in tags(7) and tags(8) == {abi.TV_NULL}
    dec = plan.fetch_column_values(4)
    assert ((dec["tag"] == DEC) & (dec["hi"] < 0)).any()
    flt = plan.fetch_column_values(5)
    assert ((flt["tag"] == FLT) & (flt["lo"] == 0x80000000)).any()                                # -0.0, zero-extended
    assert plan.column_values(7)[0] is True and plan.column_values(2)[1] == 1 << 30 and plan.column_values(2)[0] is None   # 5 x 2^30 is no xsd:int


# ---------------------------------------------------------------------------------------------------
# row counts
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, B - 1, B, B + 1])
def test_row_count_edges(torch_cuda, gs, n):
    """MUL(ENC_TV(a), ENC_TV(b)) over n rows: entry r is r + 1, value r the product of row r, the arrays are n long and the element
    behind each of them is untouched"""
    cols = ec.mul_table(n)
    expr, fn = ec.mul_cols(0, 1)
    plan = run(torch_cuda, gs, [cols], lambda pb, t: pb.sparql_bind(t[0], expr, "product"))
    assert plan.result_info() == (n, 3)
    ptr, length = plan.result_values(2)
    assert ptr != 0 and length == n
    if n:
        assert plan.fetch()[2].tolist() == list(range(1, n + 1))
        check_in_row_order(plan, cc.rows_of(cols), [fn], first=2)
        on_device = device_words(gs, ptr, 6 * n).view(np.int64).reshape(n, 3)
        assert on_device[:, 0].tolist() == [int(a) * int(b) for a, b in zip(*cols)] and (on_device[:, 1] == 0).all() and (on_device[:, 2] == INTEGER).all()
    assert (device_words(gs, ptr + 24 * n, 6) == GUARD).all()                                     # nothing written past record n
    entries = plan.result_device()[0][2]                                                          # (no pointers are handed out for an empty result)
    assert n == 0 or (entries != 0 and device_words(gs, entries + 4 * n, 1)[0] == GUARD)          # .. nor past entry n


def test_row_count_known_on_the_device_only(torch_cuda, gs):
    """EXTEND above an inner join, whose output is sized by a guess and counted on the device (nothing is read back): one compiled plan over
    tables of 65 and then B + 1 rows — each execution's values are its own, the arrays report the rows that were written"""
    expr, fn = ec.mul_cols(1, 2)
    plan = compiled(gs, [2, 2], lambda pb, t: pb.extend(pb.hash_join(t[0], t[1], [(0, 0)], projection=[0, 1, 3]), [expr]))
    for n in (65, B + 1):
        left, right = ec.keyed_tables(n)
        bind(torch_cuda, plan, [left, right])
        plan.execute()
        m = plan.metrics()
        # the join's output capacity (at least 1024 rows) is what the host knows of it: it was not read back, and no run was repeated
        assert m.exact_reruns == 0 and m.intermediate_rows >= 1024 + 2 * n, (m.exact_reruns, m.intermediate_rows)
        assert plan.result_info() == (n, 4)
        ptr, length = plan.result_values(3)
        assert ptr != 0 and length == n                                                           # the live rows, not the capacity
        joined = cc.join(cc.rows_of(left), cc.rows_of(right), [(0, 0)])
        cc.check_rows(ec.extend([tuple(r[c] for c in (0, 1, 3)) for r in joined], [fn]), plan, [3])
        assert sorted(plan.fetch()[3].tolist()) == list(range(1, n + 1))


# ---------------------------------------------------------------------------------------------------
# downstream
# ---------------------------------------------------------------------------------------------------
def test_having_on_a_ratio(torch_cuda, gs):
    """FILTER(ratio > 0.5) above the Q3 shape: the predicate reads the computed column through ENC_TV"""
    now, before = ec.q3_tables(300)
    plan = run(torch_cuda, gs, [now, before], lambda pb, t: pb.filter(ec.q3_plan(pb, t[0], t[1]), EBV(GT(ENC_TV(col(3)), decimal(E18 // 2))), projection=[0, 3]))
    ref = cc.having(ec.q3_reference(now, before), lambda r: cc.compare("gt", ec.raw(r[3]), (DEC, E18 // 2)), [0, 3])
    assert 20 < len(ref) < 200
    cc.check_rows(ref, plan, [1])


def payload_table(seed=6):
    """(k, a, b): 90 rows, keys 1 .. 30 three times each over; one product overflows i64 (an unbound computed value)"""
    rng = np.random.default_rng(seed)
    k = np.tile(np.arange(30, dtype=np.uint32) + 1, 3)
    a, b = rng.integers(1, 1001, 90).astype(np.uint32), rng.integers(1, 1001, 90).astype(np.uint32)
    a[6], b[6] = IDS["iMAX"], IDS["iMAX"]          # (key 7)
    return [k, a, b]


@pytest.mark.parametrize("join_type", [INNER, LEFT, SEMI, ANTI])
def test_computed_column_as_join_payload(torch_cuda, gs, join_type):
    """the computed column on the right of INNER / LEFT joins (LEFT: padding = 0) and on the left of SEMI / ANTI joins"""
    t = payload_table()
    other = [np.arange(0, 60, 2, dtype=np.uint32) + 1, np.arange(30, dtype=np.uint32) + 500]       # (k, z): the odd keys
    expr, fn = ec.mul_cols(1, 2)
    e_rows = ec.extend(cc.rows_of(t), [fn])
    if join_type in (INNER, LEFT):
        plan = run(torch_cuda, gs, [t, other], lambda pb, n: pb.hash_join(n[1], pb.extend(n[0], [expr]), [(0, 0)], join_type=join_type, projection=[0, 1, 5]))
        ref = [tuple(r[c] for c in (0, 1, 5)) for r in cc.join(cc.rows_of(other), e_rows, [(0, 0)], join_type, right_width=4)]
        cc.check_rows(ref, plan, [2])
        assert any(r[2] == UNBOUND for r in ref) and (join_type == INNER or any(r[2] == 0 for r in ref)) and len(ref) >= 45
    else:
        plan = run(torch_cuda, gs, [t, other], lambda pb, n: pb.hash_join(pb.extend(n[0], [expr]), n[1], [(0, 0)], join_type=join_type))
        ref = cc.join(e_rows, cc.rows_of(other), [(0, 0)], join_type)
        cc.check_rows(ref, plan, [3])
        assert len(ref) == 45


def test_computed_column_consumed_by_two_parents(torch_cuda, gs):
    """one EXTEND feeds two FilterExecs whose outputs are joined: both sides carry the one array's entries"""
    t = payload_table()
    expr, fn = ec.mul_cols(1, 2)
    big = lambda c: EBV(GT(ENC_TV(col(c)), integer(250000)))

    def root(pb, n):
        e = pb.extend(n[0], [expr], keep=[0, 1])
        return pb.hash_join(pb.filter(e, big(2)), pb.filter(e, EBV(GT(ENC_TV(col(1)), integer(500)))), [(0, 0), (1, 1)], projection=[0, 2, 5])
    plan = run(torch_cuda, gs, [t], root)
    e_rows = ec.extend(cc.rows_of(t), [fn], keep=[0, 1])
    l = cc.having(e_rows, lambda r: cc.compare("gt", ec.raw(r[2]), (INTEGER, 250000)))
    r_ = cc.having(e_rows, lambda r: cc.compare("gt", ec.raw(r[1]), (INTEGER, 500)))
    ref = [tuple(x[c] for c in (0, 2, 5)) for x in cc.join(l, r_, [(0, 0), (1, 1)])]
    assert 5 < len(ref) < 90
    cc.check_rows(ref, plan, [1, 2])


def test_count_sum_avg_of_a_computed_column(torch_cuda, gs):
    """a further AggregateExec over the computed column: COUNT skips the unbound product, SUM skips it, AVG of its group is the error"""
    t = payload_table()
    expr, fn = ec.mul_cols(1, 2)
    aggs = [(COUNT, 3), (SUM, 3), (AVG, 3)]
    plan = run(torch_cuda, gs, [t], lambda pb, n: pb.aggregate(pb.extend(n[0], [expr]), [0], aggs))
    ref = cc.aggregate(ec.extend(cc.rows_of(t), [fn]), [0], aggs)
    assert sum(1 for r in ref if r[3] == UNBOUND) == 1 and {r[1][1] for r in ref} == {2, 3}
    cc.check_rows(ref, plan, [1, 2, 3])


def test_extend_over_extend(torch_cuda, gs):
    """the ratio, then ROUND(ratio x 100): the upper node's program loads the lower node's values"""
    now, before = ec.q3_tables(300)
    pct, pct_fn = ec.percent(3)
    plan = run(torch_cuda, gs, [now, before], lambda pb, t: pb.sparql_bind(ec.q3_plan(pb, t[0], t[1]), pct, "percent"))
    ref = ec.extend(ec.q3_reference(now, before), [pct_fn])
    assert sum(1 for r in ref if r[4] == UNBOUND) == 100 and any(r[4] != UNBOUND and r[4][1].check(100.0) for r in ref)
    cc.check_rows(ref, plan, [1, 2, 3, 4])


def test_one_program_reads_an_aggregate_value_and_an_id_column(torch_cuda, gs):
    """MUL(count, ENC_TV(key)): a value load and a typed-value gather in one program"""
    cols = cc.sized_groups(200)
    expr, fn = ec.mul_cols(1, 0)
    plan = run(torch_cuda, gs, [cols], lambda pb, t: pb.extend(pb.aggregate(t[0], [0], [(COUNT, 1)]), [expr], keep=[0]))
    ref = ec.extend(cc.aggregate(cc.rows_of(cols), [0], [(COUNT, 1)]), [fn], keep=[0])
    assert len(ref) == 200 and all(r[1][0] == INTEGER for r in ref)
    cc.check_rows(ref, plan, [1])


# ---------------------------------------------------------------------------------------------------
# the run-time refusal, the export
# ---------------------------------------------------------------------------------------------------
def test_a_string_value_fails_the_execute_and_the_plan_stays_usable(torch_cuda, gs):
    """ENC_TV(col) over a column with one string literal among integers: the record has no room for its language / datatype, the
    execute is ERR_UNSUPPORTED; the same plan over a table without that row then answers"""
    plan = compiled(gs, [1], lambda pb, t: pb.sparql_bind(t[0], ENC_TV(col(0)), "v"))
    bind(torch_cuda, plan, [ec.string_rows(True)])
    with pytest.raises(RdfGpuError) as err:
        plan.execute()
    assert err.value.status == abi.ERR_UNSUPPORTED and "computed column" in str(err.value), err.value
    cols = ec.string_rows(False)
    bind(torch_cuda, plan, [cols])
    plan.execute()
    check_in_row_order(plan, cc.rows_of(cols), [lambda r: ec.raw(r[0])], first=1)
    assert plan.column_values(1) == cols[0].tolist()


def test_export_and_decode_terms(torch_cuda, gs):
    """rdfgpu_plan_next delivers the computed column as the {tag, lo, hi} struct child in its place, null where the entry is 0;
    decode_terms of it is refused"""
    t = payload_table()
    expr, fn = ec.mul_cols(1, 2)
    plan = run(torch_cuda, gs, [t], lambda pb, n: pb.extend(n[0], [expr], keep=[0]))
    want = [nr.bits(fn(r)) for r in cc.rows_of(t)]
    arrow = list(plan.batches())
    assert sum(len(b) for b in arrow) == 90 and all(b.type.num_fields == 2 for b in arrow)
    child = [b.field(1) for b in arrow]
    valid = np.concatenate([np.asarray(c.is_valid()) for c in child])
    tags = np.concatenate([c.field("tag").to_numpy(zero_copy_only=False) for c in child])
    los = np.concatenate([c.field("lo").to_numpy(zero_copy_only=False) for c in child])
    assert valid.tolist() == [w[0] != abi.TV_NULL for w in want] and (~valid).sum() == 1
    assert [(int(t_), int(l)) for t_, l in zip(tags[valid], los[valid])] == [(w[0], w[1]) for w in want if w[0] != abi.TV_NULL]
    assert np.concatenate([b.field(0).to_numpy(zero_copy_only=False) for b in arrow]).tolist() == t[0].tolist()
    with pytest.raises(RdfGpuError) as err:
        plan.decode_terms(1)
    assert err.value.status == abi.ERR_UNSUPPORTED and "column 1" in str(err.value) and "expression 0 of node 1" in str(err.value), err.value
