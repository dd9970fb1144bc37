"""Computed columns (abi.NODE_EXTEND) on the host side: the ABI constants, the plan builder's encoding, widths, value columns and
display, the Python reference of extend_cases.py on hand-worked rows, what its tables hold, and the compile checks as a stand-alone
program.  The GPU tests (test_gpu_extend.py) take their expected rows from that reference.  No GPU needed."""
import os
import re
import subprocess

import numpy as np

from rdf_fusion_amd import abi
from rdf_fusion_amd.engine import agg_value
from rdf_fusion_amd.plan import PlanBuilder, explain, col, integer, ENC_TV, MUL, DIV, ROUND, xsd_float, xsd_int
import aggcol_cases as cc
import extend_cases as ec
import numeric_ref as nr
from extend_cases import INT, INTEGER, DEC, FLT, DBL, BOOL, UNBOUND, IDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E18 = 10 ** 18


def _header():
    return open(os.path.join(ROOT, "include", "rdfgpu.h")).read()


def test_header_constants_match_abi_py():
    h = _header()
    assert int(re.search(r"RDFGPU_NODE_EXTEND = (\d+)", h).group(1)) == abi.NODE_EXTEND == 12
    assert int(re.search(r"RDFGPU_NODE_AGGREGATE = (\d+)", h).group(1)) == abi.NODE_AGGREGATE == 11
    assert int(re.search(r"#define RDFGPU_MAX_AGGREGATES (\d+)u", h).group(1)) == abi.MAX_AGGREGATES == 8      # bounds the computed columns too
    assert int(re.search(r"#define RDFGPU_MAX_COLUMNS (\d+)u", h).group(1)) == 16
    assert int(re.search(r"#define RDFGPU_ABI_VERSION (\d+)u", h).group(1)) == abi.ABI_VERSION == 4              # an addendum: the version stays
    k = int(re.search(r"constexpr int kExtendBlock = (\d+);", open(os.path.join(ROOT, "rdf-fusion_amd", "csrc", "kernels.hpp")).read()).group(1))
    assert k == ec.BLOCK                                                                                            # the GPU tests' row-count edges


def q3(pb):
    now, before = pb.table(0, 2, ["product", "review"]), pb.table(1, 2, ["product", "review"])
    return ec.q3_plan(pb, now, before)


def test_builder_encodes_the_node():
    pb = PlanBuilder()
    t = pb.table(0, 3, ["k", "x", "y"])
    e = pb.extend(t, [MUL(ENC_TV(col(1)), ENC_TV(col(2))), xsd_int(ENC_TV(col(0)))], keep=[2, 0], names=["xy", "ki"])
    n = pb.nodes[e]
    assert n.kind == abi.NODE_EXTEND and n.left == t and n.right == -1 and n.table_cols == 2 and n.expr_len == 0
    assert n.n_proj == 2 and pb.pool[n.proj_off:n.proj_off + 2] == [2, 0]                       # the keep list
    pairs = pb.pool[n.table_slot:n.table_slot + 4]                                              # k pairs (expr_off, expr_len)
    assert pairs[1] == 5 and pairs[3] == 3 and pairs[2] == pairs[0] + 5
    ops = [x.op for x in pb.exprs[pairs[0]:pairs[0] + pairs[1]]]
    assert ops == [abi.EX_COLUMN, abi.EX_ENC_TV, abi.EX_COLUMN, abi.EX_ENC_TV, abi.EX_MUL]
    assert [x.op for x in pb.exprs[pairs[2]:pairs[2] + pairs[3]]] == [abi.EX_COLUMN, abi.EX_ENC_TV, abi.EX_CAST]
    assert pb.width[e] == 4 and pb.names[e] == ["y", "k", "xy", "ki"] and pb.values[e] == [False, False, True, True]
    d = pb.build(e, agg_columns=True)
    assert d.flags == abi.PLAN_AGG_COLUMNS and d.value_columns == [2, 3] and d.width == 4
    f = pb.filter(e, None, projection=[3, 1])                                                    # carried like an aggregate's value column
    assert pb.values[f] == [True, False]
    default = pb.extend(t, [DIV(ENC_TV(col(1)), integer(4))])                                    # named as DataFusion prints the expression
    assert pb.names[default] == ["k", "x", "y", "DIV(ENC_TV(x), 9:4)"] and pb.nodes[default].n_proj == abi.NO_PROJECTION


def test_sparql_bind_is_extend_with_all_columns_kept():
    pb, pc = PlanBuilder(), PlanBuilder()
    expr = lambda: ROUND(MUL(ENC_TV(col(1)), integer(100)))
    b = pb.sparql_bind(pb.table(0, 2, ["p", "x"]), expr(), "pct")
    e = pc.extend(pc.table(0, 2, ["p", "x"]), [expr()], keep=None, names=["pct"])
    nb, ne = pb.nodes[b], pc.nodes[e]
    assert (nb.kind, nb.left, nb.n_proj, nb.table_cols, nb.table_slot) == (ne.kind, ne.left, ne.n_proj, ne.table_cols, ne.table_slot)
    assert nb.n_proj == abi.NO_PROJECTION and nb.table_cols == 1 and pb.pool == pc.pool
    assert pb.names[b] == ["p", "x", "pct"] and pb.values[b] == [False, False, True] and pb.width[b] == 3


def test_explain_prints_the_reference_line():
    pb = PlanBuilder()
    e = q3(pb)
    lines = explain(pb, e, agg_columns=True)
    assert lines[0] == ("ProjectionExec: expr=[product@0 as product, monthCount@1 as monthCount, monthBeforeCount@2 as monthBeforeCount, "
                        "DIV(xsd:float(monthCount@1), monthBeforeCount@2) as ratio]")
    assert lines[1] == "  ProjectionExec" and lines[2].startswith("    HashJoinExec: mode=CollectLeft, join_type=Left, on=[(product@0, product@0)]")
    assert pb.values[e] == [False, True, True, True] and pb.build(e, agg_columns=True).value_columns == [1, 2, 3]
    # an id column keeps its ENC_TV: it is the gather that makes the id a value
    t = pb.table(2, 2, ["p", "price"])
    b = pb.sparql_bind(t, MUL(ENC_TV(col(1)), integer(2)), "twice")
    assert explain(pb, b)[0] == "ProjectionExec: expr=[p@0 as p, price@1 as price, MUL(ENC_TV(price@1), 9:2) as twice]"


def test_the_reference_on_hand_worked_rows():
    bits = lambda v: nr.bits(v)
    div, flt = ec.ratio(0, 1)[1], lambda v: (FLT, np.float32(v))
    assert bits(div((3, 4))) == bits(flt(0.75))                                                  # DIV(xsd:float(3), 4) is the float 0.75
    idiv = lambda r: nr.binary(abi.EX_DIV, ec.raw(r[0]), ec.raw(r[1]))
    assert idiv((6, 4)) == (DEC, 15 * E18 // 10)                                                 # DIV(6, 4) of integers is the decimal 1.5
    assert idiv((1, IDS["i0"])) == nr.ERR                                                        # DIV(1, 0) of integers is the error value
    inf = div((1, IDS["i0"]))
    assert inf[0] == FLT and np.isposinf(inf[1])                                                 # DIV of a float by 0 is +INF
    assert ec.cast(INT, (INTEGER, 1 << 31)) == nr.ERR and ec.cast(INT, (INTEGER, (1 << 31) - 1)) == (INT, (1 << 31) - 1)   # xsd:int of 2^31
    rows = ec.extend([(7, (INTEGER, 3), (INTEGER, 4)), (9, (INTEGER, 1), 0)], [ec.ratio(1, 2)[1]], keep=[0, 2])
    assert rows[0][:2] == (7, (INTEGER, 4)) and rows[0][2][0] == FLT and rows[0][2][1].check(0.75) and not rows[0][2][1].check(0.7500001)
    assert rows[1] == (9, 0, UNBOUND)                                                            # a padded count: the ratio is unbound
    again = ec.extend(rows, [ec.percent(2)[1]])
    assert again[0][3][0] == FLT and again[0][3][1].check(75.0) and again[1][3] == UNBOUND       # EXTEND over EXTEND reads the cell back
    assert ec.cell((BOOL, 1))[1].check(agg_value(BOOL, 1)) and ec.cell((INT, -5))[1].check(agg_value(INT, -5 & ((1 << 64) - 1)))
    assert ec.cell((FLT, np.float32(-0.0)))[1].check(-0.0) and not ec.cell((FLT, np.float32(-0.0)))[1].check(0.0)
    assert ec.cell((DBL, np.float64("nan")))[1].check(float("nan"))


def test_the_tables_hold_what_the_gpu_tests_need():
    rows = cc.rows_of(ec.kinds_rows())
    by_col = {name: [fn(r) for r in rows] for name, _, fn in ec.KINDS}
    assert len(ec.KINDS) == abi.MAX_AGGREGATES
    tags = {name: {v[0] for v in vs} for name, vs in by_col.items()}
    assert INT in tags["int"] and abi.TV_NULL in tags["int"]                                     # 2 x 2^30 = 2^31: the error value
    assert INTEGER in tags["integer"] and abi.TV_NULL in tags["integer"]                         # 2^32 x 2^32 overflows
    assert any(v[0] == DEC and v[1] < 0 and nr.bits(v)[2] < 0 for v in by_col["decimal"])        # a negative high word
    assert abi.TV_NULL in tags["decimal"]                                                        # DIV by an integer zero
    assert any(v[0] == FLT and nr.bits(v)[1] == 0x80000000 for v in by_col["float"])             # -0.0 from CEIL(-0.5)
    assert any(v[0] == DBL and np.isnan(v[1]) for v in by_col["double"]) and any(v[0] == DBL and np.isinf(v[1]) for v in by_col["double"])
    assert {v for v in by_col["boolean"]} >= {(BOOL, 0), (BOOL, 1), nr.ERR}
    assert tags["error"] == {abi.TV_NULL}
    assert {DEC, FLT, DBL, INTEGER, INT, abi.TV_NULL} <= tags["as is"]
    assert IDS["str"] not in ec.kinds_rows()[0] and IDS["str"] not in ec.kinds_rows()[1]         # the run-time refusal has a test of its own
    assert IDS["str"] in ec.string_rows(True)[0] and IDS["str"] not in ec.string_rows(False)[0]
    now, before = ec.q3_tables()
    ref = ec.q3_reference(now, before)
    assert len(ref) == 300 and sum(1 for r in ref if r[3] == UNBOUND) == 100 and all(r[3] == UNBOUND for r in ref if r[2] == 0)
    assert any(r[3] != UNBOUND and r[3][1].check(0.5) for r in ref) or len({r[3][1].key for r in ref if r[3] != UNBOUND}) > 5
    l, r = ec.keyed_tables(ec.BLOCK + 1)
    assert len(set(l[0].tolist())) == ec.BLOCK + 1 and sorted(l[0].tolist()) == sorted(r[0].tolist())


def test_the_compile_checks_build_and_pass_as_a_stand_alone_program():
    """tests/host/extend_compile_checks.cpp — what compiles under the flag, every refusal of the node with its code and its text's key
    words, how an EXTEND over an EXTEND and over an AGGREGATE types its value loads — built from the library's own plan_compile.cpp and
    run without a device (the same target with SANITIZE=1 is the sanitizer build)"""
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "rdf-fusion_amd", "csrc"), "-s", "host-checks-extend"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("0 failure(s)"), out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.count(" ok ") >= 30 and "FAIL" not in out.stdout
