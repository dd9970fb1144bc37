"""Aggregate values as columns (abi.PLAN_AGG_COLUMNS) on the host side: the ABI constants and symbols, the plan builder's flag word,
widths, value columns and display, the HAVING lowering, and the Python reference of aggcol_cases.py on small hand-worked inputs.  The GPU
tests (test_gpu_agg_columns.py) take their expected rows from that reference.  No GPU needed."""
import os
import re
import subprocess
from fractions import Fraction

from rdf_fusion_amd import abi
from rdf_fusion_amd.plan import PlanBuilder, explain, col, integer, decimal, EBV, GT, MUL, ENC_TV
import aggcol_cases as cc
from aggcol_cases import STAR, COUNT, SUM, AVG, UNBOUND, E18, compare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTEGER, DEC = abi.TV_INTEGER, abi.TV_DECIMAL


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rdfgpu.h")).read(), flags=re.S)


def test_header_constants_match_abi_py():
    h = _header()
    assert int(re.search(r"#define RDFGPU_PLAN_AGG_COLUMNS (\d+)u", h).group(1)) == abi.PLAN_AGG_COLUMNS == 2
    assert int(re.search(r"#define RDFGPU_PLAN_ALLOW_OPAQUE (\d+)u", h).group(1)) == abi.PLAN_ALLOW_OPAQUE == 1
    assert int(re.search(r"#define RDFGPU_ABI_VERSION (\d+)u", h).group(1)) == abi.ABI_VERSION == 4      # an addendum: the version stays
    assert int(re.search(r"RDFGPU_EX__COUNT", h).start()) > 0


def test_the_new_symbols_exist():
    import rdf_fusion_amd as rf
    lib = rf.load_library()
    for f in ("rdfgpu_plan_result_values", "rdfgpu_plan_result_values_fetch"):
        assert f in abi.EXPORTED_SYMBOLS and f + "(" in _header() and hasattr(lib, f)


def q3_like(pb):
    t = pb.table(0, 3, ["product", "review", "price"])
    a = pb.aggregate(t, [0], [(abi.AGG_COUNT, 1), (abi.AGG_AVG, 2)])
    return t, a


def test_builder_flag_word_widths_and_value_columns():
    pb = PlanBuilder()
    t, a = q3_like(pb)
    assert pb.width[a] == 3 and pb.names[a] == ["product", "COUNT(review)", "AVG(price)"] and pb.values[a] == [False, True, True]
    h = pb.sparql_having(a, EBV(GT(ENC_TV(col(1)), integer(9))), projection=[0, 2])
    assert pb.width[h] == 2 and pb.names[h] == ["product", "AVG(price)"] and pb.values[h] == [False, True]
    g = pb.aggregate(t, [], [(abi.AGG_AVG, 2)])
    x = pb.cross_join(h, g)
    assert pb.width[x] == 3 and pb.values[x] == [False, True, True]
    s = pb.hash_join(t, a, [(0, 0)], join_type=abi.JOIN_LEFT_SEMI)
    assert pb.values[s] == [False, False, False]                       # a semi join hands on its left input only
    j = pb.hash_join(t, a, [(0, 0)], projection=[5, 1])
    assert pb.values[j] == [True, False] and pb.names[j] == ["AVG(price)", "review"]
    off = pb.build(x)
    assert off.flags == 0 and off.desc.flags == 0 and off.value_columns == []
    on = pb.build(x, agg_columns=True)
    assert on.flags == abi.PLAN_AGG_COLUMNS and on.desc.flags == 2 and on.value_columns == [1, 2] and on.width == 3
    assert pb.build(a, agg_columns=True).n_columns[a] == 3


def test_sparql_having_encodes_a_filter():
    pb = PlanBuilder()
    _, a = q3_like(pb)
    h = pb.sparql_having(a, EBV(GT(ENC_TV(col(1)), integer(9))))
    n = pb.nodes[h]
    assert n.kind == abi.NODE_FILTER and n.left == a and n.n_proj == abi.NO_PROJECTION and n.expr_len == 5
    ops = [e.op for e in pb.exprs[n.expr_off:n.expr_off + n.expr_len]]
    assert ops == [abi.EX_COLUMN, abi.EX_ENC_TV, abi.EX_LIT_TV, abi.EX_GT, abi.EX_EBV]     # INT64_AS_TERM(count) is ENC_TV of the column
    assert "Q3" in PlanBuilder.sparql_having.__doc__ and "Q6" in PlanBuilder.sparql_having.__doc__
    assert ":17" in PlanBuilder.sparql_having.__doc__ and ":6" in PlanBuilder.sparql_having.__doc__


def test_explain_prints_value_columns():
    pb = PlanBuilder()
    t, a = q3_like(pb)
    h = pb.sparql_having(a, EBV(GT(ENC_TV(col(2)), MUL(ENC_TV(col(1)), decimal(15 * E18 // 10)))))
    plain = "AggregateExec: mode=Single, gby=[product@0 as product], aggr=[COUNT(review@1), AVG(price@2)]"
    assert explain(pb, h)[1] == "  " + plain                              # without the flag: today's line
    pb.build(h, agg_columns=True)
    assert explain(pb, h)[1] == "  " + plain                              # (what was built does not change what is printed)
    lines = explain(pb, h, agg_columns=True)
    assert lines[0] == "FilterExec: EBV(GT(ENC_TV(AVG(price)@2), MUL(ENC_TV(COUNT(review)@1), 7:1500000000000000000)))"
    assert lines[1] == "  " + plain + ", values=[COUNT(review)@1, AVG(price)@2]"
    assert explain(pb, h, agg_columns=False)[1] == "  " + plain
    d = pb.aggregate(t, [1])                                               # no aggregates: no value columns to print
    assert explain(pb, d, agg_columns=True)[0] == "AggregateExec: mode=Single, gby=[review@1 as review], aggr=[]"


def test_the_reference_on_hand_worked_rows():
    rows = [(7, 2), (7, 4), (9, 1), (9, cc.IDS["iMAX"]), (9, cc.IDS["iMAX"]), (11, 0)]
    a = cc.aggregate(rows, [0], [(STAR, None), (SUM, 1), (AVG, 1), (COUNT, 1)])
    assert a == [(7, (INTEGER, 2), (INTEGER, 6), (DEC, 3 * E18), (INTEGER, 2)),
                 (9, (INTEGER, 3), UNBOUND, (DEC, ((1 << 64) - 1) * E18 // 3), (INTEGER, 3)),     # the SUM is past i64, the AVG is not
                 (11, (INTEGER, 1), (INTEGER, 0), UNBOUND, (INTEGER, 0))]
    assert cc.having(a, lambda r: compare("gt", r[2], (INTEGER, 5))) == a[:1]                      # an unbound value drops the row
    assert cc.having(a, lambda r: not cc.bound(r[2]), [0]) == [(9,)]
    up = cc.aggregate(a, [], [(SUM, 1), (COUNT, 2), (AVG, 2), (AVG, 1)])
    assert up == [((INTEGER, 6), (INTEGER, 2), UNBOUND, (DEC, 2 * E18))]                          # SUM of COUNTs = the rows; AVG over an unbound: error
    left = cc.join(a, [(7, (INTEGER, 1))], [(0, 0)], abi.JOIN_LEFT, right_width=2)
    assert [r[5:] for r in left] == [(7, (INTEGER, 1)), (0, 0), (0, 0)]
    assert len(cc.join(a, a, [(0, 0)], abi.JOIN_LEFT_ANTI, lambda r: compare("gt", r[1], (INTEGER, 2)))) == 2
    assert compare("gt", (DEC, 15 * E18 // 10), (INTEGER, 1)) is True and compare("gt", UNBOUND, (INTEGER, 1)) is None
    assert cc.mul((DEC, 3333333333333333333), (DEC, 15 * E18 // 10)) == (abi.TV_NULL, None)      # 18 fraction digits x 1.5: checked_mul refuses
    assert cc.mul((DEC, 25 * E18 // 10), (DEC, 15 * E18 // 10)) == (DEC, 375 * E18 // 100)
    assert Fraction(375, 100) == cc.exact((DEC, 375 * E18 // 100))


def test_the_tables_hold_what_the_gpu_tests_need():
    cols = cc.sized_groups(257)
    assert len(set(cols[0].tolist())) == 257 and 0 not in cols[0]
    ref = cc.aggregate(cc.rows_of(cols), [0], [(STAR, None)])
    assert {r[1][1] for r in ref} == {1, 2, 3, 4, 5}
    k = cc.aggregate(cc.rows_of(cc.kinds_table()), [0], [(SUM, 1)])
    assert [r[1][0] for r in k] == [INTEGER, DEC, abi.TV_FLOAT, abi.TV_DOUBLE, abi.TV_NULL, INTEGER] and k[1][1][1] < 0
    o = cc.aggregate(cc.rows_of(cc.overflow_table()), [0], [(SUM, 1)])
    assert sum(1 for r in o if r[1] == UNBOUND) == 8 and len(o) == 40
    per = cc.aggregate(cc.rows_of(cc.review_table()), [0], [(AVG, 1)])
    assert any(r[1] == UNBOUND for r in per) and len(per) == 300
    two = cc.two_level_table()
    inner = cc.aggregate(cc.rows_of(two), [0, 1], [(STAR, None)])
    assert cc.aggregate(inner, [], [(SUM, 2)]) == [((INTEGER, len(two[0])),)]


def test_the_compile_checks_build_and_pass_as_a_stand_alone_program():
    """tests/host/plan_compile_checks.cpp — what compiles under the flag, what is refused with which text, the kind errors — built from
    the library's own plan_compile.cpp and run without a device (the same target with SANITIZE=1 is the sanitizer build)"""
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "rdf-fusion_amd", "csrc"), "-s", "host-checks"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("0 failure(s)"), out.stdout[-2000:] + out.stderr[-2000:]
