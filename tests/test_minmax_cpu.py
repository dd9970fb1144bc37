"""MIN / MAX of AggregateExec on the host side: the constants, the hand-written cases against the device's rule, the proof by enumeration
that the rule's answer is one the reference's accumulator gives for some order of the same rows, the plan builder's encoding and display,
and the compile checks as a stand-alone program.  The GPU tests (test_gpu_minmax.py) take every expectation from
minmax_cases.device_rule.  No GPU needed."""
import os
import re
import subprocess

import pytest

from rdf_fusion_amd import abi
from rdf_fusion_amd.plan import PlanBuilder, explain, col, ENC_TV, MUL, Expr
import agg_cases as ac
import minmax_cases as mc
from minmax_cases import MIN, MAX, ERR, UNSUPPORTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_agree():
    h = open(os.path.join(ROOT, "include", "rdfgpu.h")).read()
    assert int(re.search(r"RDFGPU_AGG_MIN = (\d+)", h).group(1)) == abi.AGG_MIN == 6
    assert int(re.search(r"RDFGPU_AGG_MAX = (\d+)", h).group(1)) == abi.AGG_MAX == 7
    assert int(re.search(r"#define RDFGPU_ABI_VERSION (\d+)u", h).group(1)) == abi.ABI_VERSION == 4              # an addendum: the version stays
    assert abi.AGG_NAMES[abi.AGG_MIN] == "MIN" and abi.AGG_NAMES[abi.AGG_MAX] == "MAX"
    # the header no longer lists MIN / MAX among what is refused outright
    refused = re.search(r"Not on the device — refused with RDFGPU_ERR_UNSUPPORTED at compile, never answered differently:(.*?)\*/", h, re.S).group(1)
    assert "SAMPLE" in refused and "GROUP_CONCAT" in refused and not re.search(r"\bMIN\b|\bMAX\b", refused.split("RDFGPU_MAX")[0])
    reserved = re.search(r"/\* reserved, RDFGPU_ERR_UNSUPPORTED at compile \*/(.*?)\};", h, re.S).group(1)
    assert "RDFGPU_AGG_SAMPLE" in reserved and "RDFGPU_AGG_MIN" not in reserved and "RDFGPU_AGG_MAX" not in reserved
    k = open(os.path.join(ROOT, "rdf-fusion_amd", "csrc", "kernels.hpp")).read()
    assert int(re.search(r"constexpr u32 kAggMinMaxWords = (\d+);", k).group(1)) == mc.MINMAX_WORDS
    assert int(re.search(r"constexpr u32 kAggSumWords = (\d+);", k).group(1)) == ac.SUM_WORDS                     # unchanged
    assert int(re.search(r"constexpr size_t kAggLdsBytes = (\d+);", k).group(1)) == ac.LDS_BYTES
    assert mc.MINMAX_WORDS <= ac.SUM_WORDS                                                                        # kAggMaxWords still bounds a node's words
    e = open(os.path.join(ROOT, "rdf-fusion_amd", "csrc", "expr_device.hpp")).read()
    bits = {name: int(v) for name, v in re.findall(r"constexpr uint32_t (kRt\w+) = (\d+)u;", e)}
    assert bits["kRtMinMaxKind"] == mc.RT_MINMAX_KIND and sorted(bits.values()) == [4, 8, 16, 32, 64, 128]         # a bit of its own


@pytest.mark.parametrize("case", mc.CASES, ids=lambda c: c.name)
def test_the_rule_gives_the_hand_written_result(case):
    values = [mc.val(i) for i in case.ids]
    assert mc.same_result(mc.device_rule(values, MIN), case.min), mc.device_rule(values, MIN)
    assert mc.same_result(mc.device_rule(values, MAX), case.max), mc.device_rule(values, MAX)


def check_is_an_answer(values, fn):
    rule = mc.device_rule(values, fn)
    answers = mc.reference_answers(values, fn)
    assert any(mc.same_result(rule, a) for a in answers), (values, fn, rule, answers)
    if len(answers) == 1:
        assert mc.same_result(rule, answers[0])
    return len(answers)


@pytest.mark.parametrize("case", [c for c in mc.ANSWERED if len(c.ids) <= 6], ids=lambda c: c.name)
def test_hand_written_groups_are_answers_of_the_reference(case):
    values = [mc.val(i) for i in case.ids]
    for fn in (MIN, MAX):
        check_is_an_answer(values, fn)


def test_seeded_groups_are_answers_of_the_reference():
    """2000 groups of 1 to 5 values drawn from every numeric id, the NaNs and the unbound id: over all orders of its rows the reference
    gives a set of answers; the rule's is one of them, and the only one where there is only one"""
    groups = mc.seeded_groups()
    assert len(groups) == 2000 and {len(g) for g in groups} == {1, 2, 3, 4, 5}
    split = 0
    for g in groups:
        values = [mc.val(i) for i in g]
        for fn in (MIN, MAX):
            split += check_is_an_answer(values, fn) > 1
    assert split > 100, "the draw holds too few groups whose reference answer depends on the order"


def test_the_reference_depends_on_order_where_the_header_says_so():
    v = lambda name: mc.val(mc.IDS[name])
    assert mc.reference_accumulator([ERR, v("i3")], MIN) == ERR and mc.reference_accumulator([v("i3"), ERR], MIN) == v("i3")     # min.rs:42-53
    assert mc.is_nan(mc.reference_accumulator([v("fNaN"), v("i3")], MAX)) and mc.reference_accumulator([v("i3"), v("fNaN")], MAX) == v("i3")
    # equal after the cast: whichever comes first stays
    assert mc.reference_accumulator([v("i2^24+1"), v("f2^24")], MAX) == v("i2^24+1") and mc.reference_accumulator([v("f2^24"), v("i2^24+1")], MAX) == v("f2^24")
    assert mc.partial_cmp(v("i2^24+1"), v("f2^24")) == 0 and mc.partial_cmp(v("i2^53+1"), v("g2^53")) == 0
    assert mc.partial_cmp(v("dE18"), v("i1")) == 0 and mc.partial_cmp(v("f-0"), v("g+0")) == 0 and mc.partial_cmp(v("gNaN"), v("i1")) is None
    assert mc.partial_cmp(v("dHI+1"), v("dHI+2")) == -1 and mc.partial_cmp(v("d-HI-1"), v("dMIN")) == 1


def test_builder_encodes_min_and_max():
    pb = PlanBuilder()
    t = pb.table(0, 3, ["k", "x", "y"])
    a = pb.aggregate(t, [0], [(MIN, 1), (MAX, MUL(ENC_TV(col(1)), ENC_TV(col(2))))])
    n = pb.nodes[a]
    assert (n.kind, n.n_keys, n.table_cols) == (abi.NODE_AGGREGATE, 1, 2)
    assert pb.pool[n.table_slot:n.table_slot + 2] == [MIN, 1]
    fn, word = pb.pool[n.table_slot + 2:n.table_slot + 4]
    assert fn == MAX and word & abi.AGG_INPUT_EXPR
    off, ln = pb.pool[word & ~abi.AGG_INPUT_EXPR], pb.pool[(word & ~abi.AGG_INPUT_EXPR) + 1]
    assert ln == 5 and pb.exprs[off + ln - 1].op == abi.EX_MUL
    assert pb.names[a] == ["k", "MIN(x)", "MAX(MUL(ENC_TV(x), ENC_TV(y)))"] and pb.values[a] == [False, True, True]
    b = pb.aggregate(a, [], [(MAX, 1)])                                   # over a value column: a plain column in the description
    assert pb.pool[pb.nodes[b].table_slot:pb.nodes[b].table_slot + 2] == [MAX, 1] and pb.names[b] == ["MAX(MIN(x))"]
    assert pb.build(b, agg_columns=True).value_columns == [0] and pb.build(b, agg_columns=True).flags == abi.PLAN_AGG_COLUMNS


def test_explain_prints_min_and_max():
    pb = PlanBuilder()
    root = mc.q5_plan(pb, pb.table(0, 3, ["country", "product", "review"]))
    text = "\n".join(explain(pb, root, agg_columns=True))
    assert "gby=[country@0 as country], aggr=[MAX(COUNT(review)@2)], values=[MAX(COUNT(review))@1]" in text, text
    assert "filter=EBV(EQ(ENC_TV(COUNT(review)@0), ENC_TV(MAX(COUNT(review))@1)))" in text, text
    pb = PlanBuilder()
    root = mc.q6_plan(pb, pb.table(0, 2, ["reviewer", "score"]))
    text = "\n".join(explain(pb, root, agg_columns=True))
    assert "aggr=[AVG(score@1), MIN(AVG(score)@2)], values=[AVG(score)@1, MIN(AVG(score))@2]" in text, text
    pb = PlanBuilder()
    a = pb.aggregate(pb.table(0, 2, ["k", "x"]), [0], [(MIN, MUL(ENC_TV(col(1)), ENC_TV(col(1))))])
    assert "aggr=[MIN(MUL(ENC_TV(x@1), ENC_TV(x@1)))], values=[MIN(MUL(ENC_TV(x), ENC_TV(x)))@1]" in "\n".join(explain(pb, a, agg_columns=True))


def test_compile_checks_run_as_a_stand_alone_program():
    """tests/host/minmax_compile_checks.cpp — with the flag MIN / MAX compile over an id column, a value column and an expression, also
    under a join; without it the old status and text; SAMPLE / GROUP_CONCAT, pattern ops and a value column as a key stay refused"""
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "rdf-fusion_amd", "csrc"), "-s", "host-checks-minmax"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "\n0 failure(s)" in out.stdout and "FAIL" not in out.stdout, out.stdout[-4000:]
