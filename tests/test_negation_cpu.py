"""LeftSemi / LeftAnti joins on the host side: the ABI constants, the plan builder's output schema for them, the
EXISTS / NOT EXISTS / MINUS lowering helpers and their plan display.  No GPU needed."""
import json
import os
import re

import pytest

from rdf_fusion_amd import abi
from rdf_fusion_amd.plan import PlanBuilder, MemIndexScanInstruction as I, explain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "rdfgpu.h")).read()


def test_header_join_types_and_abi_version_match_abi_py():
    h = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert int(re.search(r"#define RDFGPU_ABI_VERSION (\d+)u", h).group(1)) == abi.ABI_VERSION == 4
    assert int(re.search(r"RDFGPU_JOIN_LEFT_SEMI = (\d+)", h).group(1)) == abi.JOIN_LEFT_SEMI == 2
    assert int(re.search(r"RDFGPU_JOIN_LEFT_ANTI = (\d+)", h).group(1)) == abi.JOIN_LEFT_ANTI == 3
    assert "NO_SEMI_LDS" in abi.OPTION_NAMES


def _three(pb, a, b, names_a=("x", "y", "z"), names_b=("y", "w")):
    return pb.table(0, a, list(names_a)[:a]), pb.table(1, b, list(names_b)[:b])


@pytest.mark.parametrize("jt", [abi.JOIN_LEFT_SEMI, abi.JOIN_LEFT_ANTI])
def test_semi_and_anti_joins_output_the_left_columns(jt):
    pb = PlanBuilder()
    l, r = _three(pb, 3, 2)
    h = pb.hash_join(l, r, on=[(1, 0)], join_type=jt)
    assert pb.width[h] == 3 and pb.names[h] == ["x", "y", "z"]
    hp = pb.hash_join(l, r, on=[(1, 0)], join_type=jt, projection=[2, 0])
    assert pb.width[hp] == 2 and pb.names[hp] == ["z", "x"]
    n = pb.nested_loop_join(l, r, jt)
    assert pb.width[n] == 3 and pb.names[n] == ["x", "y", "z"]
    npj = pb.nested_loop_join(l, r, jt, projection=[1])
    assert pb.width[npj] == 1 and pb.names[npj] == ["y"]
    # the inner join keeps both sides
    assert pb.width[pb.hash_join(l, r, on=[(1, 0)])] == 5


def _prog(pb, node):
    n = pb.nodes[node]
    return [(e.op, e.u) for e in pb.exprs[n.expr_off:n.expr_off + n.expr_len]]


@pytest.mark.parametrize("negate", [False, True])
def test_sparql_exists_without_shared_variables_is_a_filterless_nested_loop_join(negate):
    pb = PlanBuilder()
    outer, inner = pb.table(0, 2, ["a", "b"]), pb.table(1, 1, ["c"])
    j = pb.sparql_exists(outer, inner, negate=negate)
    n = pb.nodes[j]
    assert n.kind == abi.NODE_NESTED_LOOP_JOIN and n.expr_len == 0
    assert n.join_type == (abi.JOIN_LEFT_ANTI if negate else abi.JOIN_LEFT_SEMI)
    assert pb.names[j] == ["a", "b"]


@pytest.mark.parametrize("negate", [False, True])
def test_sparql_exists_with_non_nullable_shared_variables_is_a_hash_join_on_sorted_keys(negate):
    pb = PlanBuilder()
    outer, inner = pb.table(0, 3, ["z", "b", "a"]), pb.table(1, 3, ["a", "q", "z"])
    j = pb.sparql_exists(outer, inner, negate=negate)
    n = pb.nodes[j]
    assert n.kind == abi.NODE_HASH_JOIN and n.expr_len == 0
    assert n.join_type == (abi.JOIN_LEFT_ANTI if negate else abi.JOIN_LEFT_SEMI)
    # shared = {a, z}, sorted: a first
    assert [(n.left_keys[k], n.right_keys[k]) for k in range(n.n_keys)] == [(2, 0), (0, 2)]
    assert pb.names[j] == ["z", "b", "a"]


def test_sparql_exists_with_a_nullable_shared_variable_is_is_compatible_over_every_shared_variable():
    pb = PlanBuilder()
    outer, inner = pb.table(0, 2, ["a", "z"]), pb.table(1, 2, ["z", "a"])
    j = pb.sparql_exists(outer, inner, negate=True, nullable=("z",))
    n = pb.nodes[j]
    assert n.kind == abi.NODE_NESTED_LOOP_JOIN and n.join_type == abi.JOIN_LEFT_ANTI
    # [left cols, right cols]: a@0 z@1 | z@2 a@3 ; sorted shared = a, z
    assert _prog(pb, j) == [(abi.EX_COLUMN, 0), (abi.EX_COLUMN, 3), (abi.EX_IS_COMPATIBLE, 0),
                            (abi.EX_COLUMN, 1), (abi.EX_COLUMN, 2), (abi.EX_IS_COMPATIBLE, 0), (abi.EX_AND, 0)]


def test_sparql_minus_lowering_in_all_three_cases():
    pb = PlanBuilder()
    l = pb.table(0, 2, ["a", "b"])
    # no shared variable: left unchanged (minus/rewrite.rs:62-64)
    assert pb.sparql_minus(l, pb.table(1, 1, ["c"])) == l
    # shared, not nullable: anti hash join
    j = pb.sparql_minus(l, pb.table(1, 2, ["c", "b"]))
    n = pb.nodes[j]
    assert n.kind == abi.NODE_HASH_JOIN and n.join_type == abi.JOIN_LEFT_ANTI and n.expr_len == 0
    assert [(n.left_keys[k], n.right_keys[k]) for k in range(n.n_keys)] == [(1, 1)]
    assert pb.names[j] == ["a", "b"]
    # shared, nullable: IS_COMPATIBLE AND (BOUND(l) AND BOUND(r))
    j = pb.sparql_minus(l, pb.table(1, 2, ["c", "b"]), nullable=("b",))
    n = pb.nodes[j]
    assert n.kind == abi.NODE_NESTED_LOOP_JOIN and n.join_type == abi.JOIN_LEFT_ANTI
    assert _prog(pb, j) == [(abi.EX_COLUMN, 1), (abi.EX_COLUMN, 3), (abi.EX_IS_COMPATIBLE, 0),
                            (abi.EX_COLUMN, 1), (abi.EX_BOUND, 0), (abi.EX_COLUMN, 3), (abi.EX_BOUND, 0), (abi.EX_AND, 0),
                            (abi.EX_AND, 0)]
    # two shared variables, one nullable: the OR over both BOUND pairs
    pb2 = PlanBuilder()
    l2 = pb2.table(0, 2, ["a", "b"])
    j2 = pb2.sparql_minus(l2, pb2.table(1, 2, ["b", "a"]), nullable=("a",))
    ops = [op for op, _ in _prog(pb2, j2)]
    assert ops.count(abi.EX_IS_COMPATIBLE) == 2 and ops.count(abi.EX_BOUND) == 4 and ops.count(abi.EX_OR) == 1
    assert ops[-1] == abi.EX_AND


def test_plan_display_names_semi_and_anti_joins():
    pb = PlanBuilder()
    l = pb.data_source([I.traverse(), I.scan("s"), I.traverse(5), I.scan("o")])
    r = pb.data_source([I.traverse(), I.scan("s"), I.traverse(6), I.scan("v")])
    j = pb.sparql_exists(l, r, negate=False)
    lines = explain(pb, pb.hash_join(j, r, on=[(0, 0)], join_type=abi.JOIN_LEFT_ANTI, projection=[1]), choose_index=lambda ins: abi.GSPO)
    assert lines[0].startswith("HashJoinExec: mode=CollectLeft, join_type=LeftAnti, on=[(s@0, s@0)], projection=[o@1]")
    assert lines[1].startswith("  HashJoinExec: mode=CollectLeft, join_type=LeftSemi, on=[(s@0, s@0)]")
    pb2 = PlanBuilder()
    a, b = pb2.table(0, 1, ["a"]), pb2.table(1, 1, ["b"])
    assert explain(pb2, pb2.sparql_exists(a, b, negate=True))[0] == "NestedLoopJoinExec: join_type=LeftAnti"


def test_negation_fixture_transcribes_the_reference_vectors():
    with open(os.path.join(ROOT, "tests", "golden", "negation_kats.json")) as f:
        k = json.load(f)
    assert [c["name"] for c in k["cases"]] == ["values_in_filter_exists", "values_in_filter_not_exists", "subquery_in_filter_not_exists"]
    assert all(c["result_file"] == "values_in_filter_exists.srx" for c in k["cases"])
    assert k["expected"]["rows"] == [["http://example.com/a"]]
