"""SortExec (abi.NODE_SORT) on the host side: the ABI constants, the plan builder's encoding and display, the sharded path's refusal, the
Python sort key of sort_cases.py on hand-written orders, and the compile checks as a stand-alone program.  The GPU tests
(test_gpu_sort.py) take their expected row sequences from sort_cases.reference.  No GPU needed."""
import os
import re
import subprocess

import pytest

from rdf_fusion_amd import abi, sharding
from rdf_fusion_amd.plan import PlanBuilder, explain
import extend_cases as ec
import sort_cases as sc
from sort_cases import IDS, BY_ID, BY_TERM, BY_DOUBLE, BY_VALUE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I2 = 2          # id 2 is the xsd:integer 2


def test_header_constants_match_abi_py():
    h = open(os.path.join(ROOT, "include", "rdfgpu.h")).read()
    assert int(re.search(r"RDFGPU_NODE_SORT = (\d+)", h).group(1)) == abi.NODE_SORT == 13
    assert int(re.search(r"RDFGPU_SORT_BY_VALUE = (\d+)", h).group(1)) == abi.SORT_BY_VALUE == 3
    assert int(re.search(r"#define RDFGPU_SORT_DESC (0x[0-9a-f]+)u", h).group(1), 16) == abi.SORT_DESC == 0x100
    assert int(re.search(r"#define RDFGPU_ABI_VERSION (\d+)u", h).group(1)) == abi.ABI_VERSION == 4              # an addendum: the version stays
    assert (abi.SORT_BY_ID, abi.SORT_BY_TERM, abi.SORT_BY_DOUBLE) == (0, 1, 2) and abi.NODE_TOPK == 8            # what was there is unchanged
    k = open(os.path.join(ROOT, "rdf-fusion_amd", "csrc", "kernels.hpp")).read()
    assert int(re.search(r"constexpr u32 kSortTile = (\d+);", k).group(1)) == sc.T                                # the GPU tests' size edges
    assert int(re.search(r"constexpr u32 kSortMaxWords = (\d+);", k).group(1)) == sc.MAX_WORDS
    assert int(re.search(r"constexpr u32 kSortValueWords = (\d+);", k).group(1)) == 4


def q3_sorted(pb):
    now, before = pb.table(0, 2, ["product", "review"]), pb.table(1, 2, ["product", "review"])
    return pb.sparql_order_by(ec.q3_plan(pb, now, before), [(3, True), (0, False)], limit=10)


def test_builder_encodes_the_node():
    pb = PlanBuilder()
    t = pb.table(0, 3, ["k", "x", "y"])
    s = pb.sort(t, [(1, BY_DOUBLE, True), (0, BY_ID, False)], fetch=7, projection=[2, 0])
    n = pb.nodes[s]
    assert (n.kind, n.left, n.right, n.n_keys, n.table_cols) == (abi.NODE_SORT, t, -1, 2, 7)
    assert list(n.left_keys)[:2] == [1, 0] and list(n.right_keys)[:2] == [BY_DOUBLE | abi.SORT_DESC, BY_ID]
    assert n.n_proj == 2 and pb.pool[n.proj_off:n.proj_off + 2] == [2, 0] and pb.width[s] == 2 and pb.names[s] == ["y", "k"]
    plain = pb.sort(t, [(0, BY_ID, False)])
    assert pb.nodes[plain].table_cols == 0 and pb.nodes[plain].n_proj == abi.NO_PROJECTION and pb.width[plain] == 3   # no fetch: all rows


def test_order_by_picks_by_value_for_value_columns_and_carries_them():
    pb = PlanBuilder()
    s = q3_sorted(pb)
    n = pb.nodes[s]
    assert list(n.left_keys)[:2] == [3, 0] and list(n.right_keys)[:2] == [BY_VALUE | abi.SORT_DESC, BY_ID] and n.table_cols == 10
    assert pb.values[s] == [False, True, True, True] and pb.build(s, agg_columns=True).value_columns == [1, 2, 3]
    top = pb.projection(pb.sparql_order_by(s, [(0, False, BY_TERM)]), [3, 0])
    assert pb.nodes[pb.nodes[top].left].right_keys[0] == BY_TERM and pb.values[top] == [True, False]


def test_explain_prints_the_reference_lines():
    pb = PlanBuilder()
    lines = explain(pb, q3_sorted(pb), agg_columns=True)
    assert lines[0] == "SortExec: TopK(fetch=10), expr=[ratio@3 DESC, product@0 ASC]"                             # ..BI Q3 (Execution Plan).snap:6
    assert lines[1].startswith("  ProjectionExec: expr=[product@0 as product,")
    pq = PlanBuilder()                                                                                            # ..BI Q1: `ENC_SORT(reviewCount@1) DESC`
    a = pq.aggregate(pq.table(0, 2, ["productType", "review"]), [0], [(abi.AGG_COUNT, 1)])
    p = pq.projection(a, [0, 1], names=["productType", "reviewCount"])
    assert explain(pq, pq.sparql_order_by(p, [(1, True)], limit=10), agg_columns=True)[0] == "SortExec: TopK(fetch=10), expr=[reviewCount@1 DESC]"
    assert explain(pq, pq.sparql_order_by(p, [(1, True), (0, False)]), agg_columns=True)[0] == "SortExec: expr=[reviewCount@1 DESC, productType@0 ASC]"


def test_the_sharded_path_refuses_the_node():
    pb = PlanBuilder()
    desc = pb.build(pb.sort(pb.table(0, 2), [(0, BY_ID, False)]))
    first = PlanBuilder()
    first = first.build(first.table(0, 2))
    ran = []
    with pytest.raises(ValueError, match="stage 1: a SortExec .* in the sharded path"):
        sharding.run_stages([(first, 0), (desc, None)], lambda d, t: ran.append(d) or [], lambda t, k: t)
    assert len(ran) == 1                                                                                          # the stage before it ran, the sort did not


# ---------------------------------------------------------------------------------------------------
# sort_key on the edge list: hand-written orders, not the function against itself
# ---------------------------------------------------------------------------------------------------
def order_of(names, desc=False):
    """the names in the order a one-key sort BY_VALUE puts their values (each name once)"""
    ids = dict(IDS, i2=I2)
    rows = [(ids[n],) for n in names]
    return [names[r] for r in sc.reference(rows, [(0, BY_VALUE, desc)])]


def test_doubles_in_ieee_total_order():
    names = ["gNaN", "g+0", "g1.5", "g-inf", "g-0", "g+inf", "g-1.5"]
    assert order_of(names) == ["g-inf", "g-1.5", "g-0", "g+0", "g1.5", "g+inf", "gNaN"]
    assert order_of(names, desc=True) == ["gNaN", "g+inf", "g1.5", "g+0", "g-0", "g-1.5", "g-inf"]


def test_equal_doubles_order_by_their_own_bytes():
    # 2 as DECIMAL 00 x8 1B C1 .., INTEGER 00 x7 02, INT 00 00 00 02, FLOAT 40 00 00 00, DOUBLE 40 00 x7: the float is a prefix of the double
    assert order_of(["g2", "int2", "f2", "i2", "d2"]) == ["d2", "i2", "int2", "f2", "g2"]
    assert sc.sort_key(sc.val(IDS["d2"]))[2].hex() == "00000000000000001bc16d674ec80000" and sc.sort_key((sc.FLT, 2.0))[2].hex() == "40000000"
    # 2^53 + 1 rounds to 2^53: the same double, the last byte decides
    assert sc.sort_key(sc.val(IDS["i2^53"]))[1] == sc.sort_key(sc.val(IDS["i2^53+1"]))[1]
    assert order_of(["i2^53+1", "i2^53"]) == ["i2^53", "i2^53+1"] and order_of(["i2^53+1", "i2^53"], desc=True) == ["i2^53+1", "i2^53"]
    # zeros: INT 0 (4 bytes) is a prefix of INTEGER 0 (8) is a prefix of DECIMAL 0 (16); FLOAT +0.0 has INT 0's key: input order
    assert order_of(["d0", "i0", "int0", "f+0"]) == ["int0", "f+0", "i0", "d0"] and order_of(["d0", "i0", "f+0", "int0"]) == ["f+0", "int0", "i0", "d0"]
    assert sc.sort_key(sc.val(IDS["int0"])) == sc.sort_key(sc.val(IDS["f+0"])) == (4, 1 << 63, bytes(4))


def test_the_double_wins_over_the_bytes():
    # two's-complement bytes of a negative integer start with FF: they would sort after every positive one
    assert order_of(["i1", "i-1", "i2", "i-2", "iMIN", "iMAX"]) == ["iMIN", "i-2", "i-1", "i1", "i2", "iMAX"]
    assert sc.sort_key(sc.val(IDS["i-1"]))[2] > sc.sort_key(sc.val(IDS["i1"]))[2]
    assert order_of(["dMAX", "int-2^31", "dMIN", "f0.75", "g0.5"]) == ["dMIN", "int-2^31", "g0.5", "f0.75", "dMAX"]


def test_types_unbound_then_booleans_then_numerics():
    names = ["iMIN", "bT", "unbound", "g-inf", "bF"]
    assert order_of(names) == ["unbound", "bF", "bT", "g-inf", "iMIN"]
    assert order_of(names, desc=True) == ["iMIN", "g-inf", "bT", "bF", "unbound"]                                  # unbound last under DESC
    assert sc.sort_key((abi.TV_NULL, None)) == (0, 0, b"") and sc.sort_key(sc.val(IDS["bT"])) == (3, 0xBFF0000000000000, b"\x01")


def test_ties_keep_input_order_in_both_directions():
    rows = [(5, 9), (3, 9), (5, 9), (3, 9), (5, 9)]
    assert sc.reference(rows, [(1, BY_ID, False)]) == [0, 1, 2, 3, 4] == sc.reference(rows, [(1, BY_ID, True)])     # all equal: as they came
    assert sc.reference(rows, [(0, BY_ID, True)]) == [0, 2, 4, 1, 3]                                                # DESC does not reverse the tie-break
    assert sc.reference(rows, [(0, BY_ID, False), (0, BY_ID, True)], fetch=3) == [1, 3, 0]                           # a column twice: the first decides
    assert sc.reference(rows, [(0, BY_ID, True)], fetch=9) == [0, 2, 4, 1, 3] and sc.reference([], [(0, BY_ID, False)]) == []


def test_id_keys_as_topk_defines_them():
    rows = [(IDS[n],) for n in ["sB", "iriB", "unbound", "sA", "iriA"]]
    assert sc.reference(rows, [(0, BY_TERM, False)]) == [2, 4, 1, 3, 0]                                             # unbound, IRIs by rank, strings by rank
    rows = [(IDS[n],) for n in ["g0.5", "sA", "i-1", "unbound", "f0.75"]]
    assert sc.reference(rows, [(0, BY_DOUBLE, False)]) == [1, 3, 2, 0, 4]                                           # not numeric = unbound: first, as they came
    assert sc.reference(rows, [(0, BY_DOUBLE, True)]) == [4, 0, 2, 1, 3]


def test_the_tables_hold_what_the_gpu_tests_need():
    assert sc.SIZES == [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 3077, 5123] and sc.FETCHES == [1, 10, 1023, 1024, 1025, 3077, 3084]
    edge = sc.edge_ids()
    assert len(edge) == 2 * len(sc.EDGE_NAMES) and 0 in edge and all(sc.val(int(i))[0] in (0, sc.BOOL, *sc.nr.NUMERIC) for i in edge)
    v, x, d, s = sc.mixed_table(3 * sc.T + 5)
    assert {sc.val(int(i))[0] for i in v} == {0, sc.BOOL, sc.INT, sc.INTEGER, sc.DEC, sc.FLT, sc.DBL}
    assert {sc.val(int(i))[0] for i in s} == {0, sc.STRING, sc.IRI} and sc.STRING in {sc.val(int(i))[0] for i in d}
    order = sc.reference(sc.rows_of([v, x, d, s]), [(0, BY_VALUE, True), (1, BY_ID, False), (2, BY_DOUBLE, True), (3, BY_TERM, False)])
    assert sorted(order) == list(range(3 * sc.T + 5)) and order != sorted(order)
    assert (sc.TV[:len(sc.ac.TV)] == sc.ac.TV).all() and sc.IDS["i1"] == 1                                           # agg_cases' ids are what they were


def test_the_compile_checks_build_and_pass_as_a_stand_alone_program():
    """tests/host/sort_compile_checks.cpp — what compiles (a valid SORT: `unknown kind` before the node existed), the record widths, how
    value columns keep their origin through the node, and every compile-time refusal with its code and its text's key words — built
    from the library's own plan_compile.cpp and run without a device (the same target with SANITIZE=1 is the sanitizer build)"""
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "rdf-fusion_amd", "csrc"), "-s", "host-checks-sort"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("0 failure(s)"), out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.count(" ok ") >= 25 and "FAIL" not in out.stdout
