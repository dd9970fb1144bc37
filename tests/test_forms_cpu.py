"""The functional forms (IF, COALESCE, IN / NOT IN), the term tests (isIRI ..), LANG(x) = "tag" and the LeftMark join without a GPU: the
header's constants, the hand-written truth tables against the Python reference, the builder's node sequences and plan text, and the
compile checks as a stand-alone program."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from rdf_fusion_amd import abi
from rdf_fusion_amd import plan as P
from rdf_fusion_amd.plan import PlanBuilder, col, ENC_TV, EBV
import forms_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rdf-fusion_amd", "csrc")
HEADER = open(os.path.join(ROOT, "include", "rdfgpu.h")).read()
Z = (0, 0, 0, 0, 0)


def test_abi_values_and_the_header_agree():
    ops = ["IF", "COALESCE", "IS_IRI", "IS_BLANK", "IS_LITERAL", "IS_NUMERIC"]
    assert [getattr(abi, "EX_" + n) for n in ops] == list(range(55, 61))
    for k, n in enumerate(ops):
        assert re.search(rf"RDFGPU_EX_{n} = {55 + k},", HEADER), n
    assert HEADER.index("RDFGPU_EX_SECONDS = 53") < HEADER.index("RDFGPU_EX_IF = 55") < HEADER.index("RDFGPU_EX_IS_NUMERIC = 60") < HEADER.index("RDFGPU_EX__COUNT")
    assert abi.EX_SECONDS == 53 and abi.EX_COLUMN == 1                                     # the existing values did not move
    assert abi.JOIN_LEFT_MARK == 4 and re.search(r"RDFGPU_JOIN_LEFT_MARK = 4", HEADER)
    assert (abi.JOIN_INNER, abi.JOIN_LEFT, abi.JOIN_LEFT_SEMI, abi.JOIN_LEFT_ANTI) == (0, 1, 2, 3)
    assert re.search(r"#define RDFGPU_ABI_VERSION 4u", HEADER) and abi.ABI_VERSION == 4    # an addendum: no struct changed size
    assert abi.MAX_STACK == 8 and "constexpr int kMaxStack = 8;" in open(os.path.join(CSRC, "expr_device.hpp")).read()


def test_the_typed_table_has_every_tag():
    assert sorted({tag for tag, _ in F.TABLE}) == list(range(abi.TV_NULL, abi.TV_OTHER + 1))
    tv, dec = F.typed_table()
    assert len(tv) == F.N_IDS and F.BEYOND >= F.N_IDS and F.enc(F.BEYOND) == F.NULL and F.enc(0) == F.NULL
    assert tv[F.ID["dec"]]["tag"] == abi.TV_DECIMAL and tuple(dec[tv[F.ID["dec"]]["lo"]]) == F.split_i128(25 * F.E18 // 10)     # through the side table
    assert tv[F.ID["str_en"]]["aux"] == 1 and tv[F.ID["str"]]["aux"] == 0 and tv[F.ID["str_empty"]]["flags"] == abi.TVF_EMPTY_STRING
    assert np.isnan(F.f32_of(F.TABLE[F.ID["f32_nan"]][1])) and F.TABLE[F.ID["f32_neg0"]][1] == 0x80000000 and F.TABLE[F.ID["f32_pos0"]][1] == 0
    assert F.TABLE[F.ID["date_time"]][0] == abi.TV_DATE_TIME and F.TABLE[F.ID["true"]] == (abi.TV_BOOLEAN, True)
    off, heap = F.string_heap()
    assert heap[off[F.ID["str_minus_nan"]]:off[F.ID["str_minus_nan"] + 1]] == b"-nan" and len(off) == F.N_IDS + 1


# ---------------------------------------------------------------------------------------------------
# the truth tables hold against the reference
# ---------------------------------------------------------------------------------------------------
def test_if_truth_table():
    assert len(F.IF_TRUTH) == 24 and len({r[:3] for r in F.IF_TRUTH}) == 24           # six tests x value / error branches
    for test, a, b, want in F.IF_TRUTH:
        assert F.sparql_if(F.enc(test), F.enc(a), F.enc(b)) == F.enc(want), (test, a, b)
    # the test is Boolean::try_from, not the EBV: what the EBV would call true chooses nothing
    assert F.ebv(F.enc(F.ID["integer1"])) == 1 and F.ebv(F.enc(F.ID["str"])) == 1
    assert F.sparql_if(F.enc(F.ID["integer1"]), F.enc(F.ID["integer7"]), F.enc(F.ID["f64"])) == F.NULL


def test_coalesce_truth_tables():
    assert sorted({len(ops) for ops, _ in F.COALESCE_TRUTH}) == [1, 2, 3, 8]
    for k in (1, 2, 3, 8):                                                             # every position of the first non-error, and none
        firsts = {next((i for i, o in enumerate(ops) if o), None) for ops, _ in F.COALESCE_TRUTH if len(ops) == k}
        assert firsts == set(range(k)) | {None}, k
    for ops, want in F.COALESCE_TRUTH:
        assert F.coalesce_tv(*[F.enc(o) for o in ops]) == F.enc(want), ops
    for ops, want in F.COALESCE_ID_TRUTH:
        assert F.coalesce_id(*ops) == want, ops


def test_term_tests_by_tag():
    for i in list(range(F.N_IDS)) + [F.BEYOND]:
        v = F.enc(i)
        got = (F.is_iri(v), F.is_blank(v), F.is_literal(v), F.is_numeric(v))
        if v[0] == abi.TV_NULL:
            assert got == (F.NULL,) * 4, i
            continue
        t, f = F.tv_bool(True), F.tv_bool(False)
        want = {abi.TV_NAMED_NODE: (t, f, f, f), abi.TV_BLANK_NODE: (f, t, f, f)}.get(
            v[0], (f, f, t, t if v[0] in (abi.TV_INT, abi.TV_INTEGER, abi.TV_DECIMAL, abi.TV_FLOAT, abi.TV_DOUBLE) else f))
        assert got == want, i


def test_in_not_in_and_lang_equals():
    t, f, e = F.tv_bool(True), F.tv_bool(False), F.NULL
    seven, two5, s_en, iri2 = F.enc(F.ID["integer7"]), F.enc(F.ID["f64"]), F.enc(F.ID["str_en"]), F.enc(F.ID["iri2"])
    assert F.sparql_in(seven, []) == f and F.sparql_not_in(seven, []) == t              # lit(false)
    assert F.sparql_in(F.NULL, []) == f                                                 # .. whatever the left side is
    assert F.sparql_in(seven, [seven]) == t and F.sparql_in(seven, [two5]) == f
    assert F.sparql_in(F.enc(F.ID["dec"]), [two5]) == t                                 # 2.5 = 2.5e0: `=`, not sameTerm
    assert F.sparql_in(seven, [s_en]) == e                                              # incomparable: the error of EQ ..
    assert F.sparql_in(seven, [s_en, seven]) == t and F.sparql_in(seven, [seven, s_en]) == t      # .. which a true member overrides
    assert F.sparql_in(seven, [s_en, two5]) == e and F.sparql_not_in(seven, [s_en, two5]) == e
    assert F.sparql_in(iri2, [seven, s_en]) == f and F.sparql_not_in(iri2, [seven, s_en]) == t    # an IRI is comparable with everything
    assert F.sparql_in(F.enc(F.ID["f64_nan"]), [F.enc(F.ID["f64_nan"])]) == e
    assert F.sparql_in(F.NULL, [seven]) == e and F.sparql_not_in(F.NULL, [seven]) == e
    assert F.lang_equals(s_en, "en") == t and F.lang_equals(s_en, "EN") == f and F.lang_equals(s_en, "") == f
    assert F.lang_equals(F.enc(F.ID["str"]), "") == t and F.lang_equals(seven, "") == t and F.lang_equals(seven, "en") == f
    assert F.lang_equals(F.enc(F.ID["str_en_gb"]), "en") == f and F.lang_equals(F.enc(F.ID["str_en_gb"]), "en-GB") == t      # `=`, not LANGMATCHES
    assert F.lang_equals(iri2, "") == e and F.lang_equals(F.enc(F.ID["blank"]), "") == e and F.lang_equals(F.NULL, "") == e


def test_mark_join_reference():
    a = lambda *v: np.array(v, np.uint32)
    L = [a(1, 2, 0, 2, 3), a(7, 7, 7, 8, 0)]
    R = [a(2, 2, 0, 9), a(7, 8, 7, 7)]
    assert F.mark_join(L, R, [(0, 0)]) == [(0, False), (1, True), (2, False), (3, True), (4, False)]            # a null key equals nothing, not even null
    assert F.mark_join(L, R, [(0, 0), (1, 1)]) == [(0, False), (1, True), (2, False), (3, True), (4, False)]
    assert F.mark_join(L, R, [(0, 0)], lambda l, r: l[1] != r[1]) == [(0, False), (1, True), (2, False), (3, True), (4, False)]
    assert F.mark_join(L, R, [(0, 0)], lambda l, r: l[1] == r[1] == 8) == [(0, False), (1, False), (2, False), (3, True), (4, False)]
    assert F.mark_join(L, R, []) == [(j, True) for j in range(5)]                       # no keys, no filter: the right input has a row
    assert F.mark_join(L, [a(), a()], []) == [(j, False) for j in range(5)] and F.mark_join([a(), a()], R, []) == []
    four = [a(1, 1), a(2, 2), a(3, 3), a(4, 0)]
    assert F.mark_join(four, [c[:1] for c in four], [(k, k) for k in range(4)]) == [(0, True), (1, False)]


# ---------------------------------------------------------------------------------------------------
# the builder
# ---------------------------------------------------------------------------------------------------
def ops(e):
    return [n[0] for n in e.nodes]


def test_builder_node_sequences():
    a, b, c = ENC_TV(col(0)), ENC_TV(col(1)), ENC_TV(col(2))
    assert P.IF(a, b, c).nodes == a.nodes + b.nodes + c.nodes + [(abi.EX_IF,) + Z]
    assert P.COALESCE(a, b, c).nodes == a.nodes + b.nodes + c.nodes + [(abi.EX_COALESCE, 0, 0, 3, 0, 0)]
    assert P.COALESCE(col(0), col(1)).nodes == col(0).nodes + col(1).nodes + [(abi.EX_COALESCE, 0, 0, 2, 0, 0)]
    assert P.COALESCE(a).nodes[-1] == (abi.EX_COALESCE, 0, 0, 1, 0, 0)
    for bad in ([], [a] * 9):
        with pytest.raises(ValueError):
            P.COALESCE(*bad)
    for fn, op in ((P.IS_IRI, abi.EX_IS_IRI), (P.IS_BLANK, abi.EX_IS_BLANK), (P.IS_LITERAL, abi.EX_IS_LITERAL), (P.IS_NUMERIC, abi.EX_IS_NUMERIC)):
        assert fn(a).nodes == a.nodes + [(op,) + Z]
    # IN: BOOLEAN_AS_TERM of the OR chain of EBV(EQ(lhs, e_i)), left to right
    e1, e2, e3 = P.integer(1), P.integer(2), P.integer(3)
    eq = lambda m: a.nodes + m.nodes + [(abi.EX_EQ,) + Z, (abi.EX_EBV,) + Z]
    assert P.IN(a, [e1]).nodes == eq(e1) + [(abi.EX_BOOL_AS_TV,) + Z]
    assert P.IN(a, [e1, e2, e3]).nodes == eq(e1) + eq(e2) + [(abi.EX_OR,) + Z] + eq(e3) + [(abi.EX_OR,) + Z, (abi.EX_BOOL_AS_TV,) + Z]
    assert P.IN(a, []).nodes == P.lit_bool(False).nodes + [(abi.EX_BOOL_AS_TV,) + Z] == [(abi.EX_LIT_BOOL, 0, 0, 0, 0, 0), (abi.EX_BOOL_AS_TV,) + Z]
    assert P.NOT_IN(a, [e1, e2]).nodes == P.IN(a, [e1, e2]).nodes + [(abi.EX_EBV,) + Z, (abi.EX_NOT,) + Z, (abi.EX_BOOL_AS_TV,) + Z]
    # LANG(x) = "tag": the LANGMATCHES op with a table that is 1 exactly for the ids with that tag
    tags = ["", "en", "de", "en-GB", "en"]
    (op, _, _, u, _, _), = P.LANG_EQUALS(a, "en", tags).nodes[len(a.nodes):]
    assert op == abi.EX_LANG_IN and u == (bytes([0, 1, 0, 0, 1]), b"", abi.EX_LANG_IN)
    assert P.LANG_EQUALS(a, "", tags).nodes[-1][3][0] == bytes([1, 0, 0, 0, 0])
    assert P.LANGMATCHES_LANG(a, "en", tags).nodes[-1][3][0] == bytes([0, 1, 0, 1, 1])        # the range matches en-GB, `=` does not
    with pytest.raises(ValueError):
        P.LANG_EQUALS(a, "en", ["en"])


def test_plan_text_spells_the_ops_as_the_reference_does():
    pb = PlanBuilder()
    t = pb.table(0, 3, names=["x", "y", "z"])
    a, b, c = ENC_TV(col(0)), ENC_TV(col(1)), ENC_TV(col(2))
    line = lambda e: P.explain(pb, pb.filter(t, e))[0]
    assert line(EBV(P.IS_LITERAL(a))) == "FilterExec: EBV(isLITERAL(ENC_TV(x@0)))"
    assert line(EBV(P.IS_IRI(a))) == "FilterExec: EBV(isIRI(ENC_TV(x@0)))"
    assert line(EBV(P.IS_BLANK(a))) == "FilterExec: EBV(isBLANK(ENC_TV(x@0)))"
    assert line(EBV(P.IS_NUMERIC(a))) == "FilterExec: EBV(isNUMERIC(ENC_TV(x@0)))"
    assert line(EBV(P.IF(P.IS_NUMERIC(a), P.ABS(a), P.COALESCE(b, P.integer(0))))) == \
        "FilterExec: EBV(IF(isNUMERIC(ENC_TV(x@0)), ABS(ENC_TV(x@0)), COALESCE(ENC_TV(y@1), 9:0)))"
    assert line(EBV(ENC_TV(P.COALESCE(col(1), col(2))))) == "FilterExec: EBV(ENC_TV(COALESCE(y@1, z@2)))"
    assert line(EBV(P.IN(a, [P.integer(1), c]))) == "FilterExec: EBV(BOOLEAN_AS_TERM(EBV(EQ(ENC_TV(x@0), 9:1)) OR EBV(EQ(ENC_TV(x@0), ENC_TV(z@2)))))"
    assert line(EBV(P.IN(a, []))) == "FilterExec: EBV(BOOLEAN_AS_TERM(false))"
    x = pb.extend(t, [P.IF(P.IS_IRI(a), b, c)], keep=[0], names=["v"])
    assert P.explain(pb, x)[0] == "ProjectionExec: expr=[x@0 as x, IF(isIRI(ENC_TV(x@0)), ENC_TV(y@1), ENC_TV(z@2)) as v]"


def test_sparql_exists_value_lowers_like_sparql_exists():
    for nullable in ((), ("s",), ("s", "p")):
        pb = PlanBuilder()
        o, i = pb.table(0, 3, ["s", "p", "o"]), pb.table(1, 3, ["p", "q", "s"])
        semi, mark = pb.sparql_exists(o, i, nullable=nullable), pb.sparql_exists_value(o, i, nullable=nullable)
        ns, nm = pb.nodes[semi], pb.nodes[mark]
        assert (ns.join_type, nm.join_type) == (abi.JOIN_LEFT_SEMI, abi.JOIN_LEFT_MARK)
        assert nm.kind == ns.kind and nm.n_keys == ns.n_keys and list(nm.left_keys) == list(ns.left_keys) and list(nm.right_keys) == list(ns.right_keys)
        key = lambda n: [(e.op, e.u) for e in pb.exprs[n.expr_off:n.expr_off + n.expr_len]]
        assert key(nm) == key(ns) and (nm.expr_len > 0) == bool(nullable)
        assert pb.width[mark] == pb.width[o] + 1 and pb.names[mark] == ["s", "p", "o", "mark"] and pb.width[semi] == pb.width[o]
        assert pb.values[mark] == [False, False, False, True] and pb.values[semi] == [False] * 3
        if not nullable:
            assert nm.kind == abi.NODE_HASH_JOIN and [(nm.left_keys[k], nm.right_keys[k]) for k in range(2)] == [(1, 0), (0, 2)]      # p, s: sorted
    pb = PlanBuilder()
    o, i = pb.table(0, 2, ["a", "b"]), pb.table(1, 1, ["c"])                             # no shared variable: does `inner` have a row?
    m = pb.sparql_exists_value(o, i)
    assert pb.nodes[m].kind == abi.NODE_NESTED_LOOP_JOIN and pb.nodes[m].join_type == abi.JOIN_LEFT_MARK and pb.nodes[m].expr_len == 0
    d = pb.build(pb.filter(m, P.OR(EBV(P.GT(ENC_TV(col(1)), P.integer(10))), EBV(ENC_TV(col(2))))), agg_columns=True)
    assert d.flags == abi.PLAN_AGG_COLUMNS and d.value_columns == [2]


def test_plan_text_of_a_mark_join_and_the_builder_entry_points():
    pb = PlanBuilder()
    o, i = pb.table(0, 2, ["s", "p"]), pb.table(1, 2, ["s", "q"])
    m = pb.sparql_exists_value(o, i)
    f = pb.filter(m, P.OR(EBV(P.GT(ENC_TV(col(1)), P.integer(10))), EBV(ENC_TV(col(2)))), projection=[0, 1])
    lines = P.explain(pb, f)
    assert lines[0] == "FilterExec: EBV(GT(ENC_TV(p@1), 9:10)) OR EBV(ENC_TV(mark@2)), projection=[s@0, p@1]"
    assert lines[1] == "  HashJoinExec: mode=CollectLeft, join_type=LeftMark, on=[(s@0, s@0)]"
    h = pb.hash_join(o, i, [(0, 0)], join_type=abi.JOIN_LEFT_MARK, filter=P.ID_NEQ(col(1), col(3)), projection=[2, 0])
    assert pb.width[h] == 2 and pb.names[h] == ["mark", "s"] and pb.values[h] == [True, False]
    assert P.explain(pb, h)[0] == "HashJoinExec: mode=CollectLeft, join_type=LeftMark, on=[(s@0, s@0)], filter=p@0 != q@1, projection=[mark@2, s@0]"
    n = pb.nested_loop_join(o, i, abi.JOIN_LEFT_MARK, filter=P.ID_EQ(col(0), col(2)))
    assert pb.width[n] == 3 and pb.values[n] == [False, False, True]
    assert P.explain(pb, n)[0] == "NestedLoopJoinExec: join_type=LeftMark, filter=s@0 = s@1"
    x = pb.extend(m, [P.IF(ENC_TV(col(2)), ENC_TV(col(0)), ENC_TV(col(1)))], names=["v"])
    assert pb.values[x] == [False, False, True, True]
    g = pb.aggregate(m, [0], [(abi.AGG_SUM, 2), (abi.AGG_COUNT, 2)])
    assert pb.names[g] == ["s", "SUM(mark)", "COUNT(mark)"]


def test_the_sharded_path_refuses_a_mark_join():
    from rdf_fusion_amd import sharding
    pb = PlanBuilder()
    m = pb.sparql_exists_value(pb.table(0, 2, ["s", "p"]), pb.table(1, 2, ["s", "q"]))
    ran = []
    with pytest.raises(ValueError, match="LeftMark"):
        sharding.run_stages([(pb.build(m, agg_columns=True), None)], execute=lambda d, t: ran.append(d), repartition=lambda t, k: t)
    assert not ran


# ---------------------------------------------------------------------------------------------------
# compile checks
# ---------------------------------------------------------------------------------------------------
def test_the_compile_checks_build_and_pass_as_a_stand_alone_program():
    """tests/host/forms_compile_checks.cpp: each op accepted in a filter, every join kind's filter, an aggregate input and an EXTEND, always
    in the generic VM; IF over a BOOL-kind test, COALESCE with u of 0 or 9, with mixed kinds and with an unwrapped value column refused; a
    mark join without RDFGPU_PLAN_AGG_COLUMNS refused with its text, its mark refused as a join key, a TopK key and a UNION input, a
    projection index beyond n_left_cols refused; a semi join's compile result unchanged."""
    out = subprocess.run(["make", "-C", CSRC, "-s", "host-checks-forms"], capture_output=True, text=True)
    sys.stdout.write(out.stdout[-6000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "\n0 failure(s)" in out.stdout and out.stdout.count(" ok  ") > 100
