"""Numeric expression ops (MUL, DIV, NEG, PLUS, ABS, ROUND, CEIL, FLOOR, CAST) and expression inputs of SUM / AVG on the host side: the
restatement in numeric_ref.py against the reference's own known answers (tests/golden/numeric_kats.json), the ABI constants, the plan
builder's encodings and display.  No GPU needed."""
import json
import os
import re

import numpy as np

from rdf_fusion_amd import abi
from rdf_fusion_amd import plan as P
import numeric_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E18 = R.E18


def _f32(h):
    return np.uint32(int(h, 16)).view(np.float32)


def _f64(h):
    return np.uint64(int(h, 16)).view(np.float64)


def _payload(v):
    return None if v == R.ERR else v[1]


# how each group of the JSON is evaluated by the restatement: op -> (args -> value or None for the error value, kind of the value)
KAT_OPS = {
    "dec_mul": (lambda a, b: R.dec_mul(int(a), int(b)), "int"), "dec_div": (lambda a, b: R.dec_div(int(a), int(b)), "int"),
    "dec_round": (lambda a: R.dec_round(int(a)), "int"), "dec_ceil": (lambda a: R.dec_ceil(int(a)), "int"), "dec_floor": (lambda a: R.dec_floor(int(a)), "int"),
    "bool_from_f32": (lambda h: _payload(R.cast(R.BOOL, (R.FLT, _f32(h)))), "int"), "bool_from_f64": (lambda h: _payload(R.cast(R.BOOL, (R.DBL, _f64(h)))), "int"),
    "dec_from_f32": (lambda h: _payload(R.cast(R.DEC, (R.FLT, _f32(h)))), "int"), "dec_from_f64": (lambda h: _payload(R.cast(R.DEC, (R.DBL, _f64(h)))), "int"),
    "f32_from_dec": (lambda a: _payload(R.cast(R.FLT, (R.DEC, int(a)))), "f32"), "f64_from_dec": (lambda a: _payload(R.cast(R.DBL, (R.DEC, int(a)))), "f64"),
    "int_from_f32": (lambda h: _payload(R.cast(R.INT, (R.FLT, _f32(h)))), "int"), "int_from_f64": (lambda h: _payload(R.cast(R.INT, (R.DBL, _f64(h)))), "int"),
    "int_from_dec": (lambda a: _payload(R.cast(R.INT, (R.DEC, int(a)))), "int"),
    "integer_from_f32": (lambda h: _payload(R.cast(R.INTEGER, (R.FLT, _f32(h)))), "int"), "integer_from_f64": (lambda h: _payload(R.cast(R.INTEGER, (R.DBL, _f64(h)))), "int"),
    "integer_from_dec": (lambda a: _payload(R.cast(R.INTEGER, (R.DEC, int(a)))), "int"),
    "int_mul": (lambda a, b: _payload(R.binary(abi.EX_MUL, (R.INT, int(a)), (R.INT, int(b)))), "int"),
    "int_div": (lambda a, b: _payload(R.binary(abi.EX_DIV, (R.INT, int(a)), (R.INT, int(b)))), "int"),
    "integer_mul": (lambda a, b: _payload(R.binary(abi.EX_MUL, (R.INTEGER, int(a)), (R.INTEGER, int(b)))), "int"),
    "integer_div": (lambda a, b: _payload(R.binary(abi.EX_DIV, (R.INTEGER, int(a)), (R.INTEGER, int(b)))), "int"),
}


def test_restatement_against_the_reference_known_answers():
    kats = json.load(open(os.path.join(ROOT, "tests", "golden", "numeric_kats.json")))
    n = 0
    for g in kats["groups"]:
        fn, kind = KAT_OPS[g["op"]]
        read = {"int": int, "f32": _f32, "f64": _f64}[kind]
        for args, want in g["cases"]:
            got = fn(*args)
            where = (g["source"], args, got)
            if want == "error":
                assert got is None, where
            elif isinstance(want, dict):
                centre, bound = (read(x) for x in want["near"])
                assert got is not None and abs(got - centre) < bound, where
            elif kind == "int":
                assert got == int(want), where
            else:
                assert got is not None and got.dtype == read(want).dtype and got.tobytes() == read(want).tobytes(), where
            n += 1
    assert n == 141 and {g["op"] for g in kats["groups"]} == set(KAT_OPS)


def test_ops_by_hand():
    I, G, D, F, B = R.INT, R.INTEGER, R.DEC, R.FLT, R.DBL
    assert R.binary(abi.EX_MUL, (I, 65536), (I, 65536)) == R.ERR                      # i32 checked
    assert R.binary(abi.EX_MUL, (I, 65536), (G, 65536)) == (G, 1 << 32)
    assert R.binary(abi.EX_MUL, (G, 1 << 62), (G, 2)) == R.ERR
    assert R.binary(abi.EX_DIV, (I, 1), (I, 2)) == (D, E18 // 2)                       # integers divide as decimals
    assert R.binary(abi.EX_DIV, (G, 1), (G, 0)) == R.ERR
    assert R.binary(abi.EX_DIV, (G, 1), (G, 3)) == (D, 333333333333333333)
    assert R.binary(abi.EX_MUL, (D, 0), (D, 25 * E18 // 10)) == R.ERR                  # as written: 0 zeros + 17 zeros < 18
    assert R.binary(abi.EX_MUL, (D, 1), (D, E18)) == (D, 1)
    assert R.binary(abi.EX_MUL, (D, 1), (D, 1)) == R.ERR                               # 10^-36 needs more precision
    t, v = R.binary(abi.EX_DIV, (B, np.float64(1.0)), (G, 0))
    assert t == B and np.isinf(v)
    t, v = R.binary(abi.EX_DIV, (F, np.float32(0.0)), (F, np.float32(0.0)))
    assert t == F and np.isnan(v) and isinstance(v, np.float32)
    assert R.binary(abi.EX_MUL, (R.STR, None), (G, 1)) == R.ERR
    assert R.unary(abi.EX_NEG, (I, R.I32_MIN)) == R.ERR and R.unary(abi.EX_ABS, (G, R.I64_MIN)) == R.ERR
    assert R.unary(abi.EX_NEG, (D, R.I128_MIN)) == R.ERR and R.unary(abi.EX_ABS, (D, -5)) == (D, 5)
    assert R.bits(R.unary(abi.EX_NEG, (B, np.float64(0.0)))) == (B, -(1 << 63), 0)
    assert R.bits(R.unary(abi.EX_CEIL, (B, np.float64(-0.5)))) == (B, -(1 << 63), 0)   # CEIL(-0.5) = -0.0
    assert R.unary(abi.EX_ROUND, (B, np.float64(0.49999999999999994)))[1] == 0.0
    assert R.unary(abi.EX_ROUND, (B, np.float64(2.5)))[1] == 3.0 and R.unary(abi.EX_ROUND, (B, np.float64(-2.5)))[1] == -3.0
    assert R.unary(abi.EX_ROUND, (F, np.float32(0.5)))[1] == 1.0
    assert R.unary(abi.EX_ROUND, (D, -25 * E18 // 10)) == (D, -2 * E18) and R.unary(abi.EX_ROUND, (D, 25 * E18 // 10)) == (D, 3 * E18)
    assert R.unary(abi.EX_FLOOR, (I, -3)) == (I, -3) and R.unary(abi.EX_PLUS, (R.STR, None)) == R.ERR
    # casts: decimal.rs:420-435 saturates at 2^127 exactly, integers truncate toward zero
    # x = fl(2^127 / 10^18) and its neighbours: x * 10^18 rounds to exactly 2^127 (inside the range test, `as i128` saturates to MAX), to the
    # f64 below 2^127 (converted exactly), and to the f64 above it (outside the range: error)
    x = np.float64(2.0 ** 127) / np.float64(1e18)
    below, above = np.nextafter(x, 0), np.nextafter(x, np.inf)
    assert x * np.float64(1e18) == 2.0 ** 127 and below * np.float64(1e18) == 2.0 ** 127 - 2.0 ** 74 and above * np.float64(1e18) == 2.0 ** 127 + 2.0 ** 75
    assert R.dec_from_f64(x) == R.I128_MAX and R.cast(D, (B, x)) == (D, R.I128_MAX)
    assert R.dec_from_f64(below) == (1 << 127) - (1 << 74) and R.cast(D, (B, below)) == (D, (1 << 127) - (1 << 74))
    assert R.dec_from_f64(above) is None and R.cast(D, (B, above)) == R.ERR
    assert R.dec_from_f64(-x) == R.I128_MIN and R.dec_from_f64(-above) is None
    assert R.cast(G, (B, x)) == R.ERR and R.cast(G, (B, np.float64(2.0 ** 62))) == (G, 1 << 62)      # 2^62 * 10^18 is exact in f64
    assert R.cast(D, (B, np.float64(1e21))) == R.ERR and R.cast(D, (B, np.float64(np.nan))) == R.ERR
    assert R.cast(G, (B, np.float64(-2.75))) == (G, -2) and R.cast(I, (D, -27 * E18 // 10)) == (I, -2)
    assert R.cast(I, (G, 1 << 31)) == R.ERR and R.cast(I, (G, -(1 << 31))) == (I, -(1 << 31))
    assert R.cast(G, (B, np.float64(2.0 ** 63))) == R.ERR
    assert R.cast(F, (B, np.float64(1e40)))[1] == np.inf
    assert R.cast(R.BOOL, (D, 0)) == (R.BOOL, 0) and R.cast(D, (R.BOOL, 1)) == (D, E18)
    assert R.cast(G, (abi.TV_NAMED_NODE, None)) == R.ERR and R.cast(G, (R.STR, None), aux=3) == R.ERR
    try:
        R.cast(G, (R.STR, None))
        assert False
    except R.CastFromString:
        pass


def test_header_constants_match_abi_py():
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rdfgpu.h")).read(), flags=re.S)
    assert int(re.search(r"#define RDFGPU_ABI_VERSION (\d+)u", h).group(1)) == abi.ABI_VERSION == 4
    for name in ("MUL", "DIV", "NEG", "PLUS", "ABS", "ROUND", "CEIL", "FLOOR", "CAST"):
        assert int(re.search(rf"RDFGPU_EX_{name} = (\d+)", h).group(1)) == getattr(abi, "EX_" + name), name
    assert abi.EX_MUL == abi.EX_STRAFTER + 1 and abi.EX_CAST == 45
    assert int(re.search(r"#define RDFGPU_AGG_INPUT_EXPR 0x([0-9a-fA-F]+)u", h).group(1), 16) == abi.AGG_INPUT_EXPR == 1 << 31
    assert abi.CAST_TARGETS == (abi.TV_BOOLEAN, abi.TV_INT, abi.TV_INTEGER, abi.TV_DECIMAL, abi.TV_FLOAT, abi.TV_DOUBLE)


def test_builder_node_encodings_and_explain():
    a, b = P.ENC_TV(P.col(0)), P.ENC_TV(P.col(1))
    assert [n[0] for n in P.MUL(a, b).nodes] == [abi.EX_COLUMN, abi.EX_ENC_TV, abi.EX_COLUMN, abi.EX_ENC_TV, abi.EX_MUL]
    assert P.DIV(a, b).nodes[-1][0] == abi.EX_DIV
    for fn, op in ((P.NEG, abi.EX_NEG), (P.PLUS, abi.EX_PLUS), (P.ABS, abi.EX_ABS), (P.ROUND, abi.EX_ROUND), (P.CEIL, abi.EX_CEIL), (P.FLOOR, abi.EX_FLOOR)):
        assert fn(a).nodes[-1] == (op, 0, 0, 0, 0, 0)
    assert P.CAST(a, abi.TV_FLOAT).nodes[-1] == (abi.EX_CAST, 0, 0, abi.TV_FLOAT, 0, 0)
    for fn, tag in ((P.xsd_boolean, abi.TV_BOOLEAN), (P.xsd_int, abi.TV_INT), (P.xsd_integer, abi.TV_INTEGER), (P.xsd_decimal, abi.TV_DECIMAL),
                    (P.xsd_float, abi.TV_FLOAT), (P.xsd_double, abi.TV_DOUBLE)):
        assert fn(a).nodes[-1][3] == tag
    pb = P.PlanBuilder()
    t = pb.table(0, 2, ["x", "y"])
    e = P.EBV(P.GT(P.MUL(P.integer(10), P.FLOOR(P.DIV(P.ENC_TV(P.col(0)), P.double(10.0)))), P.xsd_integer(P.NEG(P.ABS(P.ENC_TV(P.col(1)))))))
    f = pb.filter(t, e)
    ten = int(np.float64(10.0).view(np.int64))
    assert P.explain(pb, f)[0] == f"FilterExec: EBV(GT(MUL(9:10, FLOOR(DIV(ENC_TV(x@0), 6:{ten}))), xsd:integer(MINUS(ABS(ENC_TV(y@1))))))"
    names = [P.format_expr([abi.ExprNode(*((n[0], n[1], n[2], 0) + n[3:])) for n in fn(P.ENC_TV(P.col(0))).nodes], ["x"]) for fn in
             (P.PLUS, P.ROUND, P.CEIL, P.xsd_boolean, P.xsd_int, P.xsd_decimal, P.xsd_float, P.xsd_double)]
    assert names == [f"{s}(ENC_TV(x@0))" for s in ("PLUS", "ROUND", "CEIL", "xsd:boolean", "xsd:int", "xsd:decimal", "xsd:float", "xsd:double")]


def test_pool_encoding_of_an_expression_input():
    pb = P.PlanBuilder()
    t = pb.table(0, 3, ["k", "a", "b"])
    pb.filter(t, P.EBV(P.ENC_TV(P.col(0))))                   # (some expression nodes before the aggregate's)
    first_expr = len(pb.exprs)
    g = pb.aggregate(t, [0], [(abi.AGG_SUM, P.MUL(P.ENC_TV(P.col(1)), P.ENC_TV(P.col(2)))), (abi.AGG_COUNT, 1), (abi.AGG_AVG, P.NEG(P.ENC_TV(P.col(2))))])
    n = pb.nodes[g]
    s = n.table_slot
    assert n.table_cols == 3 and pb.pool[s:s + 6] == [abi.AGG_SUM, abi.AGG_INPUT_EXPR | (s + 6), abi.AGG_COUNT, 1, abi.AGG_AVG, abi.AGG_INPUT_EXPR | (s + 8)]
    assert pb.pool[s + 6:s + 10] == [first_expr, 5, first_expr + 5, 3]
    assert [e.op for e in pb.exprs[first_expr:first_expr + 5]] == [abi.EX_COLUMN, abi.EX_ENC_TV, abi.EX_COLUMN, abi.EX_ENC_TV, abi.EX_MUL]
    assert pb.names[g] == ["k", "SUM(MUL(ENC_TV(a), ENC_TV(b)))", "COUNT(a)", "AVG(MINUS(ENC_TV(b)))"]
    assert P.explain(pb, g)[0] == ("AggregateExec: mode=Single, gby=[k@0 as k], aggr=[SUM(MUL(ENC_TV(a@1), ENC_TV(b@2))), COUNT(a@1), "
                                   "AVG(MINUS(ENC_TV(b@2)))]")
    desc = pb.build(g)
    assert desc.width == 4
