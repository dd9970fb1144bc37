// lex_compile_checks.cpp — the host-side checks of the lexical casts (RDFGPU_EX_CAST_STRING / RDFGPU_EX_CAST_LEX; plan_compile.cpp:
// check_program and what routes a program).  `make host-checks-lex-compile`: what tests/test_lex_cast_cpu.py runs.
#include "compile_check_harness.hpp"

namespace {
constexpr u8 STRING = RDFGPU_EX_CAST_STRING, LEX = RDFGPU_EX_CAST_LEX, ENC = RDFGPU_EX_ENC_TV, EBV_ = RDFGPU_EX_EBV, LT = RDFGPU_EX_LT;
constexpr u32 FLOAT = RDFGPU_TV_FLOAT;
// xsd:float(xsd:string(ENC_TV(c)))
Prog price(u32 c) { return {column(c), op(STRING), op(LEX, FLOAT)}; }
}  // namespace

int main() {
  // ---- kinds and targets
  expect_program("xsd:float(xsd:string(ENC_TV(c))) leaves a typed value", price(0), 1, RDFGPU_OK, VK_TV);
  for (u32 t : {(u32)RDFGPU_TV_BOOLEAN, (u32)RDFGPU_TV_INT, (u32)RDFGPU_TV_INTEGER, (u32)RDFGPU_TV_DECIMAL, (u32)RDFGPU_TV_FLOAT, (u32)RDFGPU_TV_DOUBLE})
    expect_program("CAST_LEX to each of the six targets", {column(0), op(ENC), op(LEX, t)}, 1, RDFGPU_OK, VK_TV);
  for (u32 t : {(u32)RDFGPU_TV_STRING, (u32)RDFGPU_TV_DATE_TIME, (u32)RDFGPU_TV_NAMED_NODE, (u32)RDFGPU_TV_OTHER, 200u})
    expect_program("CAST_LEX to any other target", {column(0), op(ENC), op(LEX, t)}, 1, UNSUP, 0, {"CAST_LEX to tag"});
  expect_program("plain CAST to xsd:string stays refused", {column(0), op(ENC), op(RDFGPU_EX_CAST, RDFGPU_TV_STRING)}, 1, UNSUP, 0, {"CAST to tag"});
  expect_program("CAST_STRING of a typed value: a kind error", {column(0), op(ENC), op(STRING)}, 1, INVALID, 0, {"CAST_STRING", "wrong kind"});
  expect_program("CAST_STRING of a value column: a kind error", {column(0), op(STRING)}, 1, INVALID, 0, {"CAST_STRING", "aggregate value column"}, 1u);
  expect_program("CAST_LEX of an id: a kind error", {column(0), op(LEX, FLOAT)}, 1, INVALID, 0, {"CAST_LEX"});
  expect_program("CAST_LEX of a value column's value is a CAST", {column(0), op(ENC), op(LEX, FLOAT)}, 1, RDFGPU_OK, VK_TV, {}, 1u);
  expect_program("CAST_LEX of a rank-only string literal", {lit(RDFGPU_TV_STRING, 5), op(LEX, FLOAT)}, 0, UNSUP, 0, {"CAST_LEX", "dictionary rank"});
  expect_program("CAST_STRING beside a rank-only string literal", cat({{column(0), op(STRING), lit(RDFGPU_TV_STRING, 5)}}, {op(RDFGPU_EX_EQ), op(EBV_)}), 1, UNSUP, 0, {"given by rank"});
  expect_program("STRLEN(xsd:string(..)): a view like STR's", {column(0), op(STRING), op(RDFGPU_EX_STRLEN)}, 1, RDFGPU_OK, VK_TV);
  // ---- routing: a predicate or join filter with either op runs in the generic VM
  const Prog q8 = cat({price(0), {column(3), op(ENC), op(LT)}}, {op(EBV_)});   // EBV(LT(xsd:float(xsd:string(ENC_TV(price))), avg))
  { Builder b; b.filter((int)b.table(0, 2), cat({price(0)}, {lit(RDFGPU_TV_FLOAT, 0), op(LT), op(EBV_)}));
    check("FilterExec: the generic VM", expect("FilterExec over the cast", b, 0, RDFGPU_OK).back().shape == 0); }
  { Builder b; b.filter((int)b.table(0, 2), {column(0), op(ENC), lit(RDFGPU_TV_FLOAT, 0), op(LT), op(EBV_)});
    check("  .. and the compare shape without it is still shape 2", expect("FilterExec without the cast", b, 0, RDFGPU_OK).back().shape == 2); }
  for (u32 type : {(u32)RDFGPU_JOIN_INNER, (u32)RDFGPU_JOIN_LEFT, (u32)RDFGPU_JOIN_LEFT_SEMI, (u32)RDFGPU_JOIN_LEFT_ANTI}) {
    Builder b; u32 l = b.table(0, 2), r = b.table(1, 2); b.join(RDFGPU_NODE_HASH_JOIN, (int)l, (int)r, type, {{0, 0}}, q8);
    check("HashJoinExec filter: the generic VM", expect("the BI Q8 join filter, every join type", b, 0, RDFGPU_OK).back().shape == 1); }
  // ---- the hosts that prepare no patterns take the two ops
  { Builder b; b.aggregate((int)b.table(0, 2), {0}, {{RDFGPU_AGG_SUM, b.input_expr(price(1))}}); expect("SUM(xsd:float(xsd:string(ENC_TV(price))))", b, 0, RDFGPU_OK); }
  { Builder b; b.aggregate((int)b.table(0, 2), {0}, {{RDFGPU_AGG_AVG, b.input_expr({column(1), op(STRING), op(LEX, RDFGPU_TV_DECIMAL)})}}); expect("AVG(xsd:decimal(xsd:string(..)))", b, 0, RDFGPU_OK); }
  { Builder b; b.extend((int)b.table(0, 2), {price(1)}); expect("a computed column of the cast", b, F, RDFGPU_OK); }
  { Builder b; b.extend((int)b.table(0, 2), {{column(1), op(STRING), op(RDFGPU_EX_STRLEN)}});
    expect("a computed column with STRLEN stays refused", b, F, UNSUP, {"string functions in a computed column"}); }
  { Builder b; b.aggregate((int)b.table(0, 2), {0}, {{RDFGPU_AGG_SUM, b.input_expr({column(1), op(STRING), op(LEX, RDFGPU_TV_STRING)})}});
    expect("SUM over a CAST_LEX to xsd:string", b, 0, UNSUP, {"CAST_LEX to tag"}); }
  return finish();
}
