// minmax_compile_checks.cpp — the host-side checks of MIN / MAX (RDFGPU_AGG_MIN / _MAX; plan_compile.cpp: compile_aggregate).
// `make host-checks-minmax`: what tests/test_minmax_cpu.py runs.
#include "compile_check_harness.hpp"

namespace {
// an aggregate's input expression `o`(ENC_TV(col a), ENC_TV(col b))
Prog binary(u32 a, u32 b, u8 o) { return cat({enc(a), enc(b)}, {op(o)}); }
constexpr u32 MIN = RDFGPU_AGG_MIN, MAX = RDFGPU_AGG_MAX;
const char* const OLD_TEXT = "aggregate 0: MIN / MAX / SAMPLE / GROUP_CONCAT are not on the device (MIN / MAX keep the first value's error state, min.rs:42-53: their result depends on row order)";
}  // namespace

int main() {
  // ---- with the flag: what compiles, and what the node is typed as
  { Builder b; u32 a = b.aggregate((int)b.table(0, 2), {0}, {{MIN, 1}, {MAX, 1}});
    auto nodes = expect("MIN and MAX over an id column", b, F, RDFGPU_OK);
    const NodeInfo& nd = nodes[a];
    check("  .. keys, then two value columns; no program", nd.width == 3 && nd.n_aggs == 2 && nd.agg_fn[0] == MIN && nd.agg_fn[1] == MAX && nd.agg_col[1] == 1 &&
          nd.agg_prog[0] < 0 && nd.agg_prog[1] < 0 && nd.origin[0].node < 0 && nd.origin[1].node == (int)a && nd.origin[2].node == (int)a && nd.origin[2].agg == 1); }
  { Builder b; u32 c = b.aggregate((int)b.table(0, 3), {0, 1}, {{RDFGPU_AGG_COUNT, 2}}); u32 a = b.aggregate((int)c, {0}, {{MAX, 2}});
    auto nodes = expect("the Q5 node: MAX over a COUNT's value column", b, F, RDFGPU_OK);
    const NodeInfo& nd = nodes[a];
    check("  .. read through a value load of node 1", nd.width == 2 && nd.agg_prog[0] == 0 && nd.agg_progs.size() == 1 && nd.agg_progs[0].n == 2 &&
          nd.agg_progs[0].nodes[1].op == kExAggValue && nd.agg_progs[0].nodes[1].u == ((c << 8) | 0u)); }
  { Builder b; u32 t = b.table(0, 3); u32 e = b.input_expr(binary(1, 2, RDFGPU_EX_MUL)); u32 a = b.aggregate((int)t, {0}, {{MIN, e}, {RDFGPU_AGG_AVG, 1}});
    auto nodes = expect("the Q6 node: MIN over an expression beside an AVG", b, F, RDFGPU_OK);
    check("  .. the program is loaded", nodes[a].agg_prog[0] == 0 && nodes[a].agg_prog[1] < 0 && nodes[a].agg_progs[0].n == 5 && nodes[a].width == 3); }
  { Builder b; u32 a = b.aggregate((int)b.table(0, 2), {0}, {{MAX, 1}}); u32 t = b.table(1, 2); b.join(RDFGPU_NODE_HASH_JOIN, (int)a, (int)t, RDFGPU_JOIN_INNER, {{0, 0}});
    auto nodes = expect("MAX at node 1 of 3, under a join", b, F, RDFGPU_OK);
    check("  .. the join carries the value column", nodes.back().width == 4 && nodes.back().origin[1].node == (int)a); }
  { Builder b; b.aggregate((int)b.table(0, 2), {}, {{MIN, 1}}); expect("zero keys", b, F, RDFGPU_OK); }
  // ---- without the flag: the status and the text every plan has always met
  { Builder b; b.aggregate((int)b.table(0, 2), {0}, {{MIN, 1}}); expect("MIN without the flag", b, 0, UNSUP, {"node 1", OLD_TEXT}); }
  { Builder b; b.aggregate((int)b.table(0, 2), {0}, {{MAX, 1}}); expect("MAX without the flag", b, 0, UNSUP, {"node 1", OLD_TEXT}); }
  { Builder b; b.aggregate((int)b.table(0, 2), {0}, {{RDFGPU_AGG_SAMPLE, 1}}); expect("SAMPLE without the flag", b, 0, UNSUP, {"node 1", OLD_TEXT}); }
  { Builder b; u32 t = b.table(0, 3); u32 e = b.input_expr(binary(1, 2, RDFGPU_EX_ADD)); b.aggregate((int)t, {0}, {{MIN, e}}); expect("MIN over an expression without the flag", b, 0, UNSUP, {"node 1", OLD_TEXT}); }
  // ---- with the flag: what stays refused
  { Builder b; b.aggregate((int)b.table(0, 2), {0}, {{RDFGPU_AGG_SAMPLE, 1}}); expect("SAMPLE with the flag", b, F, UNSUP, {"node 1: aggregate 0", "SAMPLE / GROUP_CONCAT are not on the device"}); }
  { Builder b; b.aggregate((int)b.table(0, 2), {0}, {{MAX, 1}, {RDFGPU_AGG_GROUP_CONCAT, 1}}); expect("GROUP_CONCAT with the flag", b, F, UNSUP, {"node 1: aggregate 1", "SAMPLE / GROUP_CONCAT are not on the device"}); }
  { Builder b; b.aggregate((int)b.table(0, 2), {0}, {{RDFGPU_AGG_SUM_DISTINCT, 1}}); expect("SUM DISTINCT with the flag", b, F, UNSUP, {"SUM / AVG with DISTINCT"}); }
  { Builder b; u32 t = b.table(0, 3); u32 e = b.input_expr(binary(1, 2, RDFGPU_EX_CONTAINS)); b.aggregate((int)t, {0}, {{MAX, e}});
    expect("a pattern op in the input", b, F, UNSUP, {"node 1: aggregate 0", "REGEX / CONTAINS"}); }
  { Builder b; u32 t = b.table(0, 3); u32 e = b.input_expr(enc(1)); b.pool.back() = 1; b.aggregate((int)t, {0}, {{MIN, e}});   // the program is [COLUMN] alone
    expect("an input that leaves an id", b, F, INVALID, {"node 1: aggregate 0", "does not yield a typed value"}); }
  { Builder b; b.aggregate((int)b.table(0, 2), {0}, {{MIN, 2}}); expect("an input column past the table", b, F, INVALID, {"node 1: aggregate 0 reads column 2 of 2"}); }
  // ---- a MIN / MAX value column is refused where ids are compared, like any other
  { Builder b; u32 a = b.aggregate((int)b.table(0, 2), {0}, {{MAX, 1}}); u32 t = b.table(1, 2); b.join(RDFGPU_NODE_HASH_JOIN, (int)a, (int)t, RDFGPU_JOIN_INNER, {{1, 0}});
    expect("a MAX value column as join key", b, F, UNSUP, {"node 3", "left join key column 1", "aggregate value column", "aggregate 0 of node 1"}); }
  { Builder b; u32 a = b.aggregate((int)b.table(0, 2), {0}, {{MIN, 1}}); b.aggregate((int)a, {1}, {});
    expect("a MIN value column as group column", b, F, UNSUP, {"node 2", "group column 1", "aggregate value column"}); }
  { Builder b; u32 a = b.aggregate((int)b.table(0, 2), {0}, {{MIN, 1}}); b.aggregate((int)a, {0}, {{RDFGPU_AGG_COUNT_DISTINCT, 1}});
    expect("a MIN value column under COUNT DISTINCT", b, F, UNSUP, {"node 2", "COUNT DISTINCT input column 1"}); }
  return finish();
}
