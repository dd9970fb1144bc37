// extend_compile_checks.cpp — the host-side checks of ProjectionExec with expressions (RDFGPU_NODE_EXTEND; plan_compile.cpp:
// compile_extend and what it calls).  `make host-checks-extend`: what tests/test_extend_cpu.py runs.
#include "compile_check_harness.hpp"

namespace {
Prog ratio(u32 a, u32 b) {   // DIV(xsd:float(ENC_TV(col a)), ENC_TV(col b))
  return {column(a), op(RDFGPU_EX_ENC_TV), op(RDFGPU_EX_CAST, RDFGPU_TV_FLOAT), column(b), op(RDFGPU_EX_ENC_TV), op(RDFGPU_EX_DIV)};
}

// table(0: k, x, y) -> EXTEND keep all, [MUL(ENC_TV(x), ENC_TV(y))]: columns k, x, y, product; node 1, its computed column is column 3
u32 ext(Builder& b) {
  return b.extend((int)b.table(0, 3), {{column(1), op(RDFGPU_EX_ENC_TV), column(2), op(RDFGPU_EX_ENC_TV), op(RDFGPU_EX_MUL)}});
}
}  // namespace

int main() {
  // ---- what compiles under the flag, and how the value loads are typed
  { Builder b; u32 e = ext(b);
    auto nodes = expect("BIND over a table, all columns kept", b, F, RDFGPU_OK);
    const NodeInfo& nd = nodes[e];
    check("  .. width, origins, the program as written", nd.width == 4 && nd.n_proj == 3 && nd.origin[2].node < 0 && nd.origin[3].node == (int)e && nd.origin[3].agg == 0 &&
          nd.agg_progs.size() == 1 && nd.agg_progs[0].n == 5 && nd.agg_progs[0].nodes[1].op == RDFGPU_EX_ENC_TV && nd.n_cols_read == 2 && nd.n_enc_tv == 2); }
  { Builder b; u32 a = b.aggregate((int)b.table(0, 3), {0}, {{RDFGPU_AGG_COUNT, 1}, {RDFGPU_AGG_COUNT, 2}});
    u32 e = b.extend((int)a, {ratio(1, 2), enc(0)}, {0, 2});   // a program ranges over all input columns, not only the kept ones
    auto nodes = expect("EXTEND over an AGGREGATE (the Q3 ratio)", b, F, RDFGPU_OK);
    const NodeInfo& nd = nodes[e];
    const ExprProgram& p = nd.agg_progs[0];
    check("  .. value loads of aggregates 0 and 1 of the node", p.nodes[1].op == kExAggValue && p.nodes[1].u == ((a << 8) | 0u) && p.nodes[4].op == kExAggValue && p.nodes[4].u == ((a << 8) | 1u));
    check("  .. an id column keeps ENC_TV", nd.agg_progs[1].nodes[1].op == RDFGPU_EX_ENC_TV);
    check("  .. kept [0, 2] then two computed columns", nd.width == 4 && nd.origin[0].node < 0 && nd.origin[1].node == (int)a && nd.origin[1].agg == 1 &&
          nd.origin[2].node == (int)e && nd.origin[2].agg == 0 && nd.origin[3].node == (int)e && nd.origin[3].agg == 1); }
  { Builder b; u32 e1 = ext(b);
    u32 e2 = b.extend((int)e1, {{column(3), op(RDFGPU_EX_ENC_TV), op(RDFGPU_EX_ROUND)}, {column(3), op(RDFGPU_EX_BOUND), op(RDFGPU_EX_BOOL_AS_TV)}});
    auto nodes = expect("EXTEND over an EXTEND", b, F, RDFGPU_OK);
    const NodeInfo& nd = nodes[e2];
    check("  .. the value load names the lower node", nd.agg_progs[0].nodes[1].op == kExAggValue && nd.agg_progs[0].nodes[1].u == ((e1 << 8) | 0u) && nd.width == 6 &&
          nd.origin[3].node == (int)e1 && nd.origin[4].node == (int)e2 && nd.origin[5].node == (int)e2 && nd.origin[5].agg == 1); }
  { Builder b; u32 e = ext(b); b.aggregate((int)e, {0}, {{RDFGPU_AGG_SUM, 3}, {RDFGPU_AGG_COUNT, 3}, {RDFGPU_AGG_AVG, 3}});
    auto nodes = expect("SUM / COUNT / AVG of a computed column", b, F, RDFGPU_OK);
    check("  .. SUM as [COLUMN, value load]", nodes.back().agg_progs.size() == 2 && nodes.back().agg_progs[0].nodes[1].op == kExAggValue && nodes.back().agg_progs[0].nodes[1].u == ((e << 8) | 0u)); }
  { Builder b; u32 e = ext(b); u32 t = b.table(1, 2); b.join(RDFGPU_NODE_HASH_JOIN, (int)t, (int)e, RDFGPU_JOIN_LEFT, {{0, 0}});
    auto nodes = expect("a computed column as LEFT join payload", b, F, RDFGPU_OK);
    check("  .. origin carried through the join", nodes.back().width == 6 && nodes.back().origin[5].node == (int)e); }
  { Builder b; std::vector<Prog> eight(8, enc(1)); b.extend((int)b.table(0, 8), eight); expect("8 expressions over 8 columns: 16 outputs", b, F, RDFGPU_OK); }
  // ---- the refusals of the node itself
  { Builder b; ext(b); expect("no flag", b, 0, UNSUP, {"node 1", "RDFGPU_PLAN_AGG_COLUMNS"}); }
  { Builder b; b.extend((int)b.table(0, 3), {}); expect("k = 0", b, F, UNSUP, {"node 1", "0 expressions"}); }
  { Builder b; std::vector<Prog> nine(9, enc(1)); b.extend((int)b.table(0, 3), nine); expect("k = 9", b, F, UNSUP, {"node 1", "9 expressions"}); }
  { Builder b; b.extend((int)b.table(0, 16), {enc(1)}); expect("17 output columns", b, F, UNSUP, {"node 1", "17 output columns"}); }
  { Builder b; b.extend((int)b.table(0, 3), {{column(1), op(RDFGPU_EX_ENC_TV), column(2), op(RDFGPU_EX_ENC_TV), op(RDFGPU_EX_GT), op(RDFGPU_EX_EBV)}});
    expect("a program leaving a verdict", b, F, INVALID, {"node 1", "expression 0", "BOOLEAN_AS_TERM"}); }
  { Builder b; b.extend((int)b.table(0, 3), {enc(1), {column(1)}}); expect("a program leaving an id", b, F, INVALID, {"node 1", "expression 1", "projection"}); }
  { Builder b; b.extend((int)b.table(0, 3), {{column(1), op(RDFGPU_EX_STR), op(RDFGPU_EX_STRLEN)}}); expect("a string op (STR, STRLEN)", b, F, UNSUP, {"node 1", "expression 0", "string"}); }
  { Builder b; b.extend((int)b.table(0, 3), {{column(1), op(RDFGPU_EX_ENC_TV), op(RDFGPU_EX_CONTAINS)}}); expect("a string op (CONTAINS)", b, F, UNSUP, {"node 1", "CONTAINS"}); }
  { Builder b; u32 e = ext(b); b.nodes[e].table_slot = (u32)b.pool.size() - 1; expect("a pool pair out of range", b, F, INVALID, {"node 1", "outside the pool"}); }
  { Builder b; u32 e = ext(b); b.pool[b.nodes[e].table_slot + 1] = 99; expect("a program out of range", b, F, INVALID, {"node 1", "outside the expression array"}); }
  { Builder b; b.extend((int)b.table(0, 3), {enc(3)}); expect("a program reading a column past the input", b, F, INVALID, {"out of range"}); }
  { Builder b; b.extend((int)b.table(0, 3), {enc(1)}, {0, 3}); expect("keeping a column past the input", b, F, INVALID, {"out of range"}); }
  { Builder b; u32 e = ext(b); b.extend((int)e, {{column(3), op(RDFGPU_EX_LIT_ID, 3), op(RDFGPU_EX_ID_EQ), op(RDFGPU_EX_BOOL_AS_TV)}}); expect("ID_EQ of a computed column", b, F, INVALID, {"value column"}); }
  // ---- a computed column where ids are compared: RDFGPU_ERR_UNSUPPORTED, the text names the node and the expression
  { Builder b; u32 e = ext(b); u32 t = b.table(1, 2); b.join(RDFGPU_NODE_HASH_JOIN, (int)e, (int)t, RDFGPU_JOIN_INNER, {{3, 0}});
    expect("join key", b, F, UNSUP, {"node 3: left join key column 3", "expression 0", "node 1"}); }
  { Builder b; u32 e = ext(b); b.aggregate((int)e, {0, 3}, {}); expect("group column", b, F, UNSUP, {"node 2: group column 3", "expression 0", "node 1"}); }
  { Builder b; u32 e = ext(b); b.aggregate((int)e, {0}, {{RDFGPU_AGG_COUNT_DISTINCT, 3}}); expect("COUNT_DISTINCT input", b, F, UNSUP, {"node 2: COUNT DISTINCT input column 3", "expression 0"}); }
  { Builder b; u32 e = ext(b); auto n = Builder::blank(RDFGPU_NODE_TOPK, (int)e); n.n_keys = 2; n.left_keys[0] = 0; n.left_keys[1] = 3; n.right_keys[1] = RDFGPU_SORT_BY_DOUBLE; n.table_cols = 5; b.project(n, {0}); b.push(n);
    expect("TopK key", b, F, UNSUP, {"node 2: TopK sort key column 3", "expression 0"}); }
  { Builder b; u32 e = b.extend((int)b.table(0, 3), {enc(1), enc(2)}, {0, 1, 2}); u32 t = b.table(1, 5); b.push(Builder::blank(RDFGPU_NODE_UNION, (int)t, (int)e));
    expect("UNION input", b, F, UNSUP, {"node 3: UnionExec right input column 3", "expression 0", "node 1"}); }
  return finish();
}
