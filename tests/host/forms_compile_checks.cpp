// forms_compile_checks.cpp — the host-side checks of the functional forms and term tests (RDFGPU_EX_IF, RDFGPU_EX_COALESCE,
// RDFGPU_EX_IS_IRI .. RDFGPU_EX_IS_NUMERIC) and of LeftMark joins (RDFGPU_JOIN_LEFT_MARK; plan_compile.cpp: check_program, compile_join,
// needs_generic_vm).  `make host-checks-forms`: what tests/test_forms_cpu.py runs.
#include "compile_check_harness.hpp"

namespace {
Prog integer(long long v) { return {lit(RDFGPU_TV_INTEGER, v)}; }

// the ops, each as a program over columns 0 .. 2 that leaves a typed value
struct Form { const char* name; Prog tv; };
std::vector<Form> forms() {
  return {
      {"IF", cat({enc(0), enc(1), enc(2)}, {op(RDFGPU_EX_IF)})},
      {"COALESCE x 3", cat({enc(0), enc(1), enc(2)}, {op(RDFGPU_EX_COALESCE, 3)})},
      {"COALESCE x 1", cat({enc(0)}, {op(RDFGPU_EX_COALESCE, 1)})},
      {"COALESCE of ids", cat({{column(0)}, {column(1)}}, {op(RDFGPU_EX_COALESCE, 2), op(RDFGPU_EX_ENC_TV)})},
      {"IS_IRI", cat({enc(0)}, {op(RDFGPU_EX_IS_IRI)})},
      {"IS_BLANK", cat({enc(0)}, {op(RDFGPU_EX_IS_BLANK)})},
      {"IS_LITERAL", cat({enc(0)}, {op(RDFGPU_EX_IS_LITERAL)})},
      {"IS_NUMERIC", cat({enc(0)}, {op(RDFGPU_EX_IS_NUMERIC)})},
  };
}
Prog ebv(const Prog& p) { return cat({p}, {op(RDFGPU_EX_EBV)}); }
}  // namespace

int main() {
  static_assert(RDFGPU_EX_SECONDS == 53 && RDFGPU_EX_IF == 55 && RDFGPU_EX_COALESCE == 56 && RDFGPU_EX_IS_IRI == 57 && RDFGPU_EX_IS_NUMERIC == 60 && RDFGPU_EX__COUNT == 61, "the ops are appended");
  static_assert(RDFGPU_JOIN_LEFT_MARK == 4 && RDFGPU_JOIN_LEFT_ANTI == 3, "the join type is appended");
  static_assert(kExAggValue >= RDFGPU_EX__COUNT, "the internal op stays outside the ABI's range");
  static_assert(sizeof(rdfgpu_expr_node) == 24 && sizeof(rdfgpu_typed_value) == 16, "no struct changed size");
  char name[128];
  // ---- each op accepted in a filter, a join filter, an aggregate input and an EXTEND; always the generic VM with the cases compiled in
  for (const Form& f : forms()) {
    { Builder b; u32 t = b.table(0, 3); u32 n = b.filter((int)t, ebv(f.tv));
      std::snprintf(name, sizeof name, "FILTER EBV(%s)", f.name);
      auto nodes = expect(name, b, 0, RDFGPU_OK);
      check("  .. runs in the generic VM, in the instantiation that compiles the op in", nodes[n].shape == 0 && nodes[n].lex); }
    for (u32 type : {(u32)RDFGPU_JOIN_INNER, (u32)RDFGPU_JOIN_LEFT, (u32)RDFGPU_JOIN_LEFT_SEMI, (u32)RDFGPU_JOIN_LEFT_ANTI}) {
      Builder b; u32 l = b.table(0, 3), r = b.table(1, 2); u32 j = b.join(RDFGPU_NODE_HASH_JOIN, (int)l, (int)r, type, {{0, 0}}, ebv(f.tv));
      std::snprintf(name, sizeof name, "a hash join of type %u filtered by EBV(%s)", type, f.name);
      auto nodes = expect(name, b, 0, RDFGPU_OK);
      check("  .. takes the generic join filter", nodes[j].shape == 1 && nodes[j].lex); }
    { Builder b; u32 l = b.table(0, 3), r = b.table(1, 2); u32 j = b.join(RDFGPU_NODE_NESTED_LOOP_JOIN, (int)l, (int)r, RDFGPU_JOIN_INNER, {}, ebv(f.tv));
      std::snprintf(name, sizeof name, "a nested-loop join filtered by EBV(%s)", f.name);
      auto nodes = expect(name, b, 0, RDFGPU_OK);
      check("  .. takes the generic join filter", nodes[j].shape == 1 && nodes[j].lex); }
    { Builder b; u32 t = b.table(0, 3); u32 e = b.input_expr(f.tv); u32 a = b.aggregate((int)t, {0}, {{RDFGPU_AGG_SUM, e}, {RDFGPU_AGG_MAX, e}});
      std::snprintf(name, sizeof name, "SUM and MAX over %s", f.name);
      auto nodes = expect(name, b, F, RDFGPU_OK);
      check("  .. the programs are loaded", nodes[a].agg_progs.size() == 2 && nodes[a].agg_progs[0].n == f.tv.size() && nodes[a].lex); }
    { Builder b; u32 t = b.table(0, 3); u32 x = b.extend((int)t, {f.tv});
      std::snprintf(name, sizeof name, "EXTEND %s", f.name);
      auto nodes = expect(name, b, F, RDFGPU_OK);
      check("  .. a computed column of its own origin", nodes[x].width == 4 && nodes[x].origin[3].node == (int)x && nodes[x].origin[3].extend && nodes[x].lex); }
  }
  // HAVING over a COUNT: the value column read through ENC_TV, tested and chosen from
  { Builder b; u32 a = b.aggregate((int)b.table(0, 2), {0}, {{RDFGPU_AGG_COUNT, 1}});
    u32 f = b.filter((int)a, ebv(cat({enc(1)}, {op(RDFGPU_EX_IS_NUMERIC), integer(1)[0], integer(0)[0], op(RDFGPU_EX_IF)})));
    auto nodes = expect("HAVING EBV(IF(IS_NUMERIC(ENC_TV(count)), 1, 0))", b, F, RDFGPU_OK);
    check("  .. reads the aggregate's value", nodes[f].prog.nodes[1].op == kExAggValue && nodes[f].lex); }
  // a filter without a new op keeps its specialised shape
  { Builder b; u32 t = b.table(0, 3); rdfgpu_expr_node lit = integer(5)[0];
    u32 f = b.filter((int)t, {op(RDFGPU_EX_COLUMN, 1), op(RDFGPU_EX_ENC_TV), lit, op(RDFGPU_EX_GT), op(RDFGPU_EX_EBV)});
    auto nodes = expect("FILTER EBV(GT(ENC_TV(c1), 5)) as before", b, 0, RDFGPU_OK);
    check("  .. keeps the typed-comparison shape, without the new cases", nodes[f].shape == 2 && !nodes[f].lex); }
  // ---- what check_program refuses
  { Builder b; b.filter((int)b.table(0, 3), ebv(cat({enc(0), {op(RDFGPU_EX_EBV)}, enc(1), enc(2)}, {op(RDFGPU_EX_IF)})));
    expect("IF over a BOOL-kind test", b, 0, INVALID, {"IF test", "wrong kind"}); }
  { Builder b; b.filter((int)b.table(0, 3), ebv(cat({enc(0), enc(1)}, {op(RDFGPU_EX_IF)})));
    expect("IF with two operands", b, 0, INVALID, {"stack underflow"}); }
  { Builder b; b.filter((int)b.table(0, 3), ebv(cat({enc(0)}, {op(RDFGPU_EX_COALESCE, 0)})));
    expect("COALESCE with u = 0", b, 0, INVALID, {"COALESCE takes 1 to 8 operands, not 0"}); }
  { Builder b; b.filter((int)b.table(0, 3), ebv(cat({enc(0)}, {op(RDFGPU_EX_COALESCE, 9)})));
    expect("COALESCE with u = 9", b, 0, INVALID, {"COALESCE takes 1 to 8 operands, not 9"}); }
  { Builder b; b.filter((int)b.table(0, 3), ebv(cat({enc(0), enc(1)}, {op(RDFGPU_EX_COALESCE, 3)})));
    expect("COALESCE with more operands than the stack holds", b, 0, INVALID, {"stack underflow at COALESCE"}); }
  { Builder b; b.filter((int)b.table(0, 3), ebv(cat({{column(0)}, enc(1)}, {op(RDFGPU_EX_COALESCE, 2)})));
    expect("COALESCE mixing an id and a typed value", b, 0, INVALID, {"COALESCE mixes operand kinds"}); }
  { Builder b; b.filter((int)b.table(0, 3), ebv(cat({enc(1), {column(0)}}, {op(RDFGPU_EX_COALESCE, 2), op(RDFGPU_EX_ENC_TV)})));
    expect("COALESCE mixing a typed value and an id", b, 0, INVALID, {"COALESCE mixes operand kinds"}); }
  { Builder b; Prog eight; for (u32 k = 0; k < 8; k++) { Prog e = enc(k % 3); eight.insert(eight.end(), e.begin(), e.end()); }
    eight.push_back(op(RDFGPU_EX_COALESCE, 8));
    b.filter((int)b.table(0, 3), ebv(eight)); expect("COALESCE with 8 operands", b, 0, RDFGPU_OK); }
  { Builder b; u32 a = b.aggregate((int)b.table(0, 2), {0}, {{RDFGPU_AGG_COUNT, 1}});
    b.filter((int)a, ebv(cat({{column(1)}, {column(0)}}, {op(RDFGPU_EX_COALESCE, 2), op(RDFGPU_EX_ENC_TV)})));
    expect("COALESCE with a value column unwrapped", b, F, INVALID, {"COALESCE got an aggregate value column, whose entries are not object ids"}); }
  { Builder b; u32 a = b.aggregate((int)b.table(0, 2), {0}, {{RDFGPU_AGG_COUNT, 1}});
    b.filter((int)a, ebv(cat({enc(1), enc(0)}, {op(RDFGPU_EX_COALESCE, 2)})));
    expect("COALESCE with a value column through ENC_TV", b, F, RDFGPU_OK); }
  { Builder b; b.filter((int)b.table(0, 3), ebv(cat({{column(0)}}, {op(RDFGPU_EX_IS_IRI)})));
    expect("IS_IRI over an id operand", b, 0, INVALID, {"term test", "wrong kind"}); }
  // ---- LeftMark joins
  for (u32 kind : {(u32)RDFGPU_NODE_HASH_JOIN, (u32)RDFGPU_NODE_NESTED_LOOP_JOIN}) {
    const bool hash = kind == RDFGPU_NODE_HASH_JOIN;
    std::vector<std::pair<u32, u32>> on; if (hash) on.push_back({0, 1});
    { Builder b; u32 l = b.table(0, 3), r = b.table(1, 2); b.join(kind, (int)l, (int)r, RDFGPU_JOIN_LEFT_MARK, on);
      expect(hash ? "a mark hash join without the flag" : "a mark nested-loop join without the flag", b, 0, UNSUP, {"LeftMark join", "RDFGPU_PLAN_AGG_COLUMNS"}); }
    { Builder b; u32 l = b.table(0, 3), r = b.table(1, 2); u32 j = b.join(kind, (int)l, (int)r, RDFGPU_JOIN_LEFT_MARK, on);
      auto nodes = expect(hash ? "a mark hash join" : "a mark nested-loop join", b, F, RDFGPU_OK);
      const NodeInfo& nd = nodes[j];
      check("  .. outputs [left cols, mark], the mark a value column of the join", nd.width == 4 && nd.origin[0].node < 0 && nd.origin[2].node < 0 &&
                                                                                nd.origin[3].node == (int)j && nd.origin[3].agg == 0 && nd.origin[3].mark && !nd.origin[3].extend); }
    { Builder b; u32 l = b.table(0, 3), r = b.table(1, 2); u32 j = b.join(kind, (int)l, (int)r, RDFGPU_JOIN_LEFT_MARK, on, ebv(cat({enc(4)}, {op(RDFGPU_EX_IS_LITERAL)})), {3, 1});
      auto nodes = expect("  with a filter over [left cols, right cols] and a projection [mark, c1]", b, F, RDFGPU_OK);
      check("  .. the projection indexes [left cols, mark]", nodes[j].width == 2 && nodes[j].origin[0].node == (int)j && nodes[j].origin[0].mark && nodes[j].origin[1].node < 0 && nodes[j].shape == 1); }
    { Builder b; u32 l = b.table(0, 3), r = b.table(1, 2); b.join(kind, (int)l, (int)r, RDFGPU_JOIN_LEFT_MARK, on, {}, {0, 4});
      expect("  a projection index beyond n_left_cols", b, F, INVALID, {"projection column 4 out of range (4 columns)"}); }
  }
  { Builder b; u32 l = b.table(0, 3), r = b.table(1, 2); b.join(RDFGPU_NODE_CROSS_JOIN, (int)l, (int)r, RDFGPU_JOIN_LEFT_MARK, {});
    expect("CrossJoinExec stays inner-only", b, F, INVALID, {"CrossJoinExec takes no filter / join type"}); }
  { Builder b; u32 l = b.table(0, 3), r = b.table(1, 2); b.join(RDFGPU_NODE_HASH_JOIN, (int)l, (int)r, 5, {{0, 0}});
    expect("join type 5 is still unknown", b, F, UNSUP, {"join type 5"}); }
  { Builder b; u32 l = b.table(0, 16), r = b.table(1, 2); b.join(RDFGPU_NODE_HASH_JOIN, (int)l, (int)r, RDFGPU_JOIN_LEFT_MARK, {{0, 0}});
    expect("16 left columns and the mark", b, F, UNSUP, {"17 columns (max 16)"}); }
  // the mark above: read through ENC_TV; refused wherever a value column is
  auto mark = [](Builder& b) { u32 l = b.table(0, 2), r = b.table(1, 2); return b.join(RDFGPU_NODE_HASH_JOIN, (int)l, (int)r, RDFGPU_JOIN_LEFT_MARK, {{0, 0}}); };
  { Builder b; u32 m = mark(b);
    u32 f = b.filter((int)m, cat({ebv(cat({enc(1), integer(10)}, {op(RDFGPU_EX_GT)})), ebv(enc(2))}, {op(RDFGPU_EX_OR)}));
    auto nodes = expect("FILTER EBV(GT(ENC_TV(c1), 10)) OR EBV(ENC_TV(mark))", b, F, RDFGPU_OK);
    check("  .. the mark is loaded as a value of the join", nodes[f].prog.nodes[6].op == kExAggValue && nodes[f].prog.nodes[6].u == ((m << 8) | 0u)); }
  { Builder b; u32 m = mark(b); u32 x = b.extend((int)m, {cat({enc(2), enc(0), enc(1)}, {op(RDFGPU_EX_IF)})});
    auto nodes = expect("EXTEND IF(ENC_TV(mark), ENC_TV(c0), ENC_TV(c1))", b, F, RDFGPU_OK);
    check("  .. keeps the mark's origin beside its own", nodes[x].origin[2].node == (int)m && nodes[x].origin[2].mark && nodes[x].origin[3].node == (int)x); }
  { Builder b; u32 m = mark(b); u32 a = b.aggregate((int)m, {0}, {{RDFGPU_AGG_SUM, 2}, {RDFGPU_AGG_COUNT, 2}, {RDFGPU_AGG_AVG, 2}});
    auto nodes = expect("SUM, COUNT and AVG of the mark", b, F, RDFGPU_OK); check("  .. SUM and AVG read its value", nodes[a].agg_progs.size() == 2); }
  { Builder b; u32 m = mark(b); b.aggregate((int)m, {2}, {{RDFGPU_AGG_COUNT_STAR, 0}});
    expect("the mark as group column under RDFGPU_PLAN_VALUE_KEYS", b, F | RDFGPU_PLAN_VALUE_KEYS, RDFGPU_OK); }
  { Builder b; u32 m = mark(b); b.aggregate((int)m, {2}, {{RDFGPU_AGG_COUNT_STAR, 0}});
    expect("the mark as group column without that flag", b, F, UNSUP, {"group column 2 is a mark column (of the LeftMark join, node 2)"}); }
  { Builder b; u32 m = mark(b); auto n = Builder::blank(RDFGPU_NODE_SORT, (int)m); n.n_keys = 1; n.left_keys[0] = 2; n.right_keys[0] = RDFGPU_SORT_BY_VALUE; b.push(n);
    expect("the mark sorted BY_VALUE", b, F, RDFGPU_OK); }
  { Builder b; u32 m = mark(b); u32 t = b.table(2, 2); b.join(RDFGPU_NODE_HASH_JOIN, (int)m, (int)t, RDFGPU_JOIN_INNER, {{2, 0}});
    expect("the mark as a join key", b, F, UNSUP, {"node 4: left join key column 2 is a mark column"}); }
  { Builder b; u32 m = mark(b); b.aggregate((int)m, {0}, {{RDFGPU_AGG_COUNT_DISTINCT, 2}});
    expect("the mark under COUNT DISTINCT", b, F, UNSUP, {"node 3: COUNT DISTINCT input column 2"}); }
  { Builder b; u32 m = mark(b); auto n = Builder::blank(RDFGPU_NODE_TOPK, (int)m); n.n_keys = 1; n.left_keys[0] = 2; n.right_keys[0] = RDFGPU_SORT_BY_ID; n.table_cols = 3; b.push(n);
    expect("the mark as a TopK key", b, F, UNSUP, {"node 3: TopK sort key column 2"}); }
  { Builder b; u32 m = mark(b); u32 m2 = mark(b); auto n = Builder::blank(RDFGPU_NODE_UNION, (int)m, (int)m2); b.push(n);
    expect("marks under a UNION", b, F, UNSUP, {"UnionExec left input column 2"}); }
  // ---- a semi join's compile result is what it was
  for (u32 type : {(u32)RDFGPU_JOIN_LEFT_SEMI, (u32)RDFGPU_JOIN_LEFT_ANTI}) {
    Builder b; u32 l = b.table(0, 3), r = b.table(1, 2);
    u32 j = b.join(RDFGPU_NODE_HASH_JOIN, (int)l, (int)r, type, {{0, 0}, {1, 1}}, {op(RDFGPU_EX_COLUMN, 1), op(RDFGPU_EX_COLUMN, 4), op(RDFGPU_EX_ID_NEQ)}, {2, 0});
    auto nodes = expect(type == RDFGPU_JOIN_LEFT_SEMI ? "a semi join" : "an anti join", b, 0, RDFGPU_OK);
    const NodeInfo& nd = nodes[j];
    check("  .. left columns only, the id-pair filter shape, no value column, no new cases", nd.width == 2 && nd.n_proj == 2 && nd.proj[0] == 2 && nd.proj[1] == 0 && nd.shape == 2 &&
                                                                                          !nd.lex && nd.origin[0].node < 0 && nd.origin[1].node < 0 && nd.prog.n == 3);
    Builder c; u32 l2 = c.table(0, 3), r2 = c.table(1, 2); c.join(RDFGPU_NODE_HASH_JOIN, (int)l2, (int)r2, type, {{0, 0}}, {}, {3});
    expect("  .. its projection still indexes the left columns only", c, 0, INVALID, {"projection column 3 out of range (3 columns)"});
  }
  return finish();
}
