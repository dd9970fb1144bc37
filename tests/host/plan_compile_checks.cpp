// plan_compile_checks.cpp — the host-side checks of aggregate values as columns (RDFGPU_PLAN_AGG_COLUMNS; plan_compile.cpp: compile_nodes
// and what it calls, check_program included), and the pin of the op table (expr_ops.hpp).  `make host-checks`: what
// tests/test_agg_columns_cpu.py runs.  Every case is a plan description with the flag (or without it) and the status its compilation
// must end in; a refusal's text must name the node.
#include "compile_check_harness.hpp"

namespace {
std::vector<rdfgpu_expr_node> value_gt(u32 c, int64_t k) {   // EBV(GT(ENC_TV(col c), integer k))
  return {column(c), op(RDFGPU_EX_ENC_TV), op(RDFGPU_EX_LIT_TV, 0, RDFGPU_TV_INTEGER, k), op(RDFGPU_EX_GT), op(RDFGPU_EX_EBV)};
}

// table(0: k, x, y) -> AggregateExec gby=[k] aggr=[COUNT(*), SUM(x)]: columns k, COUNT(*), SUM(x); node 1
u32 agg(Builder& b) { return b.aggregate((int)b.table(0, 3), {0}, {{RDFGPU_AGG_COUNT_STAR, 0}, {RDFGPU_AGG_SUM, 1}}); }

// The pin of op_traits (expr_ops.hpp): every trait against its list written out, as plan compilation spelled it before the table existed.
// A new op that belongs to a list and is missing from it in op_traits, or the other way round, fails here.
struct TraitList { const char* name; u32 trait; std::vector<u32> ops; };
const std::vector<TraitList> kTraitLists = {
    {"kOpCmp", kOpCmp, {RDFGPU_EX_GT, RDFGPU_EX_LT, RDFGPU_EX_GEQ, RDFGPU_EX_LEQ, RDFGPU_EX_EQ, RDFGPU_EX_NEQ}},
    {"kOpSlot", kOpSlot, {RDFGPU_EX_REGEX, RDFGPU_EX_CONTAINS, RDFGPU_EX_STRSTARTS, RDFGPU_EX_STRENDS, RDFGPU_EX_LANG_IN, RDFGPU_EX_LIT_STR}},
    {"kOpNeedle", kOpNeedle, {RDFGPU_EX_CONTAINS, RDFGPU_EX_STRSTARTS, RDFGPU_EX_STRENDS}},
    {"kOpPattern", kOpPattern, {RDFGPU_EX_REGEX, RDFGPU_EX_REGEX_VAR, RDFGPU_EX_CONTAINS, RDFGPU_EX_STRSTARTS, RDFGPU_EX_STRENDS, RDFGPU_EX_LANG_IN}},
    {"kOpView", kOpView, {RDFGPU_EX_STR, RDFGPU_EX_LIT_STR, RDFGPU_EX_SUBSTR, RDFGPU_EX_UCASE, RDFGPU_EX_LCASE, RDFGPU_EX_STRBEFORE, RDFGPU_EX_STRAFTER, RDFGPU_EX_CAST_STRING}},
    {"kOpStringFn", kOpStringFn, {RDFGPU_EX_STR, RDFGPU_EX_LIT_STR, RDFGPU_EX_STRLEN, RDFGPU_EX_SUBSTR, RDFGPU_EX_UCASE, RDFGPU_EX_LCASE, RDFGPU_EX_STRBEFORE, RDFGPU_EX_STRAFTER}},
    {"kOpStoreStrings", kOpStoreStrings, {RDFGPU_EX_STR, RDFGPU_EX_STRLEN, RDFGPU_EX_SUBSTR, RDFGPU_EX_UCASE, RDFGPU_EX_LCASE, RDFGPU_EX_STRBEFORE, RDFGPU_EX_STRAFTER, RDFGPU_EX_CAST_STRING, RDFGPU_EX_CAST_LEX}},
    {"kOpGenericVm", kOpGenericVm, {kExAggValue, RDFGPU_EX_CAST_STRING, RDFGPU_EX_CAST_LEX, RDFGPU_EX_YEAR, RDFGPU_EX_MONTH, RDFGPU_EX_DAY, RDFGPU_EX_HOURS, RDFGPU_EX_MINUTES, RDFGPU_EX_SECONDS,
                                    RDFGPU_EX_IF, RDFGPU_EX_COALESCE, RDFGPU_EX_IS_IRI, RDFGPU_EX_IS_BLANK, RDFGPU_EX_IS_LITERAL, RDFGPU_EX_IS_NUMERIC}},
    {"kOpExtended", kOpExtended, {RDFGPU_EX_CAST_LEX, RDFGPU_EX_YEAR, RDFGPU_EX_MONTH, RDFGPU_EX_DAY, RDFGPU_EX_HOURS, RDFGPU_EX_MINUTES, RDFGPU_EX_SECONDS,
                                  RDFGPU_EX_IF, RDFGPU_EX_COALESCE, RDFGPU_EX_IS_IRI, RDFGPU_EX_IS_BLANK, RDFGPU_EX_IS_LITERAL, RDFGPU_EX_IS_NUMERIC}},
    {"kOpDatePart", kOpDatePart, {RDFGPU_EX_YEAR, RDFGPU_EX_MONTH, RDFGPU_EX_DAY, RDFGPU_EX_HOURS, RDFGPU_EX_MINUTES, RDFGPU_EX_SECONDS}},
    {"kOpForm", kOpForm, {RDFGPU_EX_IF, RDFGPU_EX_COALESCE, RDFGPU_EX_IS_IRI, RDFGPU_EX_IS_BLANK, RDFGPU_EX_IS_LITERAL, RDFGPU_EX_IS_NUMERIC}},
};
// check_program knows the op: alone on an empty stack it is refused for its operands or accepted, never as "unknown op"
bool check_program_knows(u32 o) {
  const rdfgpu_expr_node e = op((u8)o);
  try { check_program(&e, 1, 1, 1); } catch (const Error& err) { return std::string(err.what()).find("unknown op") == std::string::npos; }
  return true;
}
void pin_op_traits() {
  char name[96];
  for (const TraitList& t : kTraitLists) {
    bool ok = true;
    for (u32 o = 0; o < 256; o++) {   // the ABI's ops 1 .. RDFGPU_EX__COUNT - 1, the internal op, and nothing beyond them
      const bool listed = std::find(t.ops.begin(), t.ops.end(), o) != t.ops.end();
      ok = ok && op_is(o, t.trait) == listed;
    }
    std::snprintf(name, sizeof name, "op_traits: %s marks its %u ops and no other", t.name, (u32)t.ops.size());
    check(name, ok);
  }
  bool entries = true;
  for (u32 o = 0; o < 256; o++) entries = entries && op_is(o, kOpKnown) == (check_program_knows(o) || o == kExAggValue);
  check("op_traits: an entry for every op check_program accepts, and for the value load", entries);
  check("  .. the unused value 54 has none", op_traits(54) == 0 && !check_program_knows(54) && op_traits(0) == 0 && op_traits(RDFGPU_EX__COUNT) == 0);
}
}  // namespace

int main() {
  // ---- what compiles, and what the compiled plan knows about its value columns
  {
    Builder b; u32 a = agg(b);
    u32 f = b.filter((int)a, value_gt(1, 3), {2, 0});
    auto nodes = expect("HAVING over an aggregate", b, F, RDFGPU_OK);
    const NodeInfo& nd = nodes[f];
    bool ok = nd.prog.n == 5 && nd.prog.nodes[1].op == kExAggValue && nd.prog.nodes[1].u == ((a << 8) | 0u) && nd.shape == 0 &&
              nd.origin[0].node == (int)a && nd.origin[0].agg == 1 && nd.origin[1].node < 0 && nodes[a].width == 3;
    check("  .. rewritten to a value load, VM shape", ok);
  }
  { Builder b; u32 a = agg(b); b.filter((int)a, value_gt(0, 3));   // the key column: an ordinary ENC_TV, the specialised shape
    auto nodes = expect("filter on the key column of an aggregate", b, F, RDFGPU_OK);
    bool ok = nodes.back().prog.nodes[1].op == RDFGPU_EX_ENC_TV && nodes.back().shape == 2;
    check("  .. keeps ENC_TV and its shape", ok); }
  { Builder b; u32 a = agg(b); u32 t = b.table(1, 2);
    b.join(RDFGPU_NODE_HASH_JOIN, (int)t, (int)a, RDFGPU_JOIN_LEFT, {{0, 0}}, {column(1), op(RDFGPU_EX_ENC_TV), column(4), op(RDFGPU_EX_ENC_TV), op(RDFGPU_EX_GT), op(RDFGPU_EX_EBV)}, {0, 4, 3});
    auto nodes = expect("LEFT join, filter over both sides", b, F, RDFGPU_OK);
    const NodeInfo& nd = nodes.back();
    bool ok = nd.prog.nodes[1].op == RDFGPU_EX_ENC_TV && nd.prog.nodes[3].op == kExAggValue && nd.shape == 1 && nd.origin[1].agg == 1 && nd.origin[2].agg == 0 && nd.origin[0].node < 0;
    check("  .. origins through the projection", ok); }
  { Builder b; u32 a = agg(b); u32 t = b.table(1, 2); b.join(RDFGPU_NODE_HASH_JOIN, (int)t, (int)a, RDFGPU_JOIN_LEFT_SEMI, {{0, 0}}, value_gt(4, 1));
    auto nodes = expect("semi join reads the right side's value", b, F, RDFGPU_OK);
    bool ok = nodes.back().width == 2 && nodes.back().origin[0].node < 0 && nodes.back().origin[1].node < 0;
    check("  .. hands on its left side only", ok); }
  { Builder b; u32 a = agg(b); b.aggregate((int)a, {0}, {{RDFGPU_AGG_SUM, 1}, {RDFGPU_AGG_COUNT, 2}, {RDFGPU_AGG_AVG, 2}});
    auto nodes = expect("aggregate over an aggregate", b, F, RDFGPU_OK);
    const NodeInfo& nd = nodes.back();
    bool ok = nd.agg_prog[0] == 0 && nd.agg_prog[1] < 0 && nd.agg_prog[2] == 1 && nd.agg_progs[0].n == 2 && nd.agg_progs[0].nodes[1].op == kExAggValue &&
              nd.agg_progs[1].nodes[1].u == ((a << 8) | 1u) && nd.width == 4 && nd.origin[3].node == (int)nodes.size() - 1;
    check("  .. SUM / AVG as [COLUMN, value load]", ok); }
  { Builder b; u32 a = agg(b); u32 g = b.aggregate((int)b.table(1, 2), {}, {{RDFGPU_AGG_AVG, 1}}); u32 x = b.join(RDFGPU_NODE_CROSS_JOIN, (int)a, (int)g, RDFGPU_JOIN_INNER, {});
    b.filter((int)x, {column(2), op(RDFGPU_EX_ENC_TV), column(3), op(RDFGPU_EX_ENC_TV), op(RDFGPU_EX_LIT_TV, 0, RDFGPU_TV_INTEGER, 2), op(RDFGPU_EX_MUL), op(RDFGPU_EX_GT), op(RDFGPU_EX_EBV)});
    expect("cross join with a zero-key aggregate", b, F, RDFGPU_OK); }
  { Builder b; u32 a = agg(b); b.filter((int)a, {column(2), op(RDFGPU_EX_BOUND)});
    expect("BOUND of a value column", b, F, RDFGPU_OK); }
  // ---- opt-in: the same descriptions without the flag
  { Builder b; u32 a = agg(b); b.filter((int)a, value_gt(1, 3)); expect("no flag: filter over an aggregate", b, 0, UNSUP, {"must be the plan's root"}); }
  { Builder b; u32 a = agg(b); b.aggregate((int)a, {0}, {{RDFGPU_AGG_SUM, 1}}); expect("no flag: aggregate over an aggregate", b, 0, UNSUP, {"must be the plan's root"}); }
  { Builder b; agg(b); auto nodes = expect("no flag: the root form", b, 0, RDFGPU_OK); failures += nodes.back().width != 1; }
  // ---- refusals under the flag: RDFGPU_ERR_UNSUPPORTED, the text names node and column
  { Builder b; u32 a = agg(b); u32 t = b.table(1, 2); b.join(RDFGPU_NODE_HASH_JOIN, (int)a, (int)t, RDFGPU_JOIN_INNER, {{2, 0}}); expect("left join key", b, F, UNSUP, {"node 3: left join key column 2"}); }
  { Builder b; u32 a = agg(b); u32 t = b.table(1, 2); b.join(RDFGPU_NODE_HASH_JOIN, (int)t, (int)a, RDFGPU_JOIN_LEFT_ANTI, {{0, 0}, {1, 1}}); expect("right join key of an anti join", b, F, UNSUP, {"node 3: right join key column 1"}); }
  { Builder b; u32 a = agg(b); b.aggregate((int)a, {0, 1}, {}); expect("group column", b, F, UNSUP, {"node 2: group column 1"}); }
  { Builder b; u32 a = agg(b); b.aggregate((int)a, {0}, {{RDFGPU_AGG_COUNT_DISTINCT, 2}}); expect("COUNT DISTINCT input", b, F, UNSUP, {"node 2: COUNT DISTINCT input column 2"}); }
  { Builder b; u32 a = agg(b); auto n = Builder::blank(RDFGPU_NODE_TOPK, (int)a); n.n_keys = 2; n.left_keys[0] = 0; n.left_keys[1] = 2; n.right_keys[1] = RDFGPU_SORT_BY_DOUBLE; n.table_cols = 5; b.project(n, {0}); b.push(n);
    expect("TopK sort key", b, F, UNSUP, {"node 2: TopK sort key column 2"}); }
  { Builder b; u32 a = agg(b); auto n = Builder::blank(RDFGPU_NODE_TOPK, (int)a); n.n_keys = 1; n.left_keys[0] = 0; n.table_cols = 5; b.project(n, {0, 1}); b.push(n);
    expect("TopK output", b, F, UNSUP, {"node 2: TopK output column 1"}); }
  { Builder b; u32 a = agg(b); auto n = Builder::blank(RDFGPU_NODE_TOPK, (int)a); n.n_keys = 1; n.left_keys[0] = 0; n.table_cols = 5; n.table_slot = 2; b.project(n, {0}); b.push(n);
    expect("TopK group", b, F, UNSUP, {"node 2: TopK group column 1"}); }
  { Builder b; u32 a = agg(b); b.push(Builder::blank(RDFGPU_NODE_CLOSURE, (int)a)); expect("CLOSURE input", b, F, UNSUP, {"node 2: KleenePlusClosureExec input column 1"}); }
  { Builder b; u32 a = agg(b); u32 t = b.table(1, 3); b.push(Builder::blank(RDFGPU_NODE_UNION, (int)t, (int)a)); expect("UNION input", b, F, UNSUP, {"node 3: UnionExec right input column 1"}); }
  { Builder b; u32 a = agg(b); auto p = Builder::blank(RDFGPU_NODE_PROJECTION, (int)a); b.project(p, {2, 2, 0}); u32 pr = b.push(p); u32 t = b.table(1, 2);
    b.join(RDFGPU_NODE_HASH_JOIN, (int)pr, (int)t, RDFGPU_JOIN_INNER, {{1, 0}}); expect("a key behind a projection", b, F, UNSUP, {"node 4: left join key column 1"}); }
  // ---- kind errors: RDFGPU_ERR_INVALID
  { Builder b; u32 a = agg(b); b.filter((int)a, {column(1), op(RDFGPU_EX_LIT_ID, 3), op(RDFGPU_EX_ID_EQ)}); expect("ID_EQ of a value column", b, F, INVALID, {"aggregate value column"}); }
  { Builder b; u32 a = agg(b); b.filter((int)a, {column(0), column(2), op(RDFGPU_EX_ID_NEQ)}); expect("ID_NEQ of a value column", b, F, INVALID, {"aggregate value column"}); }
  { Builder b; u32 a = agg(b); b.filter((int)a, {column(2), column(0), op(RDFGPU_EX_IS_COMPATIBLE)}); expect("IS_COMPATIBLE of a value column", b, F, INVALID, {"aggregate value column"}); }
  { Builder b; u32 a = agg(b); b.filter((int)a, {column(1), op(RDFGPU_EX_STR), op(RDFGPU_EX_STRLEN), op(RDFGPU_EX_EBV)}); expect("STR of a value column", b, F, INVALID, {"aggregate value column"}); }
  { Builder b; u32 a = agg(b); b.filter((int)a, {column(1), op(kExAggValue), op(RDFGPU_EX_EBV)}); expect("the internal op in a description", b, F, INVALID, {"unknown op"}); }
  { Builder b; u32 a = agg(b); b.filter((int)a, {column(3), op(RDFGPU_EX_BOUND)}); expect("a column past the value columns", b, F, INVALID, {"out of range"}); }
  { Builder b; u32 a = agg(b); b.aggregate((int)a, {0}, {{RDFGPU_AGG_SUM, 3}}); expect("an aggregate input past the value columns", b, F, INVALID, {"reads column 3 of 3"}); }
  // ---- the op table
  pin_op_traits();
  return finish();
}
