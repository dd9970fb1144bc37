// value_keys_compile_checks.cpp — the host-side checks of the date parts (RDFGPU_EX_YEAR .. RDFGPU_EX_SECONDS) and of GROUP BY over value
// columns and up to 8 group columns (RDFGPU_PLAN_VALUE_KEYS; plan_compile.cpp: check_program, compile_aggregate, check_plan_flags).
// `make host-checks-value-keys`: what tests/test_dateparts_cpu.py runs.
#include "compile_check_harness.hpp"

namespace {
constexpr u32 V = RDFGPU_PLAN_AGG_COLUMNS | RDFGPU_PLAN_VALUE_KEYS;
// the program `o`(ENC_TV(col c)) (of_value = false: `o`(col c), an id operand), followed by `tail`
Prog part(u32 c, bool of_value, u8 o, std::vector<u8> tail = {}) {
  Prog p = of_value ? enc(c) : Prog{column(c)};
  p.push_back(op(o));
  for (u8 t : tail) p.push_back(t == RDFGPU_EX_LIT_TV ? lit(RDFGPU_TV_INTEGER, 2024) : op(t));
  return p;
}
const u8 PARTS[6] = {RDFGPU_EX_YEAR, RDFGPU_EX_MONTH, RDFGPU_EX_DAY, RDFGPU_EX_HOURS, RDFGPU_EX_MINUTES, RDFGPU_EX_SECONDS};
const char* const PART_NAMES[6] = {"YEAR", "MONTH", "DAY", "HOURS", "MINUTES", "SECONDS"};
// the Wind Farm tail: table(site, wtur, val, tv) -> EXTEND(year .. minute of tv) -> AggregateExec by 2 ids + 5 values, AVG(val)
u32 windfarm(Builder& b) {
  const u32 t = b.table(0, 4);
  const u32 x = b.extend((int)t, {part(3, true, RDFGPU_EX_YEAR), part(3, true, RDFGPU_EX_MONTH), part(3, true, RDFGPU_EX_DAY),
                                  part(3, true, RDFGPU_EX_HOURS), part(3, true, RDFGPU_EX_MINUTES)});
  return b.aggregate((int)x, {0, 1, 4, 5, 6, 7, 8}, {{RDFGPU_AGG_AVG, 2}});
}
}  // namespace

int main() {
  static_assert(RDFGPU_EX_YEAR == 48 && RDFGPU_EX_SECONDS == 53 && RDFGPU_PLAN_VALUE_KEYS == 4u && RDFGPU_MAX_GROUP_KEYS == 8u && RDFGPU_MAX_KEYS == 4u, "the header's constants");
  static_assert(sizeof(rdfgpu_typed_value) == 16 && offsetof(rdfgpu_typed_value, tz_minutes) == 14 && sizeof(rdfgpu_expr_node) == 24, "no struct changed size");
  // ---- the six ops: TV -> TV, wherever MUL is allowed; refused over an id operand
  for (int p = 0; p < 6; p++) {
    char name[96];
    { Builder b; u32 t = b.table(0, 2); u32 f = b.filter((int)t, part(1, true, PARTS[p], {RDFGPU_EX_LIT_TV, RDFGPU_EX_EQ, RDFGPU_EX_EBV}));
      std::snprintf(name, sizeof name, "FILTER EBV(EQ(%s(ENC_TV(c1)), 2024))", PART_NAMES[p]);
      auto nodes = expect(name, b, 0, RDFGPU_OK);
      check("  .. runs in the generic VM, in the instantiation that compiles the op in", nodes[f].shape == 0 && nodes[f].lex); }
    { Builder b; b.filter((int)b.table(0, 2), part(1, false, PARTS[p], {RDFGPU_EX_LIT_TV, RDFGPU_EX_EQ, RDFGPU_EX_EBV}));
      std::snprintf(name, sizeof name, "%s over an id operand", PART_NAMES[p]);
      expect(name, b, 0, INVALID, {"date part", "wrong kind"}); }
    { Builder b; u32 t = b.table(0, 2); u32 x = b.extend((int)t, {part(1, true, PARTS[p])});
      std::snprintf(name, sizeof name, "EXTEND %s(ENC_TV(c1))", PART_NAMES[p]);
      auto nodes = expect(name, b, F, RDFGPU_OK);
      check("  .. a computed column of its own origin", nodes[x].width == 3 && nodes[x].origin[2].node == (int)x && nodes[x].origin[2].extend && nodes[x].lex); }
  }
  { Builder b; u32 t = b.table(0, 3); u32 e = b.input_expr(part(2, true, RDFGPU_EX_HOURS)); u32 a = b.aggregate((int)t, {0}, {{RDFGPU_AGG_AVG, e}, {RDFGPU_AGG_MAX, e}});
    auto nodes = expect("AVG and MAX over HOURS(ENC_TV(c2))", b, F, RDFGPU_OK);
    check("  .. the programs are loaded", nodes[a].agg_progs.size() == 2 && nodes[a].agg_progs[0].n == 3 && nodes[a].lex); }
  { Builder b; u32 l = b.table(0, 2), r = b.table(1, 2); u32 j = b.join(RDFGPU_NODE_HASH_JOIN, (int)l, (int)r, RDFGPU_JOIN_INNER, {{0, 0}}, part(3, true, RDFGPU_EX_MONTH, {RDFGPU_EX_LIT_TV, RDFGPU_EX_GT, RDFGPU_EX_EBV}));
    auto nodes = expect("a join filter with MONTH", b, 0, RDFGPU_OK);
    check("  .. takes the generic join filter", nodes[j].shape == 1 && nodes[j].lex); }
  { Builder b; b.filter((int)b.table(0, 2), part(1, true, 54, {RDFGPU_EX_EBV})); expect("op 54 is still unknown", b, 0, INVALID, {"unknown op 54"}); }
  // ---- RDFGPU_PLAN_VALUE_KEYS: 5..8 keys, value keys, the origins of the output
  { Builder b; u32 a = windfarm(b);
    auto nodes = expect("the Wind Farm list: 2 id + 5 value keys, AVG", b, V, RDFGPU_OK);
    const NodeInfo& nd = nodes[a];
    bool ok = nd.width == 8 && nd.origin[0].node < 0 && nd.origin[1].node < 0 && nd.origin[7].node == (int)a && nd.origin[7].agg == 0 && !nd.origin[7].extend;
    for (u32 k = 2; k < 7; k++) ok = ok && nd.origin[k].node == 1 && nd.origin[k].agg == k - 2 && nd.origin[k].extend;
    check("  .. value keys keep the EXTEND's origins, then the AVG's own", ok); }
  for (u32 nk = 5; nk <= 8; nk++) {
    Builder b; std::vector<u32> keys; for (u32 k = 0; k < nk; k++) keys.push_back(nk - 1 - k);
    u32 a = b.aggregate((int)b.table(0, nk + 1), keys, {{RDFGPU_AGG_COUNT, nk}});
    char name[64]; std::snprintf(name, sizeof name, "%u id keys", nk);
    auto nodes = expect(name, b, V, RDFGPU_OK);
    check("  .. keys, then the value column", nodes[a].width == nk + 1 && nodes[a].origin[nk - 1].node < 0 && nodes[a].origin[nk].node == (int)a && agg_key_col(nodes[a].d, nk - 1) == 0); }
  { Builder b; u32 c = b.aggregate((int)b.table(0, 2), {0}, {{RDFGPU_AGG_COUNT, 1}}); u32 a = b.aggregate((int)c, {1}, {{RDFGPU_AGG_COUNT_STAR, 0}});
    auto nodes = expect("a COUNT's value column alone as key", b, V, RDFGPU_OK);
    check("  .. stays that COUNT's value column", nodes[a].width == 2 && nodes[a].origin[0].node == (int)c && nodes[a].origin[1].node == (int)a); }
  { Builder b; b.aggregate((int)b.table(0, 8), {0, 1, 2, 3, 4, 5, 6, 7}, {{1, 0}, {1, 0}, {1, 0}, {1, 0}, {1, 0}, {1, 0}, {1, 0}, {1, 0}});
    auto nodes = expect("8 keys + 8 aggregates = 16 columns", b, V, RDFGPU_OK); check("  .. fit", nodes.back().width == 16); }
  { Builder b; b.aggregate((int)b.table(0, 9), {0, 1, 2, 3, 4, 5, 6, 7, 8}, {}); expect("9 keys", b, V, UNSUP, {"node 1: AggregateExec with 9 group columns (at most 8)"}); }
  { Builder b; b.aggregate((int)b.table(0, 6), {0, 1, 2, 3, 9}, {}); expect("key 4 out of range (right_keys[] is read)", b, V, INVALID, {"node 1: group column 9 out of range"}); }
  { Builder b; windfarm(b); expect("the flag without RDFGPU_PLAN_AGG_COLUMNS", b, RDFGPU_PLAN_VALUE_KEYS, INVALID, {"RDFGPU_PLAN_VALUE_KEYS", "RDFGPU_PLAN_AGG_COLUMNS"}); }
  // ---- without the flag: the texts of today, verbatim
  { Builder b; b.aggregate((int)b.table(0, 5), {0, 1, 2, 3, 4}, {}); expect("5 keys without the flag", b, F, UNSUP, {"node 1: AggregateExec with 5 group columns (at most 4)"}); }
  { Builder b; b.aggregate((int)b.table(0, 5), {0, 1, 2, 3, 4}, {}); expect("5 keys without any flag", b, 0, UNSUP, {"node 1: AggregateExec with 5 group columns (at most 4)"}); }
  { Builder b; u32 c = b.aggregate((int)b.table(0, 2), {0}, {{RDFGPU_AGG_COUNT, 1}}); b.aggregate((int)c, {1}, {});
    expect("an aggregate's value column as group column, no flag", b, F, UNSUP,
           {"node 2: group column 1 is an aggregate value column (aggregate 0 of node 1): its entries index values, equal values have different indexes"}); }
  { Builder b; u32 x = b.extend((int)b.table(0, 4), {part(3, true, RDFGPU_EX_YEAR)}); b.aggregate((int)x, {0, 4}, {});
    expect("a computed column as group column, no flag", b, F, UNSUP,
           {"node 2: group column 4 is a computed value column (expression 0 of the ProjectionExec with expressions, node 1): its entries index values, equal values have different indexes"}); }
  // ---- with the flag: the other roles of a value column stay refused, with their texts
  { Builder b; u32 a = windfarm(b); u32 t = b.table(1, 2); b.join(RDFGPU_NODE_HASH_JOIN, (int)a, (int)t, RDFGPU_JOIN_INNER, {{2, 0}});
    expect("a value key's column as join key", b, V, UNSUP, {"node 4: left join key column 2 is a computed value column (expression 0 of the ProjectionExec with expressions, node 1)"}); }
  { Builder b; u32 a = windfarm(b); u32 t = b.table(1, 2); b.join(RDFGPU_NODE_HASH_JOIN, (int)a, (int)t, RDFGPU_JOIN_INNER, {{7, 0}});
    expect("the AVG's column as join key", b, V, UNSUP, {"node 4: left join key column 7 is an aggregate value column (aggregate 0 of node 2)"}); }
  { Builder b; u32 c = b.aggregate((int)b.table(0, 2), {0}, {{RDFGPU_AGG_COUNT, 1}}); b.aggregate((int)c, {0}, {{RDFGPU_AGG_COUNT_DISTINCT, 1}});
    expect("a value column under COUNT DISTINCT", b, V, UNSUP, {"node 2: COUNT DISTINCT input column 1"}); }
  { Builder b; u32 a = windfarm(b); auto n = Builder::blank(RDFGPU_NODE_TOPK, (int)a); n.n_keys = 1; n.left_keys[0] = 2; n.right_keys[0] = RDFGPU_SORT_BY_ID; n.table_cols = 3; b.push(n);
    expect("a value key's column as TopK key", b, V, UNSUP, {"node 3: TopK sort key column 2"}); }
  { Builder b; u32 a = windfarm(b); u32 a2 = windfarm(b); auto n = Builder::blank(RDFGPU_NODE_UNION, (int)a, (int)a2); b.push(n);
    expect("value keys under a UNION", b, V, UNSUP, {"UnionExec left input column 2"}); }
  { Builder b; u32 t = b.table(0, 2); auto n = Builder::blank(RDFGPU_NODE_SORT, (int)t); n.n_keys = 5; b.push(n);
    expect("SortExec keeps its 4 keys", b, V, UNSUP, {"SortExec with 5 sort keys (1 to 4)"}); }
  return finish();
}
