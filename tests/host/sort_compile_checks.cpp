// sort_compile_checks.cpp — the host-side checks of SortExec (RDFGPU_NODE_SORT; plan_compile.cpp: compile_sort and what it calls).
// `make host-checks-sort`: what tests/test_sort_cpu.py runs.
#include "compile_check_harness.hpp"

namespace {
constexpr u32 ID = RDFGPU_SORT_BY_ID, TERM = RDFGPU_SORT_BY_TERM, DOUBLE = RDFGPU_SORT_BY_DOUBLE, VALUE = RDFGPU_SORT_BY_VALUE;
// table(0: product, x, y) -> EXTEND [ENC_TV(x)]: columns product, x, y, value; node 1, its computed column is column 3
u32 ext(Builder& b) { return b.extend((int)b.table(0, 3), {enc(1)}); }
}  // namespace

int main() {
  // ---- what compiles, and what the node is typed as
  { Builder b; b.sort((int)b.table(0, 3), {{1, ID, true}});
    auto nodes = expect("one id key, no flag, no fetch", b, 0, RDFGPU_OK);
    check("  .. width, record of 2 words, id origins", nodes.back().width == 3 && nodes.back().sort_words == 2 && nodes.back().origin[1].node < 0); }
  { Builder b; u32 e = ext(b); u32 s = b.sort((int)e, {{3, VALUE, true}, {0, ID, false}}, 10);
    auto nodes = expect("the Q3 shape: (value DESC, id ASC), fetch 10", b, F, RDFGPU_OK);
    const NodeInfo& nd = nodes[s];
    check("  .. 6 words; the value column keeps its origin", nd.sort_words == 6 && nd.width == 4 && nd.origin[3].node == (int)e && nd.origin[3].extend && nd.origin[0].node < 0 && nd.d.table_cols == 10); }
  { Builder b; u32 a = b.aggregate((int)b.table(0, 2), {0}, {{RDFGPU_AGG_COUNT, 1}}); u32 s = b.sort((int)a, {{1, VALUE, true}}, 10, {1, 0});
    auto nodes = expect("the Q1 shape: an aggregate's value, projected", b, F, RDFGPU_OK);
    check("  .. the projection carries the origin", nodes[s].width == 2 && nodes[s].origin[0].node == (int)a && nodes[s].origin[1].node < 0 && nodes[s].sort_words == 5); }
  { Builder b; u32 e = ext(b); b.sort((int)e, {{3, VALUE, false}, {0, ID, true}, {1, DOUBLE, true}, {2, TERM, false}});
    auto nodes = expect("the widest record: value + three id forms", b, F, RDFGPU_OK);
    check("  .. 8 words", nodes.back().sort_words == kSortMaxWords); }
  { Builder b; b.sort((int)b.table(0, 3), {{0, ID, false}, {0, ID, true}, {1, TERM, false}, {2, DOUBLE, true}}); expect("four id keys, a column twice", b, 0, RDFGPU_OK); }
  { Builder b; u32 e = ext(b); u32 s = b.sort((int)e, {{3, VALUE, true}}); u32 x = b.extend((int)s, {enc(0)}); b.sort((int)x, {{4, VALUE, false}, {0, ID, false}});
    auto nodes = expect("SORT under EXTEND under SORT", b, F, RDFGPU_OK);
    check("  .. origins of both nodes above", nodes.back().width == 5 && nodes.back().origin[3].node == (int)e && nodes.back().origin[4].node == (int)x); }
  { Builder b; u32 e = ext(b); u32 s = b.sort((int)e, {{3, VALUE, true}}); auto f = Builder::blank(RDFGPU_NODE_PROJECTION, (int)s); b.project(f, {3, 0}); b.push(f);
    auto nodes = expect("SORT under PROJECTION", b, F, RDFGPU_OK);
    check("  .. origin carried", nodes.back().origin[0].node == (int)e && nodes.back().width == 2); }
  // ---- the refusals
  { Builder b; b.sort((int)b.table(0, 3), {}); expect("no key", b, 0, UNSUP, {"node 1", "SortExec with 0 sort keys"}); }
  { Builder b; u32 s = b.sort((int)b.table(0, 3), {{0, ID, false}}); b.nodes[s].n_keys = 5; expect("five keys", b, 0, UNSUP, {"node 1", "SortExec with 5 sort keys (1 to 4)"}); }
  { Builder b; b.sort((int)b.table(0, 3), {{3, ID, false}}); expect("a key column past the input", b, 0, INVALID, {"node 1", "sort key column 3 out of range"}); }
  { Builder b; b.sort((int)b.table(0, 3), {{0, 4, false}}); expect("an unknown mode", b, 0, INVALID, {"node 1", "unknown sort mode"}); }
  { Builder b; u32 e = ext(b); b.sort((int)e, {{0, VALUE, false}}); expect("BY_VALUE on an id column", b, F, INVALID, {"node 2", "RDFGPU_SORT_BY_VALUE of column 0", "object ids"}); }
  { Builder b; u32 e = ext(b); b.sort((int)e, {{3, ID, false}});
    expect("BY_ID on a computed column", b, F, UNSUP, {"node 2: SortExec key by id / term / double column 3 is a computed value column", "expression 0", "node 1"}); }
  { Builder b; u32 e = ext(b); b.sort((int)e, {{0, ID, false}, {3, DOUBLE, true}}); expect("BY_DOUBLE on a computed column", b, F, UNSUP, {"node 2", "column 3 is a computed value column"}); }
  { Builder b; u32 a = b.aggregate((int)b.table(0, 2), {0}, {{RDFGPU_AGG_COUNT, 1}}); b.sort((int)a, {{1, TERM, false}});
    expect("BY_TERM on an aggregate's column", b, F, UNSUP, {"node 2", "column 1 is an aggregate value column", "aggregate 0 of node 1"}); }
  { Builder b; b.sort((int)b.table(0, 3), {{1, VALUE, true}}); expect("BY_VALUE without the flag", b, 0, UNSUP, {"node 1", "RDFGPU_PLAN_AGG_COLUMNS"}); }
  { Builder b; u32 a = b.aggregate((int)b.table(0, 2), {0}, {{RDFGPU_AGG_COUNT, 1}}); b.sort((int)a, {{0, ID, false}});
    expect("over an aggregate's values without the flag", b, 0, UNSUP, {"node 2", "AggregateExec with aggregates"}); }
  { Builder b; u32 e = ext(b); u32 x = b.extend((int)e, {enc(2)}); b.sort((int)x, {{3, VALUE, true}, {4, VALUE, false}});
    expect("two value keys: a record of 9 words", b, F, UNSUP, {"node 3", "9 64-bit words", "at most 8", "64 KB of LDS"}); }
  { Builder b; b.sort((int)b.table(0, 3), {{0, ID, false}}, 0, {0, 3}); expect("projecting a column past the input", b, 0, INVALID, {"SortExec", "out of range"}); }
  // ---- the value column of a SORT is refused where ids are compared, like any other
  { Builder b; u32 e = ext(b); u32 s = b.sort((int)e, {{3, VALUE, true}}); auto n = Builder::blank(RDFGPU_NODE_HASH_JOIN, (int)s, (int)b.table(1, 2)); n.n_keys = 1; n.left_keys[0] = 3; b.push(n);
    expect("a sorted value column as join key", b, F, UNSUP, {"left join key column 3", "computed value column"}); }
  return finish();
}
