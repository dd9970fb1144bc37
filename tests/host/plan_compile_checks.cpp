// plan_compile_checks.cpp — the host-side checks of plan compilation (plan_compile.cpp: compile_nodes and what it calls, check_program
// included) as a stand-alone program, so that they can run under AddressSanitizer / UndefinedBehaviorSanitizer without a device:
//
//   make -C rdf-fusion_amd/csrc host-checks SANITIZE=1        (without SANITIZE: a plain build, what tests/test_agg_columns_cpu.py runs)
//
// The unit under test is included as text (its checks live in an anonymous namespace); what it needs of the store and the device is stubbed
// out below — the plans here have bound tables as leaves, so nothing of the store is touched.  Every case is a plan description with
// RDFGPU_PLAN_AGG_COLUMNS (or without it) and the status its compilation must end in; a refusal's text must name the node.
#include "../../rdf-fusion_amd/csrc/plan_compile.cpp"

#include <cstdio>
#include <functional>

namespace rdfgpu {
// (what plan_compile() itself needs beyond compile_nodes: never called here)
Plan::~Plan() {}
void Plan::derive_source(SourceInfo&, const ScanInstructions&) { fail(RDFGPU_ERR_INVALID, "no store in this program"); }
void Plan::upload_pool() {}
ScanInstructions make_gspo(const rdfgpu_scan_instruction*, const u32*, u32) { fail(RDFGPU_ERR_INVALID, "no store in this program"); }
void Store::activate() const {}
ExecContext* Store::acquire_context(u32) { return nullptr; }
}  // namespace rdfgpu

using namespace rdfgpu;

namespace {
struct Builder {
  std::vector<rdfgpu_plan_node> nodes; std::vector<rdfgpu_expr_node> exprs; std::vector<u32> pool;
  u32 push(rdfgpu_plan_node n) { nodes.push_back(n); return (u32)nodes.size() - 1; }
  static rdfgpu_plan_node blank(u32 kind, int left, int right = -1) {
    rdfgpu_plan_node n{}; n.kind = kind; n.left = left; n.right = right; n.n_proj = RDFGPU_NO_PROJECTION; return n;
  }
  u32 table(u32 slot, u32 cols) { auto n = blank(RDFGPU_NODE_TABLE, -1); n.table_slot = slot; n.table_cols = cols; return push(n); }
  void project(rdfgpu_plan_node& n, std::vector<u32> p) { n.proj_off = (u32)pool.size(); n.n_proj = (u32)p.size(); pool.insert(pool.end(), p.begin(), p.end()); }
  void program(rdfgpu_plan_node& n, std::vector<rdfgpu_expr_node> e) { n.expr_off = (u32)exprs.size(); n.expr_len = (u32)e.size(); exprs.insert(exprs.end(), e.begin(), e.end()); }
  u32 aggregate(int in, std::vector<u32> keys, std::vector<std::pair<u32, u32>> aggs) {
    auto n = blank(RDFGPU_NODE_AGGREGATE, in);
    n.n_keys = (u32)keys.size();
    for (size_t k = 0; k < keys.size() && k < RDFGPU_MAX_KEYS; k++) n.left_keys[k] = keys[k];
    n.table_cols = (u32)aggs.size(); n.table_slot = (u32)pool.size();
    for (auto& a : aggs) { pool.push_back(a.first); pool.push_back(a.second); }
    return push(n);
  }
  u32 filter(int in, std::vector<rdfgpu_expr_node> e, std::vector<u32> proj = {}) {
    auto n = blank(RDFGPU_NODE_FILTER, in); program(n, e); if (!proj.empty()) project(n, proj); return push(n);
  }
  u32 join(u32 kind, int l, int r, std::vector<std::pair<u32, u32>> on, u32 type = RDFGPU_JOIN_INNER, std::vector<rdfgpu_expr_node> e = {}, std::vector<u32> proj = {}) {
    auto n = blank(kind, l, r); n.join_type = type; n.n_keys = (u32)on.size();
    for (size_t k = 0; k < on.size(); k++) { n.left_keys[k] = on[k].first; n.right_keys[k] = on[k].second; }
    if (!e.empty()) program(n, e);
    if (!proj.empty()) project(n, proj);
    return push(n);
  }
};
rdfgpu_expr_node op(u8 o, u32 u = 0, u8 tag = 0, int64_t lo = 0) { rdfgpu_expr_node e{}; e.op = o; e.u = u; e.tag = tag; e.lo = lo; return e; }
rdfgpu_expr_node column(u32 c) { return op(RDFGPU_EX_COLUMN, c); }
std::vector<rdfgpu_expr_node> value_gt(u32 c, int64_t k) {   // EBV(GT(ENC_TV(col c), integer k))
  return {column(c), op(RDFGPU_EX_ENC_TV), op(RDFGPU_EX_LIT_TV, 0, RDFGPU_TV_INTEGER, k), op(RDFGPU_EX_GT), op(RDFGPU_EX_EBV)};
}

int failures = 0;
// Compiles the nodes of `b` (root = the last node); `want` = the status, `needle` = what a refusal's text must hold.  -> the compiled plan's nodes
std::vector<NodeInfo> expect(const char* name, Builder& b, u32 flags, int want, const char* needle = "") {
  rdfgpu_plan_desc d{};
  d.nodes = b.nodes.data(); d.n_nodes = (u32)b.nodes.size(); d.root = d.n_nodes - 1;
  d.exprs = b.exprs.data(); d.n_exprs = (u32)b.exprs.size(); d.pool = b.pool.data(); d.n_pool = (u32)b.pool.size(); d.flags = flags;
  Plan plan;
  plan.root = d.root; plan.agg_columns = (flags & RDFGPU_PLAN_AGG_COLUMNS) != 0;
  plan.nodes.resize(d.n_nodes);
  int got = RDFGPU_OK; std::string text;
  try { compile_nodes(&plan, &d); reorder_cross_joins(&plan); count_consumers(&plan); account_columns_read(&plan); }
  catch (const Error& e) { got = e.status; text = e.what(); }
  const bool ok = got == want && (want == RDFGPU_OK || text.find(needle) != std::string::npos);
  std::printf("%-44s %s  %s\n", name, ok ? "ok  " : "FAIL", text.c_str());
  if (!ok) failures++;
  return plan.nodes;
}
constexpr u32 F = RDFGPU_PLAN_AGG_COLUMNS;
constexpr int UNSUP = RDFGPU_ERR_UNSUPPORTED, INVALID = RDFGPU_ERR_INVALID;
// table(0: k, x, y) -> AggregateExec gby=[k] aggr=[COUNT(*), SUM(x)]: columns k, COUNT(*), SUM(x); node 1
u32 agg(Builder& b) { return b.aggregate((int)b.table(0, 3), {0}, {{RDFGPU_AGG_COUNT_STAR, 0}, {RDFGPU_AGG_SUM, 1}}); }
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
    std::printf("%-44s %s\n", "  .. rewritten to a value load, VM shape", ok ? "ok  " : "FAIL"); failures += !ok;
  }
  { Builder b; u32 a = agg(b); b.filter((int)a, value_gt(0, 3));   // the key column: an ordinary ENC_TV, the specialised shape
    auto nodes = expect("filter on the key column of an aggregate", b, F, RDFGPU_OK);
    bool ok = nodes.back().prog.nodes[1].op == RDFGPU_EX_ENC_TV && nodes.back().shape == 2;
    std::printf("%-44s %s\n", "  .. keeps ENC_TV and its shape", ok ? "ok  " : "FAIL"); failures += !ok; }
  { Builder b; u32 a = agg(b); u32 t = b.table(1, 2);
    b.join(RDFGPU_NODE_HASH_JOIN, (int)t, (int)a, {{0, 0}}, RDFGPU_JOIN_LEFT, {column(1), op(RDFGPU_EX_ENC_TV), column(4), op(RDFGPU_EX_ENC_TV), op(RDFGPU_EX_GT), op(RDFGPU_EX_EBV)}, {0, 4, 3});
    auto nodes = expect("LEFT join, filter over both sides", b, F, RDFGPU_OK);
    const NodeInfo& nd = nodes.back();
    bool ok = nd.prog.nodes[1].op == RDFGPU_EX_ENC_TV && nd.prog.nodes[3].op == kExAggValue && nd.shape == 1 && nd.origin[1].agg == 1 && nd.origin[2].agg == 0 && nd.origin[0].node < 0;
    std::printf("%-44s %s\n", "  .. origins through the projection", ok ? "ok  " : "FAIL"); failures += !ok; }
  { Builder b; u32 a = agg(b); u32 t = b.table(1, 2); b.join(RDFGPU_NODE_HASH_JOIN, (int)t, (int)a, {{0, 0}}, RDFGPU_JOIN_LEFT_SEMI, value_gt(4, 1));
    auto nodes = expect("semi join reads the right side's value", b, F, RDFGPU_OK);
    bool ok = nodes.back().width == 2 && nodes.back().origin[0].node < 0 && nodes.back().origin[1].node < 0;
    std::printf("%-44s %s\n", "  .. hands on its left side only", ok ? "ok  " : "FAIL"); failures += !ok; }
  { Builder b; u32 a = agg(b); b.aggregate((int)a, {0}, {{RDFGPU_AGG_SUM, 1}, {RDFGPU_AGG_COUNT, 2}, {RDFGPU_AGG_AVG, 2}});
    auto nodes = expect("aggregate over an aggregate", b, F, RDFGPU_OK);
    const NodeInfo& nd = nodes.back();
    bool ok = nd.agg_prog[0] == 0 && nd.agg_prog[1] < 0 && nd.agg_prog[2] == 1 && nd.agg_progs[0].n == 2 && nd.agg_progs[0].nodes[1].op == kExAggValue &&
              nd.agg_progs[1].nodes[1].u == ((a << 8) | 1u) && nd.width == 4 && nd.origin[3].node == (int)nodes.size() - 1;
    std::printf("%-44s %s\n", "  .. SUM / AVG as [COLUMN, value load]", ok ? "ok  " : "FAIL"); failures += !ok; }
  { Builder b; u32 a = agg(b); u32 g = b.aggregate((int)b.table(1, 2), {}, {{RDFGPU_AGG_AVG, 1}}); u32 x = b.join(RDFGPU_NODE_CROSS_JOIN, (int)a, (int)g, {});
    b.filter((int)x, {column(2), op(RDFGPU_EX_ENC_TV), column(3), op(RDFGPU_EX_ENC_TV), op(RDFGPU_EX_LIT_TV, 0, RDFGPU_TV_INTEGER, 2), op(RDFGPU_EX_MUL), op(RDFGPU_EX_GT), op(RDFGPU_EX_EBV)});
    expect("cross join with a zero-key aggregate", b, F, RDFGPU_OK); }
  { Builder b; u32 a = agg(b); b.filter((int)a, {column(2), op(RDFGPU_EX_BOUND)});
    expect("BOUND of a value column", b, F, RDFGPU_OK); }
  // ---- opt-in: the same descriptions without the flag
  { Builder b; u32 a = agg(b); b.filter((int)a, value_gt(1, 3)); expect("no flag: filter over an aggregate", b, 0, UNSUP, "must be the plan's root"); }
  { Builder b; u32 a = agg(b); b.aggregate((int)a, {0}, {{RDFGPU_AGG_SUM, 1}}); expect("no flag: aggregate over an aggregate", b, 0, UNSUP, "must be the plan's root"); }
  { Builder b; agg(b); auto nodes = expect("no flag: the root form", b, 0, RDFGPU_OK); failures += nodes.back().width != 1; }
  // ---- refusals under the flag: RDFGPU_ERR_UNSUPPORTED, the text names node and column
  { Builder b; u32 a = agg(b); u32 t = b.table(1, 2); b.join(RDFGPU_NODE_HASH_JOIN, (int)a, (int)t, {{2, 0}}); expect("left join key", b, F, UNSUP, "node 3: left join key column 2"); }
  { Builder b; u32 a = agg(b); u32 t = b.table(1, 2); b.join(RDFGPU_NODE_HASH_JOIN, (int)t, (int)a, {{0, 0}, {1, 1}}, RDFGPU_JOIN_LEFT_ANTI); expect("right join key of an anti join", b, F, UNSUP, "node 3: right join key column 1"); }
  { Builder b; u32 a = agg(b); b.aggregate((int)a, {0, 1}, {}); expect("group column", b, F, UNSUP, "node 2: group column 1"); }
  { Builder b; u32 a = agg(b); b.aggregate((int)a, {0}, {{RDFGPU_AGG_COUNT_DISTINCT, 2}}); expect("COUNT DISTINCT input", b, F, UNSUP, "node 2: COUNT DISTINCT input column 2"); }
  { Builder b; u32 a = agg(b); auto n = Builder::blank(RDFGPU_NODE_TOPK, (int)a); n.n_keys = 2; n.left_keys[0] = 0; n.left_keys[1] = 2; n.right_keys[1] = RDFGPU_SORT_BY_DOUBLE; n.table_cols = 5; b.project(n, {0}); b.push(n);
    expect("TopK sort key", b, F, UNSUP, "node 2: TopK sort key column 2"); }
  { Builder b; u32 a = agg(b); auto n = Builder::blank(RDFGPU_NODE_TOPK, (int)a); n.n_keys = 1; n.left_keys[0] = 0; n.table_cols = 5; b.project(n, {0, 1}); b.push(n);
    expect("TopK output", b, F, UNSUP, "node 2: TopK output column 1"); }
  { Builder b; u32 a = agg(b); auto n = Builder::blank(RDFGPU_NODE_TOPK, (int)a); n.n_keys = 1; n.left_keys[0] = 0; n.table_cols = 5; n.table_slot = 2; b.project(n, {0}); b.push(n);
    expect("TopK group", b, F, UNSUP, "node 2: TopK group column 1"); }
  { Builder b; u32 a = agg(b); b.push(Builder::blank(RDFGPU_NODE_CLOSURE, (int)a)); expect("CLOSURE input", b, F, UNSUP, "node 2: KleenePlusClosureExec input column 1"); }
  { Builder b; u32 a = agg(b); u32 t = b.table(1, 3); b.push(Builder::blank(RDFGPU_NODE_UNION, (int)t, (int)a)); expect("UNION input", b, F, UNSUP, "node 3: UnionExec right input column 1"); }
  { Builder b; u32 a = agg(b); auto p = Builder::blank(RDFGPU_NODE_PROJECTION, (int)a); b.project(p, {2, 2, 0}); u32 pr = b.push(p); u32 t = b.table(1, 2);
    b.join(RDFGPU_NODE_HASH_JOIN, (int)pr, (int)t, {{1, 0}}); expect("a key behind a projection", b, F, UNSUP, "node 4: left join key column 1"); }
  // ---- kind errors: RDFGPU_ERR_INVALID
  { Builder b; u32 a = agg(b); b.filter((int)a, {column(1), op(RDFGPU_EX_LIT_ID, 3), op(RDFGPU_EX_ID_EQ)}); expect("ID_EQ of a value column", b, F, INVALID, "aggregate value column"); }
  { Builder b; u32 a = agg(b); b.filter((int)a, {column(0), column(2), op(RDFGPU_EX_ID_NEQ)}); expect("ID_NEQ of a value column", b, F, INVALID, "aggregate value column"); }
  { Builder b; u32 a = agg(b); b.filter((int)a, {column(2), column(0), op(RDFGPU_EX_IS_COMPATIBLE)}); expect("IS_COMPATIBLE of a value column", b, F, INVALID, "aggregate value column"); }
  { Builder b; u32 a = agg(b); b.filter((int)a, {column(1), op(RDFGPU_EX_STR), op(RDFGPU_EX_STRLEN), op(RDFGPU_EX_EBV)}); expect("STR of a value column", b, F, INVALID, "aggregate value column"); }
  { Builder b; u32 a = agg(b); b.filter((int)a, {column(1), op(kExAggValue), op(RDFGPU_EX_EBV)}); expect("the internal op in a description", b, F, INVALID, "unknown op"); }
  { Builder b; u32 a = agg(b); b.filter((int)a, {column(3), op(RDFGPU_EX_BOUND)}); expect("a column past the value columns", b, F, INVALID, "out of range"); }
  { Builder b; u32 a = agg(b); b.aggregate((int)a, {0}, {{RDFGPU_AGG_SUM, 3}}); expect("an aggregate input past the value columns", b, F, INVALID, "reads column 3 of 3"); }
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
