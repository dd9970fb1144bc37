// minmax_compile_checks.cpp — the host-side checks of MIN / MAX (RDFGPU_AGG_MIN / _MAX; plan_compile.cpp: compile_aggregate) as a
// stand-alone program, so that they can run under AddressSanitizer / UndefinedBehaviorSanitizer without a device:
//
//   make -C rdf-fusion_amd/csrc host-checks-minmax SANITIZE=1     (without SANITIZE: a plain build, what tests/test_minmax_cpu.py runs)
//
// Built like sort_compile_checks.cpp: the unit under test is included as text, what it needs of the store and the device is stubbed
// out, the plans have bound tables as leaves.  Every case is a plan description and the status its compilation must end in; a refusal's
// text must hold the key words given.
#include "../../rdf-fusion_amd/csrc/plan_compile.cpp"

#include <cstdio>

namespace rdfgpu {
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
  u32 aggregate(int in, std::vector<u32> keys, std::vector<std::pair<u32, u32>> aggs) {
    auto n = blank(RDFGPU_NODE_AGGREGATE, in);
    n.n_keys = (u32)keys.size();
    for (size_t k = 0; k < keys.size() && k < RDFGPU_MAX_KEYS; k++) n.left_keys[k] = keys[k];
    n.table_cols = (u32)aggs.size(); n.table_slot = (u32)pool.size();
    for (auto& a : aggs) { pool.push_back(a.first); pool.push_back(a.second); }
    return push(n);
  }
  // an aggregate's input expression `op`(ENC_TV(col a), ENC_TV(col b)) (op = 0: ENC_TV(col a) alone) -> its RDFGPU_AGG_INPUT_EXPR word
  u32 input_expr(u32 a, u32 b, u8 op) {
    const u32 off = (u32)exprs.size();
    rdfgpu_expr_node c{}, e{}; e.op = RDFGPU_EX_ENC_TV;
    c.op = RDFGPU_EX_COLUMN; c.u = a; exprs.push_back(c); exprs.push_back(e);
    if (op) { c.u = b; exprs.push_back(c); exprs.push_back(e); rdfgpu_expr_node o{}; o.op = op; exprs.push_back(o); }
    const u32 at = (u32)pool.size();
    pool.push_back(off); pool.push_back((u32)exprs.size() - off);
    return RDFGPU_AGG_INPUT_EXPR | at;
  }
  u32 hash_join(int l, int r, u32 lk, u32 rk) { auto n = blank(RDFGPU_NODE_HASH_JOIN, l, r); n.n_keys = 1; n.left_keys[0] = lk; n.right_keys[0] = rk; return push(n); }
};

int failures = 0;
void check(const char* name, bool ok) { std::printf("%-60s %s\n", name, ok ? "ok  " : "FAIL"); failures += !ok; }
// Compiles the nodes of `b` (root = the last node); `want` = the status, `needles` = what a refusal's text must hold.  -> the compiled nodes
std::vector<NodeInfo> expect(const char* name, Builder& b, u32 flags, int want, std::vector<const char*> needles = {}) {
  rdfgpu_plan_desc d{};
  d.nodes = b.nodes.data(); d.n_nodes = (u32)b.nodes.size(); d.root = d.n_nodes - 1;
  d.exprs = b.exprs.data(); d.n_exprs = (u32)b.exprs.size(); d.pool = b.pool.data(); d.n_pool = (u32)b.pool.size(); d.flags = flags;
  Plan plan;
  plan.root = d.root; plan.agg_columns = (flags & RDFGPU_PLAN_AGG_COLUMNS) != 0;
  plan.nodes.resize(d.n_nodes);
  int got = RDFGPU_OK; std::string text;
  try { compile_nodes(&plan, &d); reorder_cross_joins(&plan); count_consumers(&plan); account_columns_read(&plan); }
  catch (const Error& e) { got = e.status; text = e.what(); }
  bool ok = got == want;
  for (const char* n : needles) ok = ok && text.find(n) != std::string::npos;
  std::printf("%-60s %s  %s\n", name, ok ? "ok  " : "FAIL", text.c_str());
  if (!ok) failures++;
  return plan.nodes;
}
constexpr u32 F = RDFGPU_PLAN_AGG_COLUMNS;
constexpr int UNSUP = RDFGPU_ERR_UNSUPPORTED, INVALID = RDFGPU_ERR_INVALID;
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
  { Builder b; u32 t = b.table(0, 3); u32 e = b.input_expr(1, 2, RDFGPU_EX_MUL); u32 a = b.aggregate((int)t, {0}, {{MIN, e}, {RDFGPU_AGG_AVG, 1}});
    auto nodes = expect("the Q6 node: MIN over an expression beside an AVG", b, F, RDFGPU_OK);
    check("  .. the program is loaded", nodes[a].agg_prog[0] == 0 && nodes[a].agg_prog[1] < 0 && nodes[a].agg_progs[0].n == 5 && nodes[a].width == 3); }
  { Builder b; u32 a = b.aggregate((int)b.table(0, 2), {0}, {{MAX, 1}}); u32 t = b.table(1, 2); b.hash_join((int)a, (int)t, 0, 0);
    auto nodes = expect("MAX at node 1 of 3, under a join", b, F, RDFGPU_OK);
    check("  .. the join carries the value column", nodes.back().width == 4 && nodes.back().origin[1].node == (int)a); }
  { Builder b; b.aggregate((int)b.table(0, 2), {}, {{MIN, 1}}); expect("zero keys", b, F, RDFGPU_OK); }
  // ---- without the flag: the status and the text every plan has always met
  { Builder b; b.aggregate((int)b.table(0, 2), {0}, {{MIN, 1}}); expect("MIN without the flag", b, 0, UNSUP, {"node 1", OLD_TEXT}); }
  { Builder b; b.aggregate((int)b.table(0, 2), {0}, {{MAX, 1}}); expect("MAX without the flag", b, 0, UNSUP, {"node 1", OLD_TEXT}); }
  { Builder b; b.aggregate((int)b.table(0, 2), {0}, {{RDFGPU_AGG_SAMPLE, 1}}); expect("SAMPLE without the flag", b, 0, UNSUP, {"node 1", OLD_TEXT}); }
  { Builder b; u32 t = b.table(0, 3); u32 e = b.input_expr(1, 2, RDFGPU_EX_ADD); b.aggregate((int)t, {0}, {{MIN, e}}); expect("MIN over an expression without the flag", b, 0, UNSUP, {"node 1", OLD_TEXT}); }
  // ---- with the flag: what stays refused
  { Builder b; b.aggregate((int)b.table(0, 2), {0}, {{RDFGPU_AGG_SAMPLE, 1}}); expect("SAMPLE with the flag", b, F, UNSUP, {"node 1: aggregate 0", "SAMPLE / GROUP_CONCAT are not on the device"}); }
  { Builder b; b.aggregate((int)b.table(0, 2), {0}, {{MAX, 1}, {RDFGPU_AGG_GROUP_CONCAT, 1}}); expect("GROUP_CONCAT with the flag", b, F, UNSUP, {"node 1: aggregate 1", "SAMPLE / GROUP_CONCAT are not on the device"}); }
  { Builder b; b.aggregate((int)b.table(0, 2), {0}, {{RDFGPU_AGG_SUM_DISTINCT, 1}}); expect("SUM DISTINCT with the flag", b, F, UNSUP, {"SUM / AVG with DISTINCT"}); }
  { Builder b; u32 t = b.table(0, 3); u32 e = b.input_expr(1, 2, RDFGPU_EX_CONTAINS); b.aggregate((int)t, {0}, {{MAX, e}});
    expect("a pattern op in the input", b, F, UNSUP, {"node 1: aggregate 0", "REGEX / CONTAINS"}); }
  { Builder b; u32 t = b.table(0, 3); u32 e = b.input_expr(1, 2, 0); b.pool.back() = 1; b.aggregate((int)t, {0}, {{MIN, e}});   // the program is [COLUMN] alone
    expect("an input that leaves an id", b, F, INVALID, {"node 1: aggregate 0", "does not yield a typed value"}); }
  { Builder b; b.aggregate((int)b.table(0, 2), {0}, {{MIN, 2}}); expect("an input column past the table", b, F, INVALID, {"node 1: aggregate 0 reads column 2 of 2"}); }
  // ---- a MIN / MAX value column is refused where ids are compared, like any other
  { Builder b; u32 a = b.aggregate((int)b.table(0, 2), {0}, {{MAX, 1}}); u32 t = b.table(1, 2); b.hash_join((int)a, (int)t, 1, 0);
    expect("a MAX value column as join key", b, F, UNSUP, {"node 3", "left join key column 1", "aggregate value column", "aggregate 0 of node 1"}); }
  { Builder b; u32 a = b.aggregate((int)b.table(0, 2), {0}, {{MIN, 1}}); b.aggregate((int)a, {1}, {});
    expect("a MIN value column as group column", b, F, UNSUP, {"node 2", "group column 1", "aggregate value column"}); }
  { Builder b; u32 a = b.aggregate((int)b.table(0, 2), {0}, {{MIN, 1}}); b.aggregate((int)a, {0}, {{RDFGPU_AGG_COUNT_DISTINCT, 1}});
    expect("a MIN value column under COUNT DISTINCT", b, F, UNSUP, {"node 2", "COUNT DISTINCT input column 1"}); }
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
