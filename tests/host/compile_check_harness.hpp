// compile_check_harness.hpp — what the *_compile_checks.cpp programs share.  Each of them checks a part of plan compilation
// (plan_compile.cpp: compile_nodes and what it calls, check_program included) as a stand-alone program, so that the checks can run under
// AddressSanitizer / UndefinedBehaviorSanitizer without a device:
//
//   make -C rdf-fusion_amd/csrc host-checks[-extend|-sort|-minmax|-lex-compile|-value-keys|-forms] [SANITIZE=1]
//
// The unit under test is included as text (its checks live in an anonymous namespace); what it needs of the store and the device is stubbed
// out below — the plans have bound tables as leaves, so nothing of the store is touched.  A case is a plan description (a Builder) with
// its flags and the status its compilation must end in; a refusal's text must hold the key words given.
#pragma once
#include "../../rdf-fusion_amd/csrc/plan_compile.cpp"

#include <cstdio>

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
// ---- programs
typedef std::vector<rdfgpu_expr_node> Prog;
rdfgpu_expr_node op(u8 o, u32 u = 0, u8 tag = 0, int64_t lo = 0) { rdfgpu_expr_node e{}; e.op = o; e.u = u; e.tag = tag; e.lo = lo; return e; }
rdfgpu_expr_node column(u32 c) { return op(RDFGPU_EX_COLUMN, c); }
rdfgpu_expr_node lit(u8 tag, int64_t lo, int64_t hi = 0) { rdfgpu_expr_node e = op(RDFGPU_EX_LIT_TV, 0, tag, lo); e.hi = hi; return e; }
Prog enc(u32 c) { return {column(c), op(RDFGPU_EX_ENC_TV)}; }   // ENC_TV(col c)
Prog cat(std::initializer_list<Prog> parts, std::initializer_list<rdfgpu_expr_node> tail = {}) {   // the parts, then the nodes of `tail`
  Prog p;
  for (const Prog& q : parts) p.insert(p.end(), q.begin(), q.end());
  p.insert(p.end(), tail.begin(), tail.end());
  return p;
}

// ---- plan descriptions: every method appends a node and returns its index
struct SortKey { u32 col, how; bool desc; };
typedef std::vector<std::pair<u32, u32>> Pairs;
struct Builder {
  std::vector<rdfgpu_plan_node> nodes; std::vector<rdfgpu_expr_node> exprs; std::vector<u32> pool;
  u32 push(rdfgpu_plan_node n) { nodes.push_back(n); return (u32)nodes.size() - 1; }
  static rdfgpu_plan_node blank(u32 kind, int left, int right = -1) {
    rdfgpu_plan_node n{}; n.kind = kind; n.left = left; n.right = right; n.n_proj = RDFGPU_NO_PROJECTION; return n;
  }
  void project(rdfgpu_plan_node& n, std::vector<u32> p) { n.proj_off = (u32)pool.size(); n.n_proj = (u32)p.size(); pool.insert(pool.end(), p.begin(), p.end()); }
  std::pair<u32, u32> program(const Prog& p) { const u32 off = (u32)exprs.size(); exprs.insert(exprs.end(), p.begin(), p.end()); return {off, (u32)p.size()}; }
  void predicate(rdfgpu_plan_node& n, const Prog& p) { auto at = program(p); n.expr_off = at.first; n.expr_len = at.second; }
  u32 table(u32 slot, u32 cols) { auto n = blank(RDFGPU_NODE_TABLE, -1); n.table_slot = slot; n.table_cols = cols; return push(n); }
  u32 filter(int in, const Prog& p, std::vector<u32> proj = {}) {
    auto n = blank(RDFGPU_NODE_FILTER, in); predicate(n, p); if (!proj.empty()) project(n, proj); return push(n);
  }
  u32 join(u32 kind, int l, int r, u32 type, Pairs on, const Prog& flt = {}, std::vector<u32> proj = {}) {
    auto n = blank(kind, l, r); n.join_type = type; n.n_keys = (u32)on.size();
    for (size_t k = 0; k < on.size() && k < RDFGPU_MAX_KEYS; k++) { n.left_keys[k] = on[k].first; n.right_keys[k] = on[k].second; }
    if (!flt.empty()) predicate(n, flt);
    if (!proj.empty()) project(n, proj);
    return push(n);
  }
  // AggregateExec: group columns (0..3 in left_keys[], 4..7 in right_keys[]), then (function, input) per aggregate; input_expr gives the
  // input word of a program
  u32 aggregate(int in, std::vector<u32> keys, Pairs aggs) {
    auto n = blank(RDFGPU_NODE_AGGREGATE, in);
    n.n_keys = (u32)keys.size();
    for (size_t k = 0; k < keys.size() && k < RDFGPU_MAX_GROUP_KEYS; k++) (k < RDFGPU_MAX_KEYS ? n.left_keys[k] : n.right_keys[k - RDFGPU_MAX_KEYS]) = keys[k];
    n.table_cols = (u32)aggs.size(); n.table_slot = (u32)pool.size();
    for (auto& a : aggs) { pool.push_back(a.first); pool.push_back(a.second); }
    return push(n);
  }
  u32 input_expr(const Prog& p) { auto at = program(p); pool.push_back(at.first); pool.push_back(at.second); return RDFGPU_AGG_INPUT_EXPR | ((u32)pool.size() - 2); }
  // EXTEND: `keep` (empty: all columns), then one computed column per program
  u32 extend(int in, std::vector<Prog> progs, std::vector<u32> keep = {}) {
    auto n = blank(RDFGPU_NODE_EXTEND, in);
    if (!keep.empty()) project(n, keep);
    Pairs at;
    for (const Prog& p : progs) at.push_back(program(p));
    n.table_cols = (u32)progs.size(); n.table_slot = (u32)pool.size();
    for (auto& p : at) { pool.push_back(p.first); pool.push_back(p.second); }
    return push(n);
  }
  u32 sort(int in, std::vector<SortKey> keys, u32 fetch = 0, std::vector<u32> proj = {}) {
    auto n = blank(RDFGPU_NODE_SORT, in);
    n.n_keys = (u32)keys.size(); n.table_cols = fetch;
    for (size_t k = 0; k < keys.size() && k < RDFGPU_MAX_KEYS; k++) { n.left_keys[k] = keys[k].col; n.right_keys[k] = keys[k].how | (keys[k].desc ? RDFGPU_SORT_DESC : 0u); }
    if (!proj.empty()) project(n, proj);
    return push(n);
  }
};

// ---- cases
int failures = 0;
constexpr u32 F = RDFGPU_PLAN_AGG_COLUMNS;
constexpr int UNSUP = RDFGPU_ERR_UNSUPPORTED, INVALID = RDFGPU_ERR_INVALID;
void report(const char* name, bool ok, const char* text = nullptr) {
  if (text) std::printf("%-84s %s  %s\n", name, ok ? "ok  " : "FAIL", text); else std::printf("%-84s %s\n", name, ok ? "ok  " : "FAIL");
  failures += !ok;
}
void check(const char* name, bool ok) { report(name, ok); }
// Compiles the nodes of `b` (root = the last node) as plan_compile does for these flags; `want` = the status, `needles` = what a refusal's
// text must hold.  -> the compiled plan's nodes
std::vector<NodeInfo> expect(const char* name, Builder& b, u32 flags, int want, std::vector<const char*> needles = {}) {
  rdfgpu_plan_desc d{};
  d.nodes = b.nodes.data(); d.n_nodes = (u32)b.nodes.size(); d.root = d.n_nodes - 1;
  d.exprs = b.exprs.data(); d.n_exprs = (u32)b.exprs.size(); d.pool = b.pool.data(); d.n_pool = (u32)b.pool.size(); d.flags = flags;
  Plan plan;
  plan.root = d.root;
  plan.nodes.resize(d.n_nodes);
  int got = RDFGPU_OK; std::string text;
  try {
    check_plan_flags(flags);
    plan.agg_columns = (flags & RDFGPU_PLAN_AGG_COLUMNS) != 0; plan.value_keys = (flags & RDFGPU_PLAN_VALUE_KEYS) != 0;
    compile_nodes(&plan, &d); reorder_cross_joins(&plan); count_consumers(&plan); account_columns_read(&plan);
  } catch (const Error& e) { got = e.status; text = e.what(); }
  bool ok = got == want;
  for (const char* n : needles) ok = ok && text.find(n) != std::string::npos;
  report(name, ok, text.c_str());
  return plan.nodes;
}
// check_program alone: the status and the kind left
void expect_program(const char* name, const Prog& p, u32 n_cols, int want, u32 kind, std::vector<const char*> needles = {}, u32 value_cols = 0) {
  int got = RDFGPU_OK; std::string text; u32 k = 99;
  try { k = check_program(p.data(), (u32)p.size(), n_cols, 0, value_cols); } catch (const Error& e) { got = e.status; text = e.what(); }
  bool ok = got == want && (want != RDFGPU_OK || k == kind);
  for (const char* n : needles) ok = ok && text.find(n) != std::string::npos;
  report(name, ok, text.c_str());
}
int finish() { std::printf("%d failure(s)\n", failures); return failures ? 1 : 0; }
}  // namespace
