// lex_compile_checks.cpp — the host-side checks of the lexical casts (RDFGPU_EX_CAST_STRING / RDFGPU_EX_CAST_LEX; plan_compile.cpp:
// check_program and what routes a program) as a stand-alone program, so that they can run under AddressSanitizer /
// UndefinedBehaviorSanitizer without a device:
//
//   make -C rdf-fusion_amd/csrc host-checks-lex-compile SANITIZE=1     (without SANITIZE: a plain build, what tests/test_lex_cast_cpu.py runs)
//
// Built like sort_compile_checks.cpp: the unit under test is included as text, what it needs of the store and the device is stubbed out,
// the plans have bound tables as leaves.
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
typedef std::vector<rdfgpu_expr_node> Prog;
rdfgpu_expr_node op(u8 o, u32 u = 0) { rdfgpu_expr_node e{}; e.op = o; e.u = u; return e; }
rdfgpu_expr_node column(u32 c) { return op(RDFGPU_EX_COLUMN, c); }
rdfgpu_expr_node lit(u8 tag, int64_t lo, int64_t hi = 0) { rdfgpu_expr_node e{}; e.op = RDFGPU_EX_LIT_TV; e.tag = tag; e.lo = lo; e.hi = hi; return e; }
constexpr u8 STRING = RDFGPU_EX_CAST_STRING, LEX = RDFGPU_EX_CAST_LEX, ENC = RDFGPU_EX_ENC_TV, EBV_ = RDFGPU_EX_EBV, LT = RDFGPU_EX_LT;
constexpr u32 FLOAT = RDFGPU_TV_FLOAT;
// xsd:float(xsd:string(ENC_TV(c)))
Prog price(u32 c) { return {column(c), op(STRING), op(LEX, FLOAT)}; }
Prog cat(Prog a, const Prog& b) { a.insert(a.end(), b.begin(), b.end()); return a; }

int failures = 0;
void check(const char* name, bool ok) { std::printf("%-64s %s\n", name, ok ? "ok  " : "FAIL"); failures += !ok; }
// check_program alone: the status and the kind left
void program(const char* name, const Prog& p, u32 n_cols, int want, u32 kind, std::vector<const char*> needles = {}, u32 value_cols = 0) {
  int got = RDFGPU_OK; std::string text; u32 k = 99;
  try { k = check_program(p.data(), (u32)p.size(), n_cols, 0, value_cols); } catch (const Error& e) { got = e.status; text = e.what(); }
  bool ok = got == want && (want != RDFGPU_OK || k == kind);
  for (const char* n : needles) ok = ok && text.find(n) != std::string::npos;
  std::printf("%-64s %s  %s\n", name, ok ? "ok  " : "FAIL", text.c_str());
  failures += !ok;
}
struct Builder {
  std::vector<rdfgpu_plan_node> nodes; std::vector<rdfgpu_expr_node> exprs; std::vector<u32> pool;
  u32 push(rdfgpu_plan_node n) { nodes.push_back(n); return (u32)nodes.size() - 1; }
  static rdfgpu_plan_node blank(u32 kind, int left, int right = -1) { rdfgpu_plan_node n{}; n.kind = kind; n.left = left; n.right = right; n.n_proj = RDFGPU_NO_PROJECTION; return n; }
  u32 table(u32 slot, u32 cols) { auto n = blank(RDFGPU_NODE_TABLE, -1); n.table_slot = slot; n.table_cols = cols; return push(n); }
  void expr(rdfgpu_plan_node& n, const Prog& p) { n.expr_off = (u32)exprs.size(); n.expr_len = (u32)p.size(); exprs.insert(exprs.end(), p.begin(), p.end()); }
  u32 filter(int in, const Prog& p) { auto n = blank(RDFGPU_NODE_FILTER, in); expr(n, p); return push(n); }
  u32 join(u32 kind, u32 type, int l, int r, const Prog& p) { auto n = blank(kind, l, r); n.join_type = type; if (kind == RDFGPU_NODE_HASH_JOIN) n.n_keys = 1; expr(n, p); return push(n); }
  u32 aggregate(int in, u32 fn, const Prog& p) {
    auto n = blank(RDFGPU_NODE_AGGREGATE, in); n.n_keys = 1; n.table_cols = 1; n.table_slot = (u32)pool.size();
    pool.push_back(fn); pool.push_back(RDFGPU_AGG_INPUT_EXPR | ((u32)pool.size() + 1)); pool.push_back((u32)exprs.size()); pool.push_back((u32)p.size());
    exprs.insert(exprs.end(), p.begin(), p.end()); return push(n);
  }
  u32 extend(int in, const Prog& p) {
    auto n = blank(RDFGPU_NODE_EXTEND, in); n.table_cols = 1; n.table_slot = (u32)pool.size();
    pool.push_back((u32)exprs.size()); pool.push_back((u32)p.size()); exprs.insert(exprs.end(), p.begin(), p.end()); return push(n);
  }
};
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
  std::printf("%-64s %s  %s\n", name, ok ? "ok  " : "FAIL", text.c_str());
  failures += !ok;
  return plan.nodes;
}
constexpr u32 F = RDFGPU_PLAN_AGG_COLUMNS;
constexpr int UNSUP = RDFGPU_ERR_UNSUPPORTED, INVALID = RDFGPU_ERR_INVALID;
}  // namespace

int main() {
  // ---- kinds and targets
  program("xsd:float(xsd:string(ENC_TV(c))) leaves a typed value", price(0), 1, RDFGPU_OK, VK_TV);
  for (u32 t : {(u32)RDFGPU_TV_BOOLEAN, (u32)RDFGPU_TV_INT, (u32)RDFGPU_TV_INTEGER, (u32)RDFGPU_TV_DECIMAL, (u32)RDFGPU_TV_FLOAT, (u32)RDFGPU_TV_DOUBLE})
    program("CAST_LEX to each of the six targets", {column(0), op(ENC), op(LEX, t)}, 1, RDFGPU_OK, VK_TV);
  for (u32 t : {(u32)RDFGPU_TV_STRING, (u32)RDFGPU_TV_DATE_TIME, (u32)RDFGPU_TV_NAMED_NODE, (u32)RDFGPU_TV_OTHER, 200u})
    program("CAST_LEX to any other target", {column(0), op(ENC), op(LEX, t)}, 1, UNSUP, 0, {"CAST_LEX to tag"});
  program("plain CAST to xsd:string stays refused", {column(0), op(ENC), op(RDFGPU_EX_CAST, RDFGPU_TV_STRING)}, 1, UNSUP, 0, {"CAST to tag"});
  program("CAST_STRING of a typed value: a kind error", {column(0), op(ENC), op(STRING)}, 1, INVALID, 0, {"CAST_STRING", "wrong kind"});
  program("CAST_STRING of a value column: a kind error", {column(0), op(STRING)}, 1, INVALID, 0, {"CAST_STRING", "aggregate value column"}, 1u);
  program("CAST_LEX of an id: a kind error", {column(0), op(LEX, FLOAT)}, 1, INVALID, 0, {"CAST_LEX"});
  program("CAST_LEX of a value column's value is a CAST", {column(0), op(ENC), op(LEX, FLOAT)}, 1, RDFGPU_OK, VK_TV, {}, 1u);
  program("CAST_LEX of a rank-only string literal", {lit(RDFGPU_TV_STRING, 5), op(LEX, FLOAT)}, 0, UNSUP, 0, {"CAST_LEX", "dictionary rank"});
  program("CAST_STRING beside a rank-only string literal", cat({column(0), op(STRING), lit(RDFGPU_TV_STRING, 5)}, {op(RDFGPU_EX_EQ), op(EBV_)}), 1, UNSUP, 0, {"given by rank"});
  program("STRLEN(xsd:string(..)): a view like STR's", {column(0), op(STRING), op(RDFGPU_EX_STRLEN)}, 1, RDFGPU_OK, VK_TV);
  // ---- routing: a predicate or join filter with either op runs in the generic VM
  const Prog q8 = cat(cat(price(0), {column(3), op(ENC), op(LT)}), {op(EBV_)});   // EBV(LT(xsd:float(xsd:string(ENC_TV(price))), avg))
  { Builder b; b.filter((int)b.table(0, 2), cat(cat(price(0), {lit(RDFGPU_TV_FLOAT, 0), op(LT)}), {op(EBV_)}));
    check("FilterExec: the generic VM", expect("FilterExec over the cast", b, 0, RDFGPU_OK).back().shape == 0); }
  { Builder b; b.filter((int)b.table(0, 2), {column(0), op(ENC), lit(RDFGPU_TV_FLOAT, 0), op(LT), op(EBV_)});
    check("  .. and the compare shape without it is still shape 2", expect("FilterExec without the cast", b, 0, RDFGPU_OK).back().shape == 2); }
  for (u32 type : {(u32)RDFGPU_JOIN_INNER, (u32)RDFGPU_JOIN_LEFT, (u32)RDFGPU_JOIN_LEFT_SEMI, (u32)RDFGPU_JOIN_LEFT_ANTI}) {
    Builder b; u32 l = b.table(0, 2), r = b.table(1, 2); b.join(RDFGPU_NODE_HASH_JOIN, type, (int)l, (int)r, q8);
    check("HashJoinExec filter: the generic VM", expect("the BI Q8 join filter, every join type", b, 0, RDFGPU_OK).back().shape == 1); }
  // ---- the hosts that prepare no patterns take the two ops
  { Builder b; b.aggregate((int)b.table(0, 2), RDFGPU_AGG_SUM, price(1)); expect("SUM(xsd:float(xsd:string(ENC_TV(price))))", b, 0, RDFGPU_OK); }
  { Builder b; b.aggregate((int)b.table(0, 2), RDFGPU_AGG_AVG, {column(1), op(STRING), op(LEX, RDFGPU_TV_DECIMAL)}); expect("AVG(xsd:decimal(xsd:string(..)))", b, 0, RDFGPU_OK); }
  { Builder b; b.extend((int)b.table(0, 2), price(1)); expect("a computed column of the cast", b, F, RDFGPU_OK); }
  { Builder b; b.extend((int)b.table(0, 2), {column(1), op(STRING), op(RDFGPU_EX_STRLEN)});
    expect("a computed column with STRLEN stays refused", b, F, UNSUP, {"string functions in a computed column"}); }
  { Builder b; b.aggregate((int)b.table(0, 2), RDFGPU_AGG_SUM, {column(1), op(STRING), op(LEX, RDFGPU_TV_STRING)});
    expect("SUM over a CAST_LEX to xsd:string", b, 0, UNSUP, {"CAST_LEX to tag"}); }
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
