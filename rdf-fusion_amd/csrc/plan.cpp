// plan.cpp — plan compilation (host) and execution (device) of the scan / filter / join subtree.
//
// What replaces what (reference paths relative to the rdf-fusion tree):
//   plan_compile            MemQuadStorePlanner::plan_extension  lib/storage/src/memory/planner.rs:31-64
//                           + plan_pattern_evaluation             storage/snapshot.rs:84-131
//   Plan::exec_source       DataSource::open + MemQuadIndexScanIterator::next  pattern_data_source.rs:42-58, scan.rs:104-212
//   Plan::exec_filter       FilterExec over ENC_TV/GT/ADD/EBV UDFs  (DataFusion 52 + lib/functions)
//   Plan::exec_join         HashJoinExec(CollectLeft) / CrossJoinExec / NestedLoopJoinExec (DataFusion 52),
//                           semantics from lib/logical/src/join/rewrite.rs:71-221
#include "plan.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <shared_mutex>

#include "regex_compile.hpp"

namespace rdfgpu {

// ------------------------------------------------------------------------------------------------
// compile
// ------------------------------------------------------------------------------------------------
namespace {

bool is_cmp(u8 op) {
  return op == RDFGPU_EX_GT || op == RDFGPU_EX_LT || op == RDFGPU_EX_GEQ || op == RDFGPU_EX_LEQ || op == RDFGPU_EX_EQ || op == RDFGPU_EX_NEQ;
}
bool range_op(u8 op) { return op == RDFGPU_EX_GT || op == RDFGPU_EX_LT || op == RDFGPU_EX_GEQ || op == RDFGPU_EX_LEQ; }
// whether column `c` of a join's [left cols, right cols] schema belongs to its build side
bool on_build_side(const LdsJoinArgs& a, u32 c) { return (c < a.n_left_cols) == (a.build_is_left != 0); }

// The literal, arithmetic and comparison of one half of the window shape (detect_join_filter_shape 3) that starts at node `o`.
TvLiteral window_literal(const rdfgpu_expr_node* e, u32 o) {
  TvLiteral l{};
  l.lo = e[o + 4].lo; l.hi = e[o + 4].hi; l.aux = e[o + 4].u; l.tag = e[o + 4].tag; l.flags = e[o + 4].flags;
  l.arith_sub = e[o + 5].op == RDFGPU_EX_SUB; l.cmp_op = e[o + 6].op;
  return l;
}

// Type-checks a postfix program against `n_cols` input columns; returns the kind it leaves.
u32 check_program(const rdfgpu_expr_node* p, u32 n, u32 n_cols, u32 n_regexes = 0) {
  if (n > (u32)kMaxExpr) fail(RDFGPU_ERR_UNSUPPORTED, "expression has %u nodes (max %d)", n, kMaxExpr);
  u32 st[kMaxStack]; bool no_bytes[kMaxStack]; int sp = 0;
  bool views = false, rank_only_string = false;   // computed strings (views) / a string literal given by its rank in the dictionary only
  bool out_no_bytes = false;                      // the value being pushed is such a literal: it has no lexical form on the device
  auto pop = [&](u32 kind, const char* what) {
    if (sp < 1) fail(RDFGPU_ERR_INVALID, "expression: stack underflow at %s", what);
    if (st[--sp] != kind) fail(RDFGPU_ERR_INVALID, "expression: %s got an operand of the wrong kind", what);
  };
  // an operand whose BYTES the op reads (REGEX / CONTAINS / STRSTARTS / STRENDS / STRLEN / SUBSTR / UCASE / LCASE): a string literal
  // that came with its rank only would be the error value on every row — refused here, loudly, instead
  auto pop_bytes = [&](const char* what) {
    if (sp >= 1 && no_bytes[sp - 1]) fail(RDFGPU_ERR_UNSUPPORTED, "%s over a string literal given by its dictionary rank only: it has no lexical form on the device (pass it as RDFGPU_EX_LIT_STR)", what);
    pop(VK_TV, what);
  };
  for (u32 i = 0; i < n; i++) {
    const rdfgpu_expr_node& e = p[i];
    u32 out;
    out_no_bytes = false;
    switch (e.op) {
      case RDFGPU_EX_COLUMN: if (e.u >= n_cols) fail(RDFGPU_ERR_INVALID, "expression: column %u out of range (%u columns)", e.u, n_cols); out = VK_ID; break;
      case RDFGPU_EX_LIT_ID: out = VK_ID; break;
      case RDFGPU_EX_LIT_TV: if (e.tag > RDFGPU_TV_OTHER) fail(RDFGPU_ERR_INVALID, "expression: bad literal tag %u", e.tag); out = VK_TV;
        out_no_bytes = e.tag == RDFGPU_TV_STRING && e.hi == 0;
        rank_only_string = rank_only_string || out_no_bytes; break;
      case RDFGPU_EX_LIT_BOOL: out = VK_BOOL; break;
      case RDFGPU_EX_ENC_TV: pop(VK_ID, "ENC_TV"); out = VK_TV; break;
      case RDFGPU_EX_GT: case RDFGPU_EX_LT: case RDFGPU_EX_GEQ: case RDFGPU_EX_LEQ: case RDFGPU_EX_EQ: case RDFGPU_EX_NEQ:
      case RDFGPU_EX_ADD: case RDFGPU_EX_SUB: case RDFGPU_EX_MUL: case RDFGPU_EX_DIV: pop(VK_TV, "binary typed op"); pop(VK_TV, "binary typed op"); out = VK_TV; break;
      case RDFGPU_EX_NEG: case RDFGPU_EX_PLUS: case RDFGPU_EX_ABS: case RDFGPU_EX_ROUND: case RDFGPU_EX_CEIL: case RDFGPU_EX_FLOOR:
        pop(VK_TV, "unary numeric op"); out = VK_TV; break;
      case RDFGPU_EX_CAST:
        if (e.u != RDFGPU_TV_BOOLEAN && e.u != RDFGPU_TV_INT && e.u != RDFGPU_TV_INTEGER && e.u != RDFGPU_TV_DECIMAL && e.u != RDFGPU_TV_FLOAT && e.u != RDFGPU_TV_DOUBLE)
          fail(RDFGPU_ERR_UNSUPPORTED, "expression: CAST to tag %u (on the device: boolean, int, integer, decimal, float, double)", e.u);
        pop(VK_TV, "CAST"); out = VK_TV; break;
      case RDFGPU_EX_EBV: pop(VK_TV, "EBV"); out = VK_BOOL; break;
      case RDFGPU_EX_REGEX: case RDFGPU_EX_CONTAINS: case RDFGPU_EX_STRSTARTS: case RDFGPU_EX_STRENDS:
        if (e.u >= n_regexes) fail(RDFGPU_ERR_INVALID, "expression: REGEX pattern %u out of range (%u patterns)", e.u, n_regexes);
        // (the operand is any string value: ENC_TV of a column, or a view — STR / SUBSTR / UCASE / LCASE / a constant with bytes)
        pop_bytes("REGEX / CONTAINS / STRSTARTS / STRENDS"); out = VK_TV; break;
      case RDFGPU_EX_STR: pop(VK_ID, "STR"); out = VK_TV; views = true; break;
      case RDFGPU_EX_LIT_STR:
        if (e.u >= n_regexes) fail(RDFGPU_ERR_INVALID, "expression: string constant %u out of range (%u entries)", e.u, n_regexes);
        out = VK_TV; views = true; break;
      case RDFGPU_EX_STRLEN: pop_bytes("STRLEN"); out = VK_TV; break;
      case RDFGPU_EX_SUBSTR:
        if (e.u != 2 && e.u != 3) fail(RDFGPU_ERR_INVALID, "expression: SUBSTR takes 2 or 3 operands, not %u", e.u);
        for (u32 k = 0; k + 1 < e.u; k++) pop(VK_TV, "SUBSTR position / length");
        pop_bytes("SUBSTR");
        out = VK_TV; views = true; break;
      case RDFGPU_EX_UCASE: case RDFGPU_EX_LCASE: pop_bytes("UCASE / LCASE"); out = VK_TV; views = true; break;
      case RDFGPU_EX_STRBEFORE: case RDFGPU_EX_STRAFTER: pop_bytes("STRBEFORE / STRAFTER"); pop_bytes("STRBEFORE / STRAFTER"); out = VK_TV; views = true; break;
      case RDFGPU_EX_REGEX_VAR:
        if (e.lo < 1 || (u64)e.u + (u64)e.lo > n_regexes) fail(RDFGPU_ERR_INVALID, "expression: REGEX pattern table %u .. +%lld out of range (%u patterns)", e.u, (long long)e.lo, n_regexes);
        pop(VK_TV, "REGEX pattern"); pop_bytes("REGEX"); out = VK_TV; break;
      case RDFGPU_EX_LANG_IN:
        if (e.u >= n_regexes) fail(RDFGPU_ERR_INVALID, "expression: language table %u out of range (%u tables)", e.u, n_regexes);
        pop(VK_TV, "LANGMATCHES(LANG())"); out = VK_TV; break;
      case RDFGPU_EX_ID_EQ: case RDFGPU_EX_ID_NEQ: case RDFGPU_EX_IS_COMPATIBLE: pop(VK_ID, "id comparison"); pop(VK_ID, "id comparison"); out = VK_BOOL; break;
      case RDFGPU_EX_AND: case RDFGPU_EX_OR: pop(VK_BOOL, "AND/OR"); pop(VK_BOOL, "AND/OR"); out = VK_BOOL; break;
      case RDFGPU_EX_NOT: pop(VK_BOOL, "NOT"); out = VK_BOOL; break;
      case RDFGPU_EX_BOUND: pop(VK_ID, "BOUND"); out = VK_BOOL; break;
      case RDFGPU_EX_BOOL_AS_TV: pop(VK_BOOL, "BOOLEAN_AS_TERM"); out = VK_TV; break;
      default: fail(RDFGPU_ERR_INVALID, "expression: unknown op %u", e.op);
    }
    if (sp >= kMaxStack) fail(RDFGPU_ERR_UNSUPPORTED, "expression: stack deeper than %d", kMaxStack);
    no_bytes[sp] = out_no_bytes;
    st[sp++] = out;
  }
  if (sp != 1) fail(RDFGPU_ERR_INVALID, "expression leaves %d values on the stack", sp);
  // a computed string compares byte-wise; a string literal that comes with its dictionary rank only has no bytes on the device
  if (views && rank_only_string) fail(RDFGPU_ERR_UNSUPPORTED, "expression mixes computed strings (STR / SUBSTR / UCASE / LCASE) with a string literal given by rank: pass the literal as RDFGPU_EX_LIT_STR");
  return st[0];
}

int detect_shape(const ExprProgram& pr, bool force_vm) {
  if (force_vm) return 0;
  const rdfgpu_expr_node* e = pr.nodes;
  if (pr.n == 3 && e[0].op == RDFGPU_EX_COLUMN && e[1].op == RDFGPU_EX_LIT_ID && (e[2].op == RDFGPU_EX_ID_EQ || e[2].op == RDFGPU_EX_ID_NEQ)) return 1;
  if (pr.n == 5 && e[0].op == RDFGPU_EX_COLUMN && e[1].op == RDFGPU_EX_ENC_TV && e[2].op == RDFGPU_EX_LIT_TV && is_cmp(e[3].op) && e[4].op == RDFGPU_EX_EBV) return 2;
  // EBV(REGEX | CONTAINS | STRSTARTS | STRENDS (ENC_TV(col), constant)): answered per distinct term (shape 3) when the
  // table is large enough to pay for a pass over the dictionary, else by the VM per row
  if (pr.n == 4 && e[0].op == RDFGPU_EX_COLUMN && e[1].op == RDFGPU_EX_ENC_TV && e[3].op == RDFGPU_EX_EBV &&
      (e[2].op == RDFGPU_EX_REGEX || e[2].op == RDFGPU_EX_CONTAINS || e[2].op == RDFGPU_EX_STRSTARTS || e[2].op == RDFGPU_EX_STRENDS)) return 3;
  return 0;
}

// Join-filter specialisation: 3 = the BSBM Q5 "window" shape
//   EBV(cmp(ENC_TV(x), ADD|SUB(ENC_TV(y), lit))) AND EBV(cmp(ENC_TV(x'), ADD|SUB(ENC_TV(y'), lit')))
// (Q5 (Execution Plan).snap:10,12), 1 = generic VM, 0 = no filter.
int detect_join_filter_shape(const ExprProgram& pr, bool force_vm) {
  if (pr.n == 0) return 0;
  if (force_vm) return 1;
  const rdfgpu_expr_node* e = pr.nodes;
  auto half = [&](u32 o) {
    return e[o].op == RDFGPU_EX_COLUMN && e[o + 1].op == RDFGPU_EX_ENC_TV && e[o + 2].op == RDFGPU_EX_COLUMN &&
           e[o + 3].op == RDFGPU_EX_ENC_TV && e[o + 4].op == RDFGPU_EX_LIT_TV &&
           (e[o + 5].op == RDFGPU_EX_ADD || e[o + 5].op == RDFGPU_EX_SUB) && is_cmp(e[o + 6].op) && e[o + 7].op == RDFGPU_EX_EBV;
  };
  if (pr.n == 17 && half(0) && half(8) && e[16].op == RDFGPU_EX_AND) return 3;
  // 2 = column <ID_EQ | ID_NEQ> column
  if (pr.n == 3 && e[0].op == RDFGPU_EX_COLUMN && e[1].op == RDFGPU_EX_COLUMN && (e[2].op == RDFGPU_EX_ID_EQ || e[2].op == RDFGPU_EX_ID_NEQ)) return 2;
  return 1;
}

void load_program(NodeInfo& nd, const rdfgpu_plan_desc* d, u32 n_cols, const char* what, const RegexProg* regex_dev, const unsigned char* str_consts = nullptr) {
  const rdfgpu_plan_node& r = nd.d;
  nd.prog.n = 0;
  if (r.expr_len == 0) return;
  if ((u64)r.expr_off + r.expr_len > d->n_exprs) fail(RDFGPU_ERR_INVALID, "%s: expression outside the expression array", what);
  if (check_program(d->exprs + r.expr_off, r.expr_len, n_cols, d->n_regexes) != VK_BOOL) fail(RDFGPU_ERR_INVALID, "%s: predicate does not yield a boolean", what);
  nd.prog.n = r.expr_len;
  std::memcpy(nd.prog.nodes, d->exprs + r.expr_off, r.expr_len * sizeof(rdfgpu_expr_node));
  nd.prog.regex = regex_dev;
  nd.prog.str_consts = str_consts;
}

void load_projection(NodeInfo& nd, const rdfgpu_plan_desc* d, u32 full, const char* what) {
  const rdfgpu_plan_node& r = nd.d;
  if (r.n_proj == RDFGPU_NO_PROJECTION) {
    if (full > (u32)kMaxCols) fail(RDFGPU_ERR_UNSUPPORTED, "%s: %u columns (max %d)", what, full, kMaxCols);
    nd.n_proj = full;
    for (u32 i = 0; i < full; i++) nd.proj[i] = i;
  } else {
    if (r.n_proj > (u32)kMaxCols) fail(RDFGPU_ERR_UNSUPPORTED, "%s: %u columns (max %d)", what, r.n_proj, kMaxCols);
    if ((u64)r.proj_off + r.n_proj > d->n_pool) fail(RDFGPU_ERR_INVALID, "%s: projection outside the pool", what);
    nd.n_proj = r.n_proj;
    for (u32 i = 0; i < r.n_proj; i++) {
      nd.proj[i] = d->pool[r.proj_off + i];
      if (nd.proj[i] >= full) fail(RDFGPU_ERR_INVALID, "%s: projection column %u out of range (%u columns)", what, nd.proj[i], full);
    }
  }
  nd.width = nd.n_proj;
}

}  // namespace

Plan* plan_compile(Store* store, const rdfgpu_plan_desc* d) {
  if (!store) fail(RDFGPU_ERR_INVALID, "plan_compile: null store");
  if (!d || !d->nodes || d->n_nodes == 0) fail(RDFGPU_ERR_INVALID, "plan_compile: empty plan");
  if (d->root >= d->n_nodes) fail(RDFGPU_ERR_INVALID, "plan_compile: root %u out of range", d->root);
  std::unique_ptr<Plan> plan(new Plan());
  plan->store = store;
  plan->opt = store->opt;
  store->retain();
  plan->root = d->root;
  plan->nodes.resize(d->n_nodes);
  std::vector<u32> scan_ids;  // sorted IN sets of all sources, uploaded once
  if (d->n_regexes) {   // REGEX patterns are plan constants: compiled here, simulated per row on the device
    if (!d->regexes) fail(RDFGPU_ERR_INVALID, "plan_compile: %u regexes but no table", d->n_regexes);
    // how each table entry is used decides how it is compiled: REGEX = a pattern with flags; CONTAINS / STRSTARTS /
    // STRENDS = a literal needle (like the `q` flag), anchored at the start / end for the latter two
    std::vector<int> use(d->n_regexes, -1);
    for (u32 i = 0; i < d->n_exprs; i++) {
      const rdfgpu_expr_node& e = d->exprs[i];
      if (e.op == RDFGPU_EX_REGEX_VAR) {   // a table of per-row patterns: entries u .. u + lo, all REGEX patterns
        for (int64_t k = 0; k < e.lo && (u64)e.u + (u64)k < d->n_regexes; k++) use[e.u + k] = RDFGPU_EX_REGEX;
        continue;
      }
      if (e.op != RDFGPU_EX_REGEX && e.op != RDFGPU_EX_CONTAINS && e.op != RDFGPU_EX_STRSTARTS && e.op != RDFGPU_EX_STRENDS && e.op != RDFGPU_EX_LANG_IN && e.op != RDFGPU_EX_LIT_STR) continue;
      if (e.u >= d->n_regexes) fail(RDFGPU_ERR_INVALID, "expression: string pattern %u out of range", e.u);
      if (use[e.u] >= 0 && use[e.u] != (int)e.op) fail(RDFGPU_ERR_INVALID, "string pattern %u is used by two different functions", e.u);
      use[e.u] = (int)e.op;
    }
    std::vector<RegexProg> progs(d->n_regexes);
    std::vector<unsigned char> consts;   // the bytes of the string constants (RDFGPU_EX_LIT_STR), back to back
    for (u32 r = 0; r < d->n_regexes; r++) {
      const rdfgpu_regex& rx = d->regexes[r];
      if (use[r] == RDFGPU_EX_LIT_STR) {   // not a pattern: raw bytes — the slot holds where they are
        std::memset(&progs[r], 0, sizeof(RegexProg));
        progs[r].first = consts.size(); progs[r].n_pos = rx.pattern_len;
        if (rx.pattern_len && !rx.pattern) fail(RDFGPU_ERR_INVALID, "string constant %u: null text", r);
        consts.insert(consts.end(), reinterpret_cast<const unsigned char*>(rx.pattern), reinterpret_cast<const unsigned char*>(rx.pattern) + rx.pattern_len);
        continue;
      }
      if (use[r] == RDFGPU_EX_LANG_IN) {   // not a pattern: one verdict byte per language id -> a bit set in the slot
        std::memset(&progs[r], 0, sizeof(RegexProg));
        if (rx.pattern_len > 256u * 64u) fail(RDFGPU_ERR_UNSUPPORTED, "language table %u: %u language ids (max 16384)", r, rx.pattern_len);
        for (u32 l = 0; l < rx.pattern_len; l++) if (rx.pattern[l]) progs[r].byte_mask[l >> 6] |= 1ull << (l & 63u);
        progs[r].n_pos = rx.pattern_len;
        continue;
      }
      if (use[r] >= 0 && !store->str_off) fail(RDFGPU_ERR_INVALID, "plan uses string functions but the store has no strings (rdfgpu_store_set_strings)");
      std::string why;
      const bool literal = use[r] == RDFGPU_EX_CONTAINS || use[r] == RDFGPU_EX_STRSTARTS || use[r] == RDFGPU_EX_STRENDS;
      const char* flags = literal ? "q" : (rx.flags ? rx.flags : "");
      const size_t n_flags = literal ? 1 : (rx.flags ? rx.flags_len : 0);
      if (regex_compile(rx.pattern ? rx.pattern : "", rx.pattern_len, flags, n_flags, progs[r], why) != REGEX_OK)
        fail(RDFGPU_ERR_UNSUPPORTED, "string pattern %u: %s", r, why.c_str());
      progs[r].pattern_id = rx.pattern_id;
      if (use[r] == RDFGPU_EX_STRSTARTS) progs[r].anchor_start = 1;
      if (use[r] == RDFGPU_EX_STRENDS) progs[r].anchor_end = 1;
    }
    for (u32 r = 0; r < d->n_regexes; r++) {   // own copies of the texts: they key the store's per-term verdict tables
      const rdfgpu_regex& rx = d->regexes[r];
      plan->regex_strings.emplace_back(rx.pattern ? std::string(rx.pattern, rx.pattern_len) : std::string());
      plan->regex_strings.emplace_back(rx.flags ? std::string(rx.flags, rx.flags_len) : std::string());
    }
    for (u32 r = 0; r < d->n_regexes; r++) {
      rdfgpu_regex rx{};
      rx.pattern = plan->regex_strings[2 * r].data(); rx.pattern_len = (u32)plan->regex_strings[2 * r].size();
      rx.flags = plan->regex_strings[2 * r + 1].data(); rx.flags_len = (u32)plan->regex_strings[2 * r + 1].size();
      plan->regex_text.push_back(rx);
    }
    store->activate();
    RDFGPU_HIP(hipMalloc((void**)&plan->regex_dev, progs.size() * sizeof(RegexProg)));
    RDFGPU_HIP(hipMemcpy(plan->regex_dev, progs.data(), progs.size() * sizeof(RegexProg), hipMemcpyHostToDevice));
    bool any_const = false;
    for (int u_ : use) any_const = any_const || u_ == RDFGPU_EX_LIT_STR;
    if (any_const) {   // (at least one byte: the empty string is a constant too, and a null base would read as "no bytes on the device")
      RDFGPU_HIP(hipMalloc((void**)&plan->str_consts_dev, consts.size() + 1));
      if (!consts.empty()) RDFGPU_HIP(hipMemcpy(plan->str_consts_dev, consts.data(), consts.size(), hipMemcpyHostToDevice));
    }
  }

  for (u32 i = 0; i < d->n_exprs; i++) {
    const u8 op = d->exprs[i].op;
    if ((op == RDFGPU_EX_STR || op == RDFGPU_EX_STRLEN || op == RDFGPU_EX_SUBSTR || op == RDFGPU_EX_UCASE || op == RDFGPU_EX_LCASE || op == RDFGPU_EX_STRBEFORE || op == RDFGPU_EX_STRAFTER) && !store->str_off)
      fail(RDFGPU_ERR_INVALID, "plan uses string functions but the store has no strings (rdfgpu_store_set_strings)");
  }
  for (u32 i = 0; i < d->n_nodes; i++) {
    NodeInfo& nd = plan->nodes[i];
    nd.d = d->nodes[i];
    const rdfgpu_plan_node& r = nd.d;
    auto child = [&](int32_t c, const char* what) -> const NodeInfo& {
      if (c < 0 || (u32)c >= i) fail(RDFGPU_ERR_INVALID, "node %u: %s child %d must precede the node", i, what, c);
      if (plan->nodes[c].d.kind == RDFGPU_NODE_AGGREGATE && plan->nodes[c].n_aggs)   // aggregate values are not object ids
        fail(RDFGPU_ERR_UNSUPPORTED, "node %u: input %d is an AggregateExec with aggregates, which must be the plan's root", i, c);
      return plan->nodes[c];
    };
    switch (r.kind) {
      case RDFGPU_NODE_DATA_SOURCE: {
        SourceInfo src;
        src.node = i;
        src.gspo = make_gspo(r.scan, d->pool, d->n_pool);
        plan->derive_source(src, src.gspo);
        nd.width = src.n_out;
        nd.source = (int)plan->sources.size();
        plan->sources.push_back(src);
        break;
      }
      case RDFGPU_NODE_FILTER: {
        const NodeInfo& c = child(r.left, "input");
        load_program(nd, d, c.width, "FilterExec", plan->regex_dev, plan->str_consts_dev);
        load_projection(nd, d, c.width, "FilterExec");
        nd.shape = detect_shape(nd.prog, plan->opt.on(RDFGPU_OPT_FORCE_GENERIC_VM));
        break;
      }
      case RDFGPU_NODE_PROJECTION: {
        const NodeInfo& c = child(r.left, "input");
        load_projection(nd, d, c.width, "ProjectionExec");
        break;
      }
      case RDFGPU_NODE_HASH_JOIN: case RDFGPU_NODE_CROSS_JOIN: case RDFGPU_NODE_NESTED_LOOP_JOIN: {
        const NodeInfo& l = child(r.left, "left");
        const NodeInfo& rr = child(r.right, "right");
        const bool semi = r.join_type == RDFGPU_JOIN_LEFT_SEMI || r.join_type == RDFGPU_JOIN_LEFT_ANTI;
        if (r.join_type != RDFGPU_JOIN_INNER && r.join_type != RDFGPU_JOIN_LEFT && !semi) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: join type %u", i, r.join_type);
        if (r.kind == RDFGPU_NODE_HASH_JOIN) {
          if (r.n_keys == 0 || r.n_keys > RDFGPU_MAX_KEYS) fail(RDFGPU_ERR_INVALID, "node %u: HashJoinExec needs 1..%u keys", i, RDFGPU_MAX_KEYS);
          for (u32 k = 0; k < r.n_keys; k++)
            if (r.left_keys[k] >= l.width || r.right_keys[k] >= rr.width) fail(RDFGPU_ERR_INVALID, "node %u: join key out of range", i);
        }
        if (r.kind == RDFGPU_NODE_CROSS_JOIN && (r.expr_len || r.join_type != RDFGPU_JOIN_INNER)) fail(RDFGPU_ERR_INVALID, "node %u: CrossJoinExec takes no filter / join type", i);
        if (l.width + rr.width > 2u * kMaxCols) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: too many columns", i);
        load_program(nd, d, l.width + rr.width, "join filter", plan->regex_dev, plan->str_consts_dev);
        // a semi / anti join outputs the left columns only: its projection indexes them (the filter still sees both sides)
        load_projection(nd, d, semi ? l.width : l.width + rr.width, "join");
        nd.shape = detect_join_filter_shape(nd.prog, plan->opt.on(RDFGPU_OPT_FORCE_GENERIC_VM));
        if (l.width > (u32)kMaxCols || rr.width > (u32)kMaxCols) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: too many columns", i);
        break;
      }
      case RDFGPU_NODE_CLOSURE: {
        const NodeInfo& c = child(r.left, "inner paths");
        if (c.width != 3) fail(RDFGPU_ERR_INVALID, "node %u: KleenePlusClosureExec input has %u columns, not (graph, start, end)", i, c.width);
        if (r.join_type > 1) fail(RDFGPU_ERR_INVALID, "node %u: allow_cross_graph_paths is 0 or 1", i);
        load_projection(nd, d, 3, "KleenePlusClosureExec");
        break;
      }
      case RDFGPU_NODE_UNION: {
        const NodeInfo& l = child(r.left, "left");
        const NodeInfo& rr = child(r.right, "right");
        if (l.width != rr.width) fail(RDFGPU_ERR_INVALID, "node %u: UnionExec inputs have %u and %u columns", i, l.width, rr.width);
        load_projection(nd, d, l.width, "UnionExec");
        break;
      }
      case RDFGPU_NODE_TABLE: {
        if (r.table_cols > (u32)kMaxCols) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: table with %u columns", i, r.table_cols);
        nd.width = r.table_cols;
        if (plan->tables.size() <= r.table_slot) plan->tables.resize(r.table_slot + 1);
        break;
      }
      case RDFGPU_NODE_TOPK: {   // DISTINCT + TopK(fetch) per group, ..Q5 (Execution Plan).snap:5-9
        const NodeInfo& c = child(r.left, "input");
        if (r.n_keys < 1 || r.n_keys > RDFGPU_MAX_KEYS) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: TopK with %u sort keys (1 to %u)", i, r.n_keys, RDFGPU_MAX_KEYS);
        if (r.table_cols < 1 || r.table_cols > 1024) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: TopK fetch = %u", i, r.table_cols);
        for (u32 k = 0; k < r.n_keys; k++) {
          if (r.left_keys[k] >= c.width) fail(RDFGPU_ERR_INVALID, "node %u: sort key column %u out of range", i, r.left_keys[k]);
          if (r.right_keys[k] > RDFGPU_SORT_BY_DOUBLE) fail(RDFGPU_ERR_INVALID, "node %u: unknown sort mode %u", i, r.right_keys[k]);
        }
        if (r.table_slot > c.width) fail(RDFGPU_ERR_INVALID, "node %u: group column out of range", i);
        load_projection(nd, d, c.width, "TopK");
        for (u32 q = 0; q < nd.n_proj; q++) {   // DISTINCT is over (group, keys): the output may not carry anything else
          bool covered = r.table_slot != 0 && nd.proj[q] == r.table_slot - 1;
          for (u32 k = 0; k < r.n_keys; k++) covered = covered || (nd.proj[q] == r.left_keys[k] && r.right_keys[k] == RDFGPU_SORT_BY_ID);
          if (!covered) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: TopK output column %u is neither the group nor a sort key by id", i, nd.proj[q]);
        }
        nd.width = nd.n_proj;
        break;
      }
      case RDFGPU_NODE_AGGREGATE: {   // AggregateExec(mode=Single), ..Business Intelligence - Q8 (Execution Plan).snap
        const NodeInfo& c = child(r.left, "input");
        if (r.n_keys > RDFGPU_MAX_KEYS) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: AggregateExec with %u group columns (at most %u)", i, r.n_keys, RDFGPU_MAX_KEYS);
        if (r.table_cols > RDFGPU_MAX_AGGREGATES) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: AggregateExec with %u aggregates (at most %u)", i, r.table_cols, RDFGPU_MAX_AGGREGATES);
        if (r.n_proj != RDFGPU_NO_PROJECTION) fail(RDFGPU_ERR_INVALID, "node %u: AggregateExec takes no projection", i);
        if (r.n_keys + r.table_cols == 0) fail(RDFGPU_ERR_INVALID, "node %u: AggregateExec without group columns and aggregates", i);
        for (u32 k = 0; k < r.n_keys; k++)
          if (r.left_keys[k] >= c.width) fail(RDFGPU_ERR_INVALID, "node %u: group column %u out of range", i, r.left_keys[k]);
        if (r.table_cols && ((u64)r.table_slot + 2ull * r.table_cols > d->n_pool || !d->pool)) fail(RDFGPU_ERR_INVALID, "node %u: aggregate list outside the pool", i);
        for (u32 a = 0; a < r.table_cols; a++) {
          const u32 fn = d->pool[r.table_slot + 2 * a], in = d->pool[r.table_slot + 2 * a + 1];
          const bool expr = fn != RDFGPU_AGG_COUNT_STAR && (in & RDFGPU_AGG_INPUT_EXPR) != 0;
          switch (fn) {
            case RDFGPU_AGG_COUNT_STAR: break;
            case RDFGPU_AGG_COUNT: case RDFGPU_AGG_COUNT_DISTINCT:
              if (expr) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: aggregate %u: COUNT / COUNT DISTINCT over an expression is not on the device (SUM and AVG are)", i, a);
              [[fallthrough]];
            case RDFGPU_AGG_SUM: case RDFGPU_AGG_AVG:
              if (expr) {   // (expr_off, expr_len) in the pool: a program over the input's columns that leaves a typed value
                const u32 at = in & ~RDFGPU_AGG_INPUT_EXPR;
                if ((u64)at + 2 > d->n_pool) fail(RDFGPU_ERR_INVALID, "node %u: aggregate %u: expression input at pool offset %u of %u", i, a, at, d->n_pool);
                const u32 off = d->pool[at], len = d->pool[at + 1];
                if (len == 0 || (u64)off + len > d->n_exprs) fail(RDFGPU_ERR_INVALID, "node %u: aggregate %u: expression outside the expression array", i, a);
                for (u32 q = 0; q < len; q++) {   // the pattern ops get their per-node preparation in FilterExec and the joins only
                  const u8 op = d->exprs[off + q].op;
                  if (op == RDFGPU_EX_REGEX || op == RDFGPU_EX_REGEX_VAR || op == RDFGPU_EX_CONTAINS || op == RDFGPU_EX_STRSTARTS || op == RDFGPU_EX_STRENDS || op == RDFGPU_EX_LANG_IN)
                    fail(RDFGPU_ERR_UNSUPPORTED, "node %u: aggregate %u: REGEX / CONTAINS / STRSTARTS / STRENDS / LANGMATCHES in an aggregate's input expression are not on the device", i, a);
                }
                if (check_program(d->exprs + off, len, c.width, d->n_regexes) != VK_TV) fail(RDFGPU_ERR_INVALID, "node %u: aggregate %u: the input expression does not yield a typed value", i, a);
                ExprProgram pr{};
                pr.n = len;
                std::memcpy(pr.nodes, d->exprs + off, len * sizeof(rdfgpu_expr_node));
                pr.regex = plan->regex_dev; pr.str_consts = plan->str_consts_dev;
                nd.agg_prog[a] = (int)nd.agg_progs.size();
                nd.agg_progs.push_back(pr);
              } else if (in >= c.width) fail(RDFGPU_ERR_INVALID, "node %u: aggregate %u reads column %u of %u", i, a, in, c.width);
              break;
            case RDFGPU_AGG_MIN: case RDFGPU_AGG_MAX: case RDFGPU_AGG_SAMPLE: case RDFGPU_AGG_GROUP_CONCAT:
              fail(RDFGPU_ERR_UNSUPPORTED, "node %u: aggregate %u: MIN / MAX / SAMPLE / GROUP_CONCAT are not on the device (MIN / MAX keep the first "
                                           "value's error state, min.rs:42-53: their result depends on row order)", i, a);
            case RDFGPU_AGG_SUM_DISTINCT: case RDFGPU_AGG_AVG_DISTINCT: case RDFGPU_AGG_COUNT_DISTINCT_STAR:
              fail(RDFGPU_ERR_UNSUPPORTED, "node %u: aggregate %u: SUM / AVG with DISTINCT and COUNT(DISTINCT *) are not on the device", i, a);
            default: fail(RDFGPU_ERR_INVALID, "node %u: aggregate %u: unknown function %u", i, a, fn);
          }
          nd.agg_fn[a] = fn; nd.agg_col[a] = fn == RDFGPU_AGG_COUNT_STAR || expr ? 0 : in;
        }
        nd.n_aggs = r.table_cols;
        if (nd.n_aggs && i != d->root) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: an AggregateExec with aggregates must be the plan's root (node %u)", i, d->root);
        nd.width = r.n_keys;   // the id columns; the aggregates leave through rdfgpu_plan_agg_*
        break;
      }
      default: fail(RDFGPU_ERR_INVALID, "node %u: unknown kind %u", i, r.kind);
    }
  }

  // Join reordering (physical rewrite, results unchanged): an inner HashJoinExec whose build child is a
  // CrossJoinExec(A, B) and whose equi-keys come partly from A and partly from B
  //     (A x B) JOIN C ON a = c1 AND b = c2          (Q5 (Execution Plan).snap:18-26: label x features(X))
  // is the join graph A - C - B; it runs as  A JOIN (B JOIN C ON b = c2) ON a = c1  without ever
  // materialising |A| x |B| rows.  Column order [A, B, C] is preserved, so filter and projection stay valid.
  if (!plan->opt.on(RDFGPU_OPT_NO_JOIN_REORDER)) {
    const u32 n0 = (u32)plan->nodes.size();
    std::vector<u32> refs(n0, 0);
    for (u32 i = 0; i < n0; i++) {
      if (plan->nodes[i].d.left >= 0) refs[plan->nodes[i].d.left]++;
      if (plan->nodes[i].d.right >= 0) refs[plan->nodes[i].d.right]++;
    }
    for (u32 i = 0; i < n0; i++) {
      if (plan->nodes[i].d.kind != RDFGPU_NODE_HASH_JOIN || plan->nodes[i].d.join_type != RDFGPU_JOIN_INNER) continue;
      const u32 ci = (u32)plan->nodes[i].d.left;
      if (plan->nodes[ci].d.kind != RDFGPU_NODE_CROSS_JOIN || refs[ci] != 1) continue;
      const u32 ai = (u32)plan->nodes[ci].d.left, bi = (u32)plan->nodes[ci].d.right, cri = (u32)plan->nodes[i].d.right;
      const u32 wA = plan->nodes[ai].width, wB = plan->nodes[bi].width, wC = plan->nodes[cri].width;
      bool identity = plan->nodes[ci].n_proj == wA + wB;
      for (u32 k = 0; identity && k < wA + wB; k++) identity = plan->nodes[ci].proj[k] == k;
      if (!identity || wB + wC > (u32)kMaxCols) continue;
      rdfgpu_plan_node jd = plan->nodes[i].d;
      u32 nA = 0, nB = 0;
      rdfgpu_plan_node td{};   // T = B JOIN C
      td.kind = RDFGPU_NODE_HASH_JOIN; td.join_type = RDFGPU_JOIN_INNER; td.left = (int32_t)bi; td.right = (int32_t)cri;
      td.n_proj = RDFGPU_NO_PROJECTION;
      u32 la[RDFGPU_MAX_KEYS], ra[RDFGPU_MAX_KEYS];
      for (u32 k = 0; k < jd.n_keys; k++) {
        if (jd.left_keys[k] < wA) { la[nA] = jd.left_keys[k]; ra[nA] = wB + jd.right_keys[k]; nA++; }
        else { td.left_keys[nB] = jd.left_keys[k] - wA; td.right_keys[nB] = jd.right_keys[k]; nB++; }
      }
      if (nA == 0 || nB == 0) continue;
      td.n_keys = nB;
      NodeInfo t;
      t.d = td; t.width = wB + wC; t.n_proj = wB + wC;
      for (u32 k = 0; k < wB + wC; k++) t.proj[k] = k;
      plan->nodes.push_back(t);
      NodeInfo& j = plan->nodes[i];
      j.d.left = (int32_t)ai; j.d.right = (int32_t)(plan->nodes.size() - 1);
      j.d.n_keys = nA;
      for (u32 k = 0; k < nA; k++) { j.d.left_keys[k] = la[k]; j.d.right_keys[k] = ra[k]; }
    }
  }

  // consumers per node, counted over the operators reachable from the root only (a rewritten-away
  // CrossJoinExec must not keep its former inputs "shared")
  for (NodeInfo& nd : plan->nodes) nd.refs = 0;
  {
    std::vector<u32> stack{plan->root};
    std::vector<bool> seen(plan->nodes.size(), false);
    while (!stack.empty()) {
      const u32 i = stack.back(); stack.pop_back();
      if (seen[i]) continue;
      seen[i] = true;
      const NodeInfo& nd = plan->nodes[i];
      if (nd.d.kind == RDFGPU_NODE_DATA_SOURCE || nd.d.kind == RDFGPU_NODE_TABLE) continue;
      const bool binary = nd.d.kind == RDFGPU_NODE_HASH_JOIN || nd.d.kind == RDFGPU_NODE_CROSS_JOIN || nd.d.kind == RDFGPU_NODE_NESTED_LOOP_JOIN || nd.d.kind == RDFGPU_NODE_UNION;
      if (nd.d.left >= 0) { plan->nodes[nd.d.left].refs++; stack.push_back((u32)nd.d.left); }
      if (binary && nd.d.right >= 0) { plan->nodes[nd.d.right].refs++; stack.push_back((u32)nd.d.right); }
    }
  }
  for (u32 i = 0; i < plan->nodes.size(); i++) {   // the one consumer of a node consumed once
    const NodeInfo& nd = plan->nodes[i];
    if (nd.d.kind == RDFGPU_NODE_DATA_SOURCE || nd.d.kind == RDFGPU_NODE_TABLE) continue;
    const bool binary = nd.d.kind == RDFGPU_NODE_HASH_JOIN || nd.d.kind == RDFGPU_NODE_CROSS_JOIN || nd.d.kind == RDFGPU_NODE_NESTED_LOOP_JOIN || nd.d.kind == RDFGPU_NODE_UNION;
    if (i != plan->root && nd.refs == 0) continue;   // (rewritten away: not an operator of this plan any more)
    if (nd.d.left >= 0 && plan->nodes[nd.d.left].refs == 1) plan->nodes[nd.d.left].parent = (int)i;
    if (binary && nd.d.right >= 0 && plan->nodes[nd.d.right].refs == 1) plan->nodes[nd.d.right].parent = (int)i;
  }
  // per-node byte accounting inputs: distinct columns read, typed gathers per row
  for (NodeInfo& nd : plan->nodes) {
    bool used[2 * kMaxCols] = {};
    for (u32 i = 0; i < nd.prog.n; i++) {
      if (nd.prog.nodes[i].op == RDFGPU_EX_COLUMN) used[nd.prog.nodes[i].u] = true;
      if (nd.prog.nodes[i].op == RDFGPU_EX_ENC_TV) nd.n_enc_tv++;
    }
    if (nd.d.kind == RDFGPU_NODE_FILTER) for (u32 c = 0; c < nd.n_proj; c++) used[nd.proj[c]] = true;
    for (bool b : used) nd.n_cols_read += b;
  }

  static_assert(sizeof(LocateJob) <= 128, "ExecContext staging assumes LocateJob <= 128 bytes");
  plan->ctx = store->acquire_context((u32)plan->sources.size());
  plan->stream = plan->ctx->stream;
  plan->counters = plan->ctx->counters;
  plan->upload_pool();
  return plan.release();
}

// The scan of a pattern from its G,S,P,O instructions: index choice (IndexPermutations::choose_index, permutations.rs:81-96),
// the instructions in that index's order, the pruning levels and what they make redundant, the output columns in G,S,P,O
// order of first binding (patterns/mod.rs:68-107).
void Plan::derive_source(SourceInfo& src, const ScanInstructions& gspo) {
  src.components = choose_index(gspo, 0b111);
  src.ix = reorder(gspo, src.components);
  src.prune = plan_pruning(src.ix);
  src.n_out = 0; src.has_residual = false;
  for (int k = 0; k < 4; k++) {
    if (gspo.in[k].kind != RDFGPU_SCAN) continue;
    bool first = true;
    for (int j = 0; j < k; j++) if (gspo.in[j].kind == RDFGPU_SCAN && gspo.in[j].var == gspo.in[k].var) first = false;
    if (!first) continue;
    for (int lvl = 0; lvl < 4; lvl++)
      if (src.ix.in[lvl].kind == RDFGPU_SCAN && src.ix.in[lvl].var == gspo.in[k].var) src.out_level[src.n_out] = lvl;
    src.n_out++;
  }
  for (int k = 0; k < 4; k++)
    if (src.ix.in[k].pred.kind != RDFGPU_PRED_NONE && !(src.prune.dropped_mask & (1u << k))) src.has_residual = true;
}
// IN sets of residual predicates live on the device: uploaded at compile time and again when push-down changed them
void Plan::upload_pool() {
  pool.clear();
  for (SourceInfo& s : sources)
    for (int k = 0; k < 4; k++)
      if (s.ix.in[k].pred.kind == RDFGPU_PRED_IN && !(s.prune.dropped_mask & (1u << k))) {
        s.ix.in[k].pred.from = (u32)pool.size();
        pool.insert(pool.end(), s.ix.in[k].pred.ids.begin(), s.ix.in[k].pred.ids.end());
      }
  store->activate();
  if (stream) RDFGPU_HIP(hipStreamSynchronize(stream));
  if (pool_dev) { RDFGPU_HIP(hipFree(pool_dev)); pool_dev = nullptr; }
  if (!pool.empty()) {
    RDFGPU_HIP(hipMalloc((void**)&pool_dev, pool.size() * 4));
    RDFGPU_HIP(hipMemcpy(pool_dev, pool.data(), pool.size() * 4, hipMemcpyHostToDevice));
  }
}

namespace {
// MemStoragePredicateExpr -> MemIndexScanPredicate (to_scan_predicate, predicate_pushdown.rs:120-157); false = `true` (no predicate)
bool filter_to_predicate(const rdfgpu_pushdown_filter& f, ScanPredicate* out) {
  if (f.kind == RDFGPU_PUSH_TRUE) return false;
  if (f.kind == RDFGPU_PUSH_BINARY) { *out = pushdown_to_scan_predicate(f.op, f.value); return true; }
  if (f.kind == RDFGPU_PUSH_BETWEEN) {
    ScanPredicate p;
    if (f.from > f.to) p.kind = RDFGPU_PRED_FALSE; else { p.kind = RDFGPU_PRED_BETWEEN; p.from = f.from; p.to = f.to; }
    *out = p; return true;
  }
  fail(RDFGPU_ERR_INVALID, "push-down filter of kind %u", f.kind);
}
// MemIndexScanInstructions::apply_filter (scan_instructions.rs:101-133)
void and_into_instructions(ScanInstructions& gspo, u32 var, const ScanPredicate& p) {
  int at = -1;
  for (int k = 0; k < 4 && at < 0; k++) if (gspo.in[k].kind == RDFGPU_SCAN && gspo.in[k].var == var) at = k;   // instructions_for_column: the first binding
  if (at < 0) fail(RDFGPU_ERR_INVALID, "Could not find scan instruction for column: variable %u", var);
  ScanPredicate combined = p;
  if (gspo.in[at].pred.kind != RDFGPU_PRED_NONE && !predicate_and(gspo.in[at].pred, p, &combined))
    fail(RDFGPU_ERR_INVALID, "Could not apply predicate to scan instruction.");
  gspo.in[at].pred = combined;
}
}  // namespace

void Plan::pushdown_filters(u32 node, const rdfgpu_pushdown_filter* filters, u32 n, u8* pushed) {
  if (node >= nodes.size() || nodes[node].source < 0) fail(RDFGPU_ERR_INVALID, "node %u is not a data source", node);
  SourceInfo& src = sources[nodes[node].source];
  ScanInstructions gspo = src.gspo;
  bool any = false;
  for (u32 i = 0; i < n; i++) {
    const bool yes = filters[i].kind != RDFGPU_PUSH_UNSUPPORTED;   // rewritten => PushedDown::Yes (pattern_data_source.rs:121-127)
    if (pushed) pushed[i] = yes ? 1 : 0;
    if (!yes) continue;
    any = true;
    ScanPredicate p;
    if (filter_to_predicate(filters[i], &p)) and_into_instructions(gspo, filters[i].var, p);
  }
  if (!any) return;                       // "Don't create a new node if no filters were pushed down"
  src.gspo = gspo;
  derive_source(src, src.gspo);           // apply_pushdown_filters ends in try_find_better_index
  src.dynamic_dirty = !src.dynamic.empty();
  upload_pool();
  located_version = ~0ull;                // the cached ranges belong to the old instructions
  for (NodeInfo& nd : nodes) { nd.has_last = false; nd.last_rows = 0; }   // and so do the cardinalities
}

void Plan::set_dynamic_filters(u32 node, const rdfgpu_pushdown_filter* filters, u32 n) {
  if (node >= nodes.size() || nodes[node].source < 0) fail(RDFGPU_ERR_INVALID, "node %u is not a data source", node);
  SourceInfo& src = sources[nodes[node].source];
  std::vector<std::pair<u32, ScanPredicate>> dyn;
  for (u32 i = 0; i < n; i++) {
    if (filters[i].kind == RDFGPU_PUSH_UNSUPPORTED) continue;      // `current_predicate_expr().ok()`: unsupported ones are skipped (scan.rs:246-249)
    ScanPredicate p;
    if (filter_to_predicate(filters[i], &p)) dyn.emplace_back(filters[i].var, p);
  }
  // validate now, against the static instructions, so that execute cannot fail on them
  ScanInstructions probe = src.gspo;
  for (auto& d : dyn) and_into_instructions(probe, d.first, d.second);
  src.dynamic = dyn;
  src.dynamic_dirty = true;
}

Plan::~Plan() {
  if (store) (void)hipSetDevice(store->device);
  if (stream) (void)hipStreamSynchronize(stream);
  release_intermediates();
  if (pool_dev) (void)hipFree(pool_dev);
  if (regex_dev) (void)hipFree(regex_dev);
  if (str_consts_dev) (void)hipFree(str_consts_dev);

  if (store && ctx) store->release_context(ctx);
  if (store) store->release();
}

// which scan an n-element scan of counts takes (kernels.hip: one workgroup up to kSmallScanElems elements, rocPRIM's device scan beyond)
static int scan_class(u64 n) { return n <= kSmallScanElems ? KC_SMALL_SCAN : KC_DEVICE_SCAN; }
// Names as rocprofv3 --kernel-trace prints them (prefix up to the argument list).
const char* kernel_class_name(int kc) {
  static const char* const fixed[KC_LDS_JOIN0] = {
      "rdfgpu::locate_kernel", "rdfgpu::scan_count_kernel", "rdfgpu::scan_write_kernel",
      "void rdfgpu::filter_kernel<1>", "void rdfgpu::filter_kernel<2>", "void rdfgpu::filter_kernel<0>",
      "rdfgpu::cross_kernel", "rdfgpu::join_build_kernel", "void rdfgpu::join_probe_kernel<false>",
      "void rdfgpu::join_probe_kernel<true>", "rdfgpu::join_left_unmatched_kernel", "void rdfgpu::nlj_kernel<false>",
      "void rdfgpu::nlj_kernel<true>", "rocprim device scan", "rdfgpu::gjoin_build_kernel", "rdfgpu::gdirect_build_kernel",
      "rdfgpu::minmax_u32_kernel", "rdfgpu::csr_rel_keys_kernel", "rocprim radix sort (CSR rows)",
      "rdfgpu::topk_max_kernel", "rdfgpu::topk_hist_kernel", "rdfgpu::topk_scatter_kernel", "rdfgpu::topk_select_kernel",
      "rdfgpu::topk_write_kernel", "void rdfgpu::filter_kernel<3>", "rdfgpu::regex_verdict_kernel", "rdfgpu::union_kernel",
      "rdfgpu::band_slow_kernel", "rocprim radix sort", "rdfgpu::band_bounds_kernel", "rdfgpu::band_blocks_kernel",
      "rdfgpu::band_decode_kernel", "void rdfgpu::band_mask_kernel", "void rdfgpu::band_emit_kernel", "rdfgpu::band_entries_kernel",
      "rdfgpu::band_desc_kernel", "rdfgpu::band_pt_kernel", "rdfgpu::band_rows_kernel",
      "void rdfgpu::filter_bits_kernel<1>", "void rdfgpu::filter_bits_kernel<2>", "void rdfgpu::filter_bits_kernel<3>", "void rdfgpu::filter_bits_kernel<4>", "rdfgpu::value_verdict_kernel",
      "rdfgpu::value_runs_kernel", "void rdfgpu::run_scan_kernel", "rdfgpu::run_copy_kernel",
      "rdfgpu::oj_probe_kernel", "rdfgpu::oj_count_kernel", "void rdfgpu::oj_write_kernel",
      "void rdfgpu::filter_write_kernel", "rdfgpu::part_keys_kernel", "void rdfgpu::part_join_kernel",
      "rdfgpu::oj_band_records_kernel", "rdfgpu::oj_write_band_kernel", "void rdfgpu::small_scan_kernel",
      "rdfgpu::part_pass (hist + scan + scatter)", "void rdfgpu::stream_join_kernel",
      "rdfgpu::oj_write_band_kernel(rdfgpu::OrderedJoinArgs, rdfgpu::OjBandFuse, rdfgpu::OjInPlace)", "void rdfgpu::semi_build_kernel",
      "void rdfgpu::semi_join_kernel<0, false", "void rdfgpu::semi_join_kernel<0, true", "void rdfgpu::semi_join_kernel<1, false",
      "void rdfgpu::semi_join_kernel<1, true", "void rdfgpu::semi_nested_kernel<false", "void rdfgpu::semi_nested_kernel<true",
      "rdfgpu::agg_groups_kernel", "void rdfgpu::agg_accum_kernel<false>", "void rdfgpu::agg_accum_kernel<true>", "rdfgpu::agg_final_kernel",
      "void rdfgpu::agg_accum_expr_kernel<false>", "void rdfgpu::agg_accum_expr_kernel<true>",
      "rdfgpu::band_row_win_keys_kernel", "rdfgpu::band_row_win_rows_kernel"};
  if (kc < KC_LDS_JOIN0) return fixed[kc];
  static std::string names[192];
  static std::once_flag once;
  std::call_once(once, [] {
    const char* items[2] = {"4", "1"};
    for (int f = 0; f < 4; f++) for (int p = 0; p < 3; p++) for (int w = 0; w < 2; w++) for (int m = 0; m < 4; m++) for (int c = 0; c < 2; c++)
      names[(((f * 3 + p) * 2 + w) * 4 + m) * 2 + c] = "void rdfgpu::lds_join_kernel<" + std::to_string(f) + ", " + std::to_string(p) + ", " +
                                                       items[w] + ", " + std::to_string(m) + ", " + (c ? "true" : "false");   // (a prefix: the key-count argument follows)
  });
  return names[kc - KC_LDS_JOIN0].c_str();
}

template <class F>
void Plan::timed(int kc, u64 fixed_bytes, u64 rows_cap, const u64* rows_dev, u64 bytes_per_row,
                 const u64* out_dev, u64 out_rows, u64 bytes_per_out, F&& launch) {
  metrics.kernels_launched++;
  if (!timing || (timing_focus >= 0 && kc != timing_focus)) { launch(); return; }
  PendingLaunch p{kc, ctx->event(events_used), ctx->event(events_used + 1), fixed_bytes, rows_cap, rows_dev, bytes_per_row, out_dev, out_rows, bytes_per_out};
  events_used += 2;
  RDFGPU_HIP(hipEventRecord(p.start, stream));
  launch();
  RDFGPU_HIP(hipEventRecord(p.stop, stream));
  pending.push_back(p);
}

// After the final sync: event durations + byte counts (device-side cardinalities come from the
// counters mirror copied back with the result count).
void Plan::resolve_timing() {
  for (KernelStat& k : kstats) k = KernelStat{};
  if (!timing) return;
  auto live = [&](const u64* dev, u64 fallback) -> u64 {
    if (!dev) return fallback;
    const u64 v = ctx->counters_host[dev - counters];
    return v < fallback || fallback == 0 ? v : fallback;
  };
  for (const PendingLaunch& p : pending) {
    float ms = 0;
    RDFGPU_HIP(hipEventElapsedTime(&ms, p.start, p.stop));
    KernelStat& k = kstats[p.kc];
    const u64 rows = live(p.rows_dev, p.rows_cap);
    const u64 out = p.out_dev ? ctx->counters_host[p.out_dev - counters] : p.out_rows;
    k.launches++; k.ms += ms; k.rows += rows;
    k.bytes += p.fixed_bytes + rows * p.bytes_per_row + out * p.bytes_per_out;
  }
  pending.clear();
  if (timing_focus < 0) {   // every launch was timed: remember the class that took longest (rdfgpu_plan_enable_kernel_timing(plan, 2))
    double top = 0;
    for (int kc = 0; kc < (int)(sizeof kstats / sizeof kstats[0]); kc++) if (kstats[kc].ms > top) { top = kstats[kc].ms; last_top_kc = kc; }
  }
}

// ------------------------------------------------------------------------------------------------
// execute
// ------------------------------------------------------------------------------------------------
void Plan::release_intermediates() {
  for (void* p : allocs) store->pool.free(p);
  allocs.clear();
}
template <class T> T* Plan::scratch(u64 n) {
  void* p = store->pool.alloc((n ? n : 1) * sizeof(T));
  allocs.push_back(p);
  metrics.device_bytes += (n ? n : 1) * sizeof(T);
  return (T*)p;
}
// Generic (VM) programs of the LDS join live in device memory; staged through the context's pinned slots.
const ExprProgram* Plan::upload_program(const ExprProgram& p) {
  if (progs_used >= ExecContext::kProgSlots) fail(RDFGPU_ERR_UNSUPPORTED, "plan needs more than %u device expression programs", ExecContext::kProgSlots);
  const u32 slot = progs_used++;
  ctx->progs_host[slot] = p;
  RDFGPU_HIP(hipMemcpyAsync(ctx->progs_dev + slot, ctx->progs_host + slot, sizeof(ExprProgram), hipMemcpyHostToDevice, stream));
  return ctx->progs_dev + slot;
}
u64* Plan::new_counter() {
  if (counters_used >= 255) fail(RDFGPU_ERR_UNSUPPORTED, "plan needs more than 255 cardinality counters");   // slot 255: run-time error flags
  return counters + counters_used++;
}
void Plan::read_back(void* host, const void* dev, size_t bytes) {
  RDFGPU_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, stream));
  RDFGPU_HIP(hipStreamSynchronize(stream));
  metrics.host_syncs++;
}

// First execution of a plan over big caller-supplied tables (a batch of query instances): nothing is known yet, so every
// join would be sized exactly and run un-fused — on the full batch that materialises every candidate pair (126 GiB of
// intermediates for 262 144 BSBM Q5 instances).  Instead the plan first runs over the first kPrimeRows rows of each
// bound table: that builds every join table of the store slices (cached per store version) and leaves cardinalities,
// which are extrapolated by the row ratio; the full batch then takes the speculative, fused path at once.  A wrong
// extrapolation is caught like any failed speculation (overflow flag -> exact re-run).
constexpr u64 kPrimeRows = 2048;
void Plan::prime() {
  primed = true;
  if (!allow_speculation || opt.on(RDFGPU_OPT_NO_SPECULATION) || opt.on(RDFGPU_OPT_NO_PRIMING) || opt.on(RDFGPU_OPT_NO_TABLE_CACHE) || opt.on(RDFGPU_OPT_NO_CHAIN_FUSION)) return;
  u64 full = 0;
  for (const BoundTable& b : tables) if (b.bound) full = std::max(full, b.n_rows);
  if (full < 16 * kPrimeRows) return;
  for (const NodeInfo& nd : nodes) if (nd.has_last) return;
  std::vector<u64> saved(tables.size());
  for (size_t i = 0; i < tables.size(); i++) { saved[i] = tables[i].n_rows; tables[i].n_rows = std::min<u64>(tables[i].n_rows, kPrimeRows); }
  priming = true;
  try { execute(); } catch (...) { priming = false; for (size_t i = 0; i < tables.size(); i++) tables[i].n_rows = saved[i]; throw; }
  priming = false;
  for (size_t i = 0; i < tables.size(); i++) tables[i].n_rows = saved[i];
  // operators above a bound table scale with it; pure store subtrees keep their exact history
  std::vector<int> dep(nodes.size(), -1);
  std::function<bool(u32)> depends = [&](u32 i) -> bool {
    if (dep[i] >= 0) return dep[i] != 0;
    const NodeInfo& nd = nodes[i];
    bool d = false;
    if (nd.d.kind == RDFGPU_NODE_TABLE) d = true;
    else if (nd.d.kind != RDFGPU_NODE_DATA_SOURCE) {
      const bool binary = nd.d.kind == RDFGPU_NODE_HASH_JOIN || nd.d.kind == RDFGPU_NODE_CROSS_JOIN || nd.d.kind == RDFGPU_NODE_NESTED_LOOP_JOIN || nd.d.kind == RDFGPU_NODE_UNION;
      if (nd.d.left >= 0) d = depends((u32)nd.d.left);
      if (binary && nd.d.right >= 0) d = depends((u32)nd.d.right) || d;
    }
    dep[i] = d ? 1 : 0;
    return d;
  };
  const u64 ratio = (full + kPrimeRows - 1) / kPrimeRows;
  for (u32 i = 0; i < nodes.size(); i++) {
    NodeInfo& nd = nodes[i];
    if (nd.has_last && depends(i)) { nd.last_rows = nd.last_rows * ratio + 1024; nd.last_scaled = true; }
  }
}

// The measurements this execution's band joins left in the counters -> NodeInfo::band.  true: one of them speculated wrongly.
bool Plan::record_band_history() {
  bool missed = false;
  for (const BandFeedback& f : band_feedback) {
    BandHistory& h = f.node->band;
    h.ran = true; h.blocks = f.known_blocks ? f.known_blocks : ctx->counters_host[f.blocks];
    h.slow_rows = ctx->counters_host[f.slow_rows] & 0xFFFFFFFFull; h.run_stats = ctx->counters_host[f.run_stats];
    if (f.slow_skipped && h.slow_rows) missed = true;   // rows with non-integer operands, and their pass was not launched
    if (f.multi_rows >= 0) h.multi_rows = ctx->counters_host[f.multi_rows] & 0xFFFFFFFFull;
    if (f.multi_rows >= 0 && f.in_place && h.multi_rows) missed = true;   // a key with 2+ table rows: the in-place records held one of them
  }
  return missed;
}

void Plan::execute() {
  if (!primed && !priming) prime();
  store->activate();
  std::shared_lock<std::shared_mutex> lock(store->mu);   // a plan holds the snapshot while it runs (snapshot.rs:35-37)
  RDFGPU_HIP(hipStreamSynchronize(stream));
  release_intermediates();
  // the pool keeps what an execution hands back for the next one — bounded by twice what the previous executions (this plan's, or any plan's of the store) used
  // (+ 1 GiB): the giant blocks of a one-off exact run go back to the device instead of staying cached for ever
  store->pool.trim_to(2 * std::max(std::max(scratch_hist[0], scratch_hist[1]), std::max(store->scratch_recent[0].load(), store->scratch_recent[1].load())) + (1ull << 30));
  held = store->gen;         // ... and the generation it read until its next execute: the result may be zero-copy slices of it
  metrics = rdfgpu_metrics{};
  const u64 mallocs0 = store->pool.mallocs() + store->table_pool.mallocs();
  const double malloc_ms0 = store->pool.malloc_ms() + store->table_pool.malloc_ms();
  counters_used = 0;
  progs_used = 0;
  arg_slots_used = 0;
  events_used = 2;   // events 0/1 bracket the whole execute
  pending.clear();
  host_valid = false; cursor = 0; executed = false;
  agg_out.clear();
  const hipEvent_t ev_start = ctx->event(0), ev_stop = ctx->event(1);
  RDFGPU_HIP(hipEventRecord(ev_start, stream));
  RDFGPU_HIP(hipMemsetAsync(counters, 0, 256 * sizeof(u64), stream));

  spec_checks.clear();
  pending_oj.active = false;
  band_feedback.clear();
  memo.assign(nodes.size(), DevTable{}); memo_valid.assign(nodes.size(), 0);
  speculative = allow_speculation && !opt.on(RDFGPU_OPT_NO_SPECULATION);

  // Dynamic filters (scan.rs:217-261): the effective instructions of a leaf = its static ones AND the filters' current
  // predicates, index re-chosen for them; derived when the filters changed, the ranges located again.
  {
    bool changed = false;
    for (SourceInfo& s : sources) {
      if (!s.dynamic_dirty) continue;
      ScanInstructions eff = s.gspo;
      for (auto& dflt : s.dynamic) and_into_instructions(eff, dflt.first, dflt.second);
      derive_source(s, eff);
      s.dynamic_dirty = false;
      changed = true;
    }
    if (changed) {
      lock.unlock();
      upload_pool();
      lock.lock();
      located_version = ~0ull;
      for (NodeInfo& nd : nodes) { nd.has_last = false; nd.last_rows = 0; }
      speculative = false;
    }
  }
  // K1: locate every data source's range in one launch, one host round trip for all of them.  The ranges
  // depend only on the plan's constants and the store's content: a re-execution on an unchanged store
  // reuses them (no launch, no sync).
  if (!sources.empty() && located_version == store->version.load()) {
    for (const SourceInfo& s : sources) metrics.input_rows += s.hi - s.lo;
  } else if (!sources.empty()) {
    located_version = store->version.load();
    LocateJob* jobs = static_cast<LocateJob*>(ctx->jobs_host);
    for (size_t i = 0; i < sources.size(); i++) {
      const SourceInfo& s = sources[i];
      const Permutation& ix = store->idx[s.components];
      LocateJob& j = jobs[i];
      for (int k = 0; k < 4; k++) j.col[k] = ix.col[k];
      j.n = ix.n;
      j.n_levels = s.prune.n_levels;
      for (int k = 0; k < 4; k++) { j.from[k] = s.prune.from[k]; j.to[k] = s.prune.to[k]; }
    }
    LocateJob* jobs_dev = static_cast<LocateJob*>(ctx->jobs_dev);
    RDFGPU_HIP(hipMemcpyAsync(jobs_dev, jobs, sources.size() * sizeof(LocateJob), hipMemcpyHostToDevice, stream));
    timed(KC_LOCATE, 0, sources.size(), nullptr, 0, nullptr, 0, 0, [&] { launch_locate(jobs_dev, (u32)sources.size(), ctx->lohi_dev, stream); });
    read_back(ctx->lohi_host, ctx->lohi_dev, sources.size() * kLocateWords * sizeof(u64));
    for (size_t i = 0; i < sources.size(); i++) {
      const u64* w = ctx->lohi_host + kLocateWords * i;
      SourceInfo& s = sources[i];
      s.lo = w[0]; s.hi = w[1]; s.sorted_level = (u32)(w[2] >> 32); s.key_min = (u32)w[2]; s.key_max = (u32)w[3];
      metrics.input_rows += s.hi - s.lo;
    }
  }

  result = exec_node(root);
  flush_pending_oj();
  // one copy brings back every device-side cardinality (the result's and, for timing, the others')
  RDFGPU_HIP(hipMemcpyAsync(ctx->counters_host, counters, 256 * sizeof(u64), hipMemcpyDeviceToHost, stream));
  RDFGPU_HIP(hipEventRecord(ev_stop, stream));
  RDFGPU_HIP(hipStreamSynchronize(stream)); metrics.host_syncs++;
  RDFGPU_HIP(hipGetLastError());
  if (const u32 rt = (u32)(ctx->counters_host[255] & 0xFFFFFFFFull)) {   // a row asked for something that is refused loudly, not answered differently
    if (rt & 1u) fail(RDFGPU_ERR_UNSUPPORTED, "REGEX with \\d \\w \\s or \\b over a string with non-ASCII characters needs the regex crate's Unicode tables (not restated)");
    if (rt & 8u) fail(RDFGPU_ERR_UNSUPPORTED, "a numeric CAST met a simple literal: the lexical forms of numbers are not parsed on the device");
    if (rt & 4u) fail(RDFGPU_ERR_UNSUPPORTED, "a string expression met what the device does not restate: UCASE / LCASE of a string with non-ASCII characters (Unicode case tables), "
                                               "a float / double / decimal SUBSTR position, or a comparison with a string that has no bytes on the device");
    fail(RDFGPU_ERR_UNSUPPORTED, "REGEX with a per-row pattern: a row's pattern literal was not announced in the plan's pattern table");
  }
  // speculative joins: did the band joins take the right route, did every output fit the size taken from the previous run?
  bool spec_failed = record_band_history();
  for (const SpecCheck& c : spec_checks) {
    if ((ctx->counters_host[c.counter + 1] & 0xFFFFFFFFull) != 0) spec_failed = true;
    else { c.node->last_rows = ctx->counters_host[c.counter]; c.node->has_last = true; c.node->last_scaled = false; }
  }
  if (spec_failed) {   // rare: run again with exact sizes (one sync per join), then speculate again next time
    metrics.host_syncs++;
    lock.unlock();
    allow_speculation = false;
    try { execute(); } catch (...) { allow_speculation = true; throw; }
    allow_speculation = true;
    metrics.exact_reruns = 1;
    return;
  }
  result_rows = result.n_dev ? ctx->counters_host[result.n_dev - counters] : result.cap;
  if (result_rows > result.cap) result_rows = result.cap;
  float ms = 0;
  RDFGPU_HIP(hipEventElapsedTime(&ms, ev_start, ev_stop));
  metrics.elapsed_compute_ms = ms;
  metrics.output_rows = result_rows;
  metrics.device_mallocs = (u32)(store->pool.mallocs() + store->table_pool.mallocs() - mallocs0);
  metrics.device_malloc_ms = store->pool.malloc_ms() + store->table_pool.malloc_ms() - malloc_ms0;
  resolve_timing();
  executed = true;
  scratch_hist[1] = scratch_hist[0]; scratch_hist[0] = metrics.device_bytes;
  store->scratch_recent[1] = store->scratch_recent[0].load(); store->scratch_recent[0] = metrics.device_bytes;
}

DevTable Plan::exec_node(u32 idx) {
  if (memo_valid[idx]) return memo[idx];   // a node runs once per execution, however many operators consume it
  NodeInfo& nd = nodes[idx];
  DevTable t;
  switch (nd.d.kind) {
    case RDFGPU_NODE_DATA_SOURCE: t = exec_source(nd); break;
    case RDFGPU_NODE_FILTER: t = exec_filter(nd); break;
    case RDFGPU_NODE_PROJECTION: {
      const DevTable in = exec_node((u32)nd.d.left);
      t.n_cols = nd.n_proj; t.cap = in.cap; t.n_dev = in.n_dev;
      for (u32 c = 0; c < nd.n_proj; c++) t.cols[c] = in.cols[nd.proj[c]];
      break;
    }
    case RDFGPU_NODE_HASH_JOIN: case RDFGPU_NODE_CROSS_JOIN: case RDFGPU_NODE_NESTED_LOOP_JOIN:
      // semi / anti joins leave before anything of exec_join (chain planning, filter fusion, side choice) sees them
      t = nd.d.join_type == RDFGPU_JOIN_LEFT_SEMI || nd.d.join_type == RDFGPU_JOIN_LEFT_ANTI ? exec_semi_join(nd) : exec_join(nd);
      break;
    case RDFGPU_NODE_TOPK: t = exec_topk(nd); break;
    case RDFGPU_NODE_AGGREGATE: t = exec_aggregate(nd); break;
    case RDFGPU_NODE_CLOSURE: {
      const DevTable in = exec_node((u32)nd.d.left);
      const u64 n = in.n_dev && in.cap ? read_back<u64>(in.n_dev) : in.cap;
      u32* out[3] = {nullptr, nullptr, nullptr};
      ClosureStats cs;
      const u64 rows = closure_exec(in.cols[0], in.cols[1], in.cols[2], n, nd.d.join_type == 1, stream, [&](u64 m) { return scratch<u32>(m); }, out, &cs);
      metrics.host_syncs += 4 + 3 * cs.iterations;
      t.n_cols = nd.n_proj; t.cap = rows; t.n_dev = nullptr;
      for (u32 c = 0; c < nd.n_proj; c++) t.cols[c] = out[nd.proj[c]];
      break;
    }
    case RDFGPU_NODE_UNION: {
      const DevTable L = exec_node((u32)nd.d.left), R = exec_node((u32)nd.d.right);
      t.n_cols = nd.n_proj;
      const u64 cap = L.cap + R.cap;
      if (cap >= 0xFFFFFFF0ull) fail(RDFGPU_ERR_UNSUPPORTED, "UnionExec of %llu rows", (unsigned long long)cap);
      if (cap == 0) { t.cap = 0; break; }
      UnionArgs a{};
      a.n_cols = nd.n_proj;
      for (u32 c = 0; c < nd.n_proj; c++) {
        a.left[c] = L.cap ? L.cols[nd.proj[c]] : nullptr; a.right[c] = R.cap ? R.cols[nd.proj[c]] : nullptr;
        a.out[c] = scratch<u32>(cap); t.cols[c] = a.out[c];
      }
      a.n_left_dev = L.n_dev; a.n_left_cap = L.cap; a.n_right_dev = R.n_dev; a.n_right_cap = R.cap;
      const bool dyn = L.n_dev || R.n_dev;
      a.n_out_dev = dyn ? new_counter() : nullptr;
      // bytes: every projected cell read once and written once
      timed(KC_UNION, R.n_dev ? 0 : 8ull * nd.n_proj * R.cap, L.cap, L.n_dev, 8ull * nd.n_proj, nullptr, 0, 0, [&] { launch_union(a, stream); });
      t.cap = cap; t.n_dev = a.n_out_dev;
      break;
    }
    case RDFGPU_NODE_TABLE: {
      const BoundTable& b = tables[nd.d.table_slot];
      if (!b.bound) fail(RDFGPU_ERR_INVALID, "table slot %u is not bound", nd.d.table_slot);
      if (b.cols.size() != nd.d.table_cols) fail(RDFGPU_ERR_INVALID, "table slot %u: %zu columns bound, node declares %u", nd.d.table_slot, b.cols.size(), nd.d.table_cols);
      t.n_cols = nd.d.table_cols; t.cap = b.n_rows;
      for (u32 c = 0; c < t.n_cols; c++) t.cols[c] = b.cols[c];
      break;
    }
    default: fail(RDFGPU_ERR_INVALID, "unknown node kind");
  }
  if (idx != root) metrics.intermediate_rows += t.cap;   // upper bound when the exact count stays on the device
  if (!(pending_chain && pending_chain->consumed)) { memo[idx] = t; memo_valid[idx] = 1; }   // (a fused chain's output belongs to its top node)
  return t;
}

// DataSourceExec: a prefix-bound pattern is a zero-copy slice of the permutation (like the
// reference's untouched row-group slices, scan.rs:146-170); residual predicates go through K2.
DevTable Plan::exec_source(NodeInfo& nd) {
  SourceInfo& s = sources[nd.source];
  const Permutation& ix = store->idx[s.components];
  DevTable t;
  t.n_cols = s.n_out;
  const u64 n = s.hi - s.lo;
  if (n == 0) { t.cap = 0; return t; }
  if (!s.has_residual) {
    for (u32 c = 0; c < s.n_out; c++) t.cols[c] = ix.col[s.out_level[c]] + s.lo;
    t.cap = n;
    t.stable_id = (u64)nd.source + 1;   // a pure slice of the store: identical on every execution until the store changes
    for (u32 c = 0; c < s.n_out; c++) if (s.out_level[c] == s.sorted_level && t.sorted_col < 0) { t.sorted_col = (int)c; t.key_min = s.key_min; t.key_max = s.key_max; }
    return t;
  }
  ScanJob job{};
  for (int k = 0; k < 4; k++) {
    job.col[k] = ix.col[k] + s.lo;
    const ScanPredicate& p = s.ix.in[k].pred;
    ScanLevelPred& q = job.pred[k];
    q.kind = (s.prune.dropped_mask & (1u << k)) ? (u32)RDFGPU_PRED_NONE : p.kind;
    if (q.kind == RDFGPU_PRED_BETWEEN) { q.a = p.from; q.b = p.to; }
    else if (q.kind == RDFGPU_PRED_IN) { q.b = (u32)p.ids.size(); q.ids = pool_dev + p.from; }
    else if (q.kind == RDFGPU_PRED_EQUAL_TO) {
      int other = -1;
      for (int l = 0; l < 4; l++) if (s.ix.in[l].kind == RDFGPU_SCAN && s.ix.in[l].var == p.equal_to) { other = l; break; }
      if (other < 0) q.kind = RDFGPU_PRED_NONE;   // `position(..)?` => no mask (scan.rs:310-313)
      else q.a = (u32)other;
    }
  }
  job.n = n;
  job.n_out = s.n_out;
  for (u32 c = 0; c < s.n_out; c++) job.out_level[c] = s.out_level[c];
  const u64 n_blocks = (n + kScanTile - 1) / kScanTile;
  u32* counts = scratch<u32>(n_blocks + 1);
  u32* offs = scratch<u32>(n_blocks + 1);
  const size_t tb = scan_temp_bytes(n_blocks + 1);
  void* temp = scratch<u8>(tb);
  RDFGPU_HIP(hipMemsetAsync(counts + n_blocks, 0, 4, stream));
  u32 n_pred_cols = 0;   // columns the residual predicates read
  for (int k = 0; k < 4; k++) n_pred_cols += job.pred[k].kind != RDFGPU_PRED_NONE && job.pred[k].kind != RDFGPU_PRED_FALSE;
  timed(KC_SCAN_COUNT, 0, n, nullptr, 4ull * n_pred_cols, nullptr, 0, 0, [&] { launch_scan_count(job, counts, stream); });
  timed(scan_class(n_blocks + 1), 0, n_blocks + 1, nullptr, 8, nullptr, 0, 0, [&] { exclusive_scan_u32(counts, offs, n_blocks + 1, temp, tb, stream); });
  const u32 total = read_back<u32>(offs + n_blocks);
  t.cap = total;
  if (total == 0) return t;
  for (u32 c = 0; c < s.n_out; c++) { job.out[c] = scratch<u32>(total); t.cols[c] = job.out[c]; }
  // scan+filter+compact: 4·c_r·N + 4·c_w·σN, c_r = predicate ∪ output columns (upper bound: both)
  if (s.n_out) timed(KC_SCAN_WRITE, 0, n, nullptr, 4ull * n_pred_cols, nullptr, total, 8ull * s.n_out, [&] { launch_scan_write(job, offs, stream); });
  return t;
}

DevTable Plan::exec_filter(NodeInfo& nd) {
  const DevTable in = exec_node((u32)nd.d.left);
  return apply_filter(nd, in);
}

DevTable Plan::apply_filter(NodeInfo& nd, const DevTable& in) {
  DevTable t;
  t.n_cols = nd.n_proj;
  if (in.cap == 0) { t.cap = 0; return t; }
  if (nd.prog.n == 0) {   // no predicate: a projection
    t.cap = in.cap; t.n_dev = in.n_dev;
    for (u32 c = 0; c < nd.n_proj; c++) t.cols[c] = in.cols[nd.proj[c]];
    return t;
  }
  FilterArgs a{};
  for (u32 c = 0; c < in.n_cols; c++) a.in[c] = in.cols[c];
  a.n_in_cols = in.n_cols; a.n_out_cols = nd.n_proj;
  for (u32 c = 0; c < nd.n_proj; c++) { a.proj[c] = nd.proj[c]; a.out[c] = scratch<u32>(in.cap); t.cols[c] = a.out[c]; }
  a.n_in_dev = in.n_dev; a.n_in_cap = in.cap;
  a.n_out_dev = new_counter();
  a.tt = typed_table();
  a.prog = nd.prog;
  int shape = nd.shape;
  if (shape == 3) {
    // per-distinct-term verdicts: worth a pass over the dictionary when the table has at least a quarter as many rows
    // as there are ids (or the verdicts exist already); the table lives on the store, keyed by the predicate
    const rdfgpu_expr_node& e = nd.prog.nodes[2];
    const rdfgpu_regex& rx = regex_text[e.u];
    std::string key(1, (char)e.op);
    key.append(reinterpret_cast<const char*>(&e.lo), sizeof e.lo);
    key.append(rx.flags ? std::string(rx.flags, rx.flags_len) : std::string()).push_back('\0');
    key.append(rx.pattern ? std::string(rx.pattern, rx.pattern_len) : std::string());
    const u64 n_ids = std::min<u64>(store->n_ids, store->n_str_ids);
    unsigned char* verdict = nullptr;
    if (!opt.on(RDFGPU_OPT_NO_STRING_VERDICTS) && n_ids > 0) {
      std::unique_lock<std::mutex> building(store->slice_build_mu);
      { std::lock_guard<std::mutex> l(store->slice_mu); auto it = store->string_verdicts.find(key); if (it != store->string_verdicts.end()) verdict = it->second; }
      if (!verdict && in.cap * 4 >= n_ids) {
        // bounded cache: a workload of ever-changing patterns must not pile up one table per pattern — beyond 64
        // entries the table is this execution's scratch
        bool cache_it;
        { std::lock_guard<std::mutex> l(store->slice_mu); cache_it = store->string_verdicts.size() < 64; }
        if (cache_it) RDFGPU_HIP(hipMalloc((void**)&verdict, n_ids)); else verdict = scratch<unsigned char>(n_ids);
        const int64_t lang = e.op == RDFGPU_EX_REGEX ? -1 : (e.lo < 0 ? 0 : e.lo);
        timed(KC_REGEX_VERDICTS, 0, n_ids, nullptr, 16 + 8 + 1, nullptr, 0, 0, [&] { TypedTable vt = a.tt; vt.rt_error = nullptr;   // a verdict pass covers the whole dictionary: what it cannot answer is verdict 3, an error only for a row that reads it
                                                                                               launch_regex_verdicts(regex_dev + e.u, vt, lang, verdict, n_ids, stream); });
        if (cache_it) {
          RDFGPU_HIP(hipStreamSynchronize(stream)); metrics.host_syncs++;   // complete before other plans may see it
          std::lock_guard<std::mutex> l(store->slice_mu);
          store->string_verdicts[key] = verdict;
        }
      }
    }
    if (verdict) { a.verdict = verdict; a.n_verdict = n_ids; } else shape = 0;
  }
  // a typed comparison on the sorted column of a big store slice with few distinct ids: the qualifying runs are copied, the
  // predicate column is not streamed at all
  if (shape == 2 && !opt.on(RDFGPU_OPT_NO_VALUE_VERDICTS) && !opt.on(RDFGPU_OPT_NO_RUN_COPY) && in.sorted_col >= 0 && (u32)in.sorted_col == nd.prog.nodes[0].u &&
      in.key_max >= in.key_min && !in.n_dev && in.cap >= (1ull << 20) && in.cap < (1ull << 32) && nd.n_proj <= 2) {
    const u64 span = (u64)in.key_max - in.key_min + 1;
    if (span <= kRunCopyMaxIds && span * 1024 <= in.cap) {
      a.value_min = in.key_min; a.value_span = span;
      a.stream_bits = reinterpret_cast<unsigned short*>(scratch<u32>(1)); a.stream_counts = scratch<u32>(1); a.stream_offs = a.stream_counts;   // (the argument block wants them non-null)
      // Where every id's run starts is a function of the slice alone: kept with the slice's other tables per store version (the searches
      // that find them are five dependent HBM round trips per id: 10 of the operator's 68 us); with the table at hand the comparison of
      // every id is answered in the scan kernel — one launch plans the copy.
      const u32* pcol = in.cols[in.sorted_col];
      const bool cacheable = in.stable_id != 0 && !opt.on(RDFGPU_OPT_NO_TABLE_CACHE);
      u32* cached_lo = nullptr;
      SliceTable* vst = nullptr;
      std::unique_lock<std::mutex> building(store->slice_build_mu, std::defer_lock);
      if (cacheable) {
        SliceKey sk; sk.n_keys = 1; sk.rows = in.cap; sk.key[0] = pcol;
        vst = store->slice_table(sk);
        building.lock();
        for (const auto& v : vst->value_starts) if (v.first == in.key_min && v.span == span) cached_lo = v.lo;
      }
      const bool own = cacheable && !cached_lo && vst->value_starts.size() < 4;
      u32* run_lo = cached_lo ? cached_lo : own ? store->table_alloc<u32>(span + 1) : scratch<u32>(span + 1);   // (one entry past the last id)
      RunCopyBuffers b{run_lo, scratch<u32>(span), scratch<u32>(span + 1), scratch<u32>(span + 1), scratch<u32>(span + 1), scratch<u32>(1)};
      if (!cached_lo) timed(KC_VALUE_RUNS, 0, span, nullptr, 16, nullptr, 0, 0, [&] { launch_value_runs(a, b, stream); });
      // (one launch for scan + copy — 2048 workgroups that each scan the run lengths in LDS and copy an equal share — was tried: 68 us
      //  against 6 + 51: the big chunks do not hide their memory latency the way 16 K small workgroups do)
      timed(KC_RUN_SCAN, 0, span, nullptr, cached_lo ? 16 + 8 : 8, nullptr, 0, 0, [&] { launch_run_scan(a, b, cached_lo != nullptr, stream); });
      if (own) {   // publish only when complete
        RDFGPU_HIP(hipStreamSynchronize(stream)); metrics.host_syncs++; metrics.tables_built++;
        vst->value_starts.push_back(SliceTable::ValueStarts{in.key_min, span, run_lo});
      }
      if (building.owns_lock()) building.unlock();
      timed(KC_RUN_COPY, 0, 0, nullptr, 0, a.n_out_dev, 0, 8ull * nd.n_proj, [&] { launch_run_copy(a, b, stream); });
      t.cap = in.cap; t.n_dev = a.n_out_dev;
      return t;
    }
  }
  // FilterExec bytes: 4·c_r·N + t·N + 4·c_w·σN with t = 9 B per typed gather (tag + i64); shape 3: t = 1 B
  if (filter_streams(a, shape)) {   // two passes without atomics: verdict bits + tile counts, device scan, ordered write
    const u64 tiles = filter_stream_tiles(a);
    a.stream_bits = scratch<unsigned short>(tiles * 256);
    a.stream_counts = scratch<u32>(tiles + 1); a.stream_offs = scratch<u32>(tiles + 1);
    a.stream_temp_bytes = scan_temp_bytes(tiles + 1);
    a.stream_temp = scratch<unsigned char>(a.stream_temp_bytes);
    RDFGPU_HIP(hipMemsetAsync(a.stream_counts + tiles, 0, sizeof(u32), stream));
    // compulsory bytes: pass 1 streams the predicate column (its typed-value gathers hit a table that is cache-resident or
    // not: not counted) and writes one bit per row; pass 2 reads the bits and the output columns and writes the survivors
    // a typed comparison over the sorted column of a store slice: answered once per id of the slice's id range when that
    // range is small next to the rows (a GPOS slice of one predicate: its objects), then one bit per row
    if (shape == 2 && !opt.on(RDFGPU_OPT_NO_VALUE_VERDICTS) && in.sorted_col >= 0 && (u32)in.sorted_col == nd.prog.nodes[0].u && in.key_max >= in.key_min) {
      const u64 span = (u64)in.key_max - in.key_min + 1;
      if (span * 4 <= in.cap) {
        u32* words = scratch<u32>(((span + 63) / 64) * 2);
        a.value_bits = words; a.value_min = in.key_min; a.value_span = span;
        timed(KC_VALUE_VERDICTS, 0, span, nullptr, 16, nullptr, 0, 0, [&] { launch_value_verdicts(a, stream); });
        shape = 4;
      }
    }
    const int kc1 = shape == 1 ? KC_FILTER_BITS_ID : shape == 2 ? KC_FILTER_BITS_TV : shape == 4 ? KC_FILTER_BITS_VALUE : KC_FILTER_BITS_VERDICT;
    timed(kc1, tiles * 4, in.cap, in.n_dev, 4, nullptr, 0, 0, [&] { launch_filter_bits(a, shape, stream); });
    timed(scan_class(tiles + 1), 0, tiles + 1, nullptr, 8, nullptr, 0, 0, [&] { exclusive_scan_u32(a.stream_counts, a.stream_offs, tiles + 1, a.stream_temp, a.stream_temp_bytes, stream); });
    timed(KC_FILTER_WRITE, tiles * 8, in.cap, in.n_dev, 4ull * nd.n_proj, a.n_out_dev, 0, 4ull * nd.n_proj, [&] { launch_filter_write(a, shape, stream); });
    t.cap = in.cap; t.n_dev = a.n_out_dev;
    return t;
  }
  const int kc = shape == 1 ? KC_FILTER_ID : shape == 2 ? KC_FILTER_TV : shape == 3 ? KC_FILTER_VERDICT : KC_FILTER_VM;
  timed(kc, 0, in.cap, in.n_dev, shape == 3 ? 4ull * nd.n_cols_read + 1 : 4ull * nd.n_cols_read + 9ull * nd.n_enc_tv, a.n_out_dev, 0, 4ull * nd.n_proj,
        [&] { launch_filter(a, shape, stream); });
  t.cap = in.cap; t.n_dev = a.n_out_dev;
  return t;
}

static u32 pow2_at_least(u64 v) { u64 p = 1024; while (p < v && p < (1ull << 31)) p <<= 1; return (u32)p; }

// DISTINCT + ORDER BY keys LIMIT k (per group): counting sort of row ids by group, one wave per group selecting the k
// smallest distinct key tuples, compaction by offsets.  Two host round trips (largest group id; final count + the
// "unsupported kind in a SORT_BY_TERM column" flag): this operator ends a query, it is not inside the join pipeline.
DevTable Plan::exec_topk(NodeInfo& nd) {
  const DevTable in = exec_node((u32)nd.d.left);
  DevTable t;
  t.n_cols = nd.n_proj;
  if (in.cap == 0) { t.cap = 0; return t; }
  if (in.cap >= (1ull << 32)) fail(RDFGPU_ERR_UNSUPPORTED, "TopK over %llu rows", (unsigned long long)in.cap);
  TopkArgs a{};
  for (u32 c = 0; c < in.n_cols; c++) a.in[c] = in.cols[c];
  a.n_in_dev = in.n_dev; a.n_in_cap = in.cap;
  a.has_group = nd.d.table_slot != 0; a.group_col = a.has_group ? nd.d.table_slot - 1 : 0;
  a.n_keys = nd.d.n_keys;
  for (u32 k = 0; k < a.n_keys; k++) { a.key_col[k] = nd.d.left_keys[k]; a.key_by_term[k] = nd.d.right_keys[k]; }   // RDFGPU_SORT_BY_*
  a.k = nd.d.table_cols;
  a.tt = typed_table();
  u64* n_out = new_counter();
  u32* flags = reinterpret_cast<u32*>(new_counter());   // {largest group id, unsupported-kind flag}
  a.n_out_dev = n_out; a.bad = flags + 1;
  a.n_groups = 1;
  if (a.has_group) {
    timed(KC_TOPK_MAX, 0, in.cap, in.n_dev, 4, nullptr, 0, 0, [&] { launch_topk_max(a.in[a.group_col], in.n_dev, in.cap, flags, stream); });
    const u32 mx = read_back<u32>(flags);
    if (mx >= (1u << 24)) fail(RDFGPU_ERR_UNSUPPORTED, "TopK: group ids up to %u (dense ids below 2^24 expected)", mx);
    a.n_groups = mx + 1;
  }
  const u64 ng = a.n_groups;
  a.counts = scratch<u32>(ng + 1); a.offsets = scratch<u32>(ng + 1); a.cursor = scratch<u32>(ng);
  a.perm = scratch<u32>(in.cap); a.picked = scratch<u32>(ng * a.k);
  a.out_counts = scratch<u32>(ng + 1); a.out_offsets = scratch<u32>(ng + 1);
  const u64 out_cap = std::min<u64>(in.cap, ng * a.k);
  a.n_out_cols = nd.n_proj;
  for (u32 c = 0; c < nd.n_proj; c++) { a.proj[c] = nd.proj[c]; a.out[c] = scratch<u32>(out_cap); t.cols[c] = a.out[c]; }
  RDFGPU_HIP(hipMemsetAsync(a.counts, 0, (ng + 1) * sizeof(u32), stream));
  RDFGPU_HIP(hipMemsetAsync(a.out_counts, 0, (ng + 1) * sizeof(u32), stream));
  const size_t tb = scan_temp_bytes(ng + 1);
  void* temp = scratch<unsigned char>(tb);
  u32 key_bytes = 4 * a.n_keys;
  for (u32 k = 0; k < a.n_keys; k++) key_bytes += a.key_by_term[k] ? 16 : 0;
  timed(KC_TOPK_HIST, 0, in.cap, in.n_dev, 4, nullptr, 0, 0, [&] { launch_topk_hist(a, stream); });
  exclusive_scan_u32(a.counts, a.offsets, ng + 1, temp, tb, stream);
  RDFGPU_HIP(hipMemcpyAsync(a.cursor, a.offsets, ng * sizeof(u32), hipMemcpyDeviceToDevice, stream));
  timed(KC_TOPK_SCATTER, 0, in.cap, in.n_dev, 8, nullptr, 0, 0, [&] { launch_topk_scatter(a, stream); });
  timed(KC_TOPK_SELECT, 0, in.cap, in.n_dev, (4ull + key_bytes) * a.k, nullptr, 0, 0, [&] { launch_topk_select(a, stream); });
  exclusive_scan_u32(a.out_counts, a.out_offsets, ng + 1, temp, tb, stream);
  timed(KC_TOPK_WRITE, 0, 0, nullptr, 0, n_out, 0, 8ull * nd.n_proj, [&] { launch_topk_write(a, stream); });
  const u32 i0 = (u32)(n_out - counters);
  read_back(ctx->counters_host + i0, counters + i0, 2 * sizeof(u64));
  if ((ctx->counters_host[i0 + 1] >> 32) != 0) fail(RDFGPU_ERR_UNSUPPORTED, "TopK: SORT_BY_TERM over a column that is not all strings / IRIs / blank nodes");
  t.cap = std::min<u64>(out_cap, ctx->counters_host[i0]);
  t.n_dev = n_out;
  return t;
}

// HashJoinExec / NestedLoopJoinExec with JoinType::LeftSemi / LeftAnti (semi_join.hip).  The output has at most as many rows as the
// left input: a table of cap L.cap whose count stays on the device, like a FilterExec's — no speculation, no overflow, no re-run.
// The right input (the existence side) is the table, the left rows probe it: a set built by every workgroup in LDS when the right
// input is small, else one set in HBM built in this execution; a NestedLoopJoinExec streams the right rows through LDS.
DevTable Plan::exec_semi_join(NodeInfo& nd) {
  const bool anti = nd.d.join_type == RDFGPU_JOIN_LEFT_ANTI;
  // the inputs are sub-plans of their own (a chain pending above must not leak into them)
  ChainRequest* const for_this_join = pending_chain;
  pending_chain = nullptr;
  const DevTable L = exec_node((u32)nd.d.left);
  const DevTable R = exec_node((u32)nd.d.right);
  pending_chain = for_this_join;
  flush_pending_oj();   // a held-back ordered-join write must have happened before either input is read
  DevTable t;
  t.n_cols = nd.n_proj;
  if (L.cap == 0) { t.cap = 0; return t; }
  const bool hash = nd.d.kind == RDFGPU_NODE_HASH_JOIN;
  const bool right_empty = R.cap == 0;
  // the verdict is the same for every left row when the right input is empty (nothing matches), or for a nested-loop join without a
  // filter over a right input whose row count the host knows: the left rows, projected, without a launch
  if (right_empty || (!hash && nd.prog.n == 0 && R.n_dev == nullptr)) {
    const bool keep_all = right_empty ? anti : !anti;
    if (!keep_all) { t.cap = 0; return t; }
    t.cap = L.cap; t.n_dev = L.n_dev;
    for (u32 c = 0; c < nd.n_proj; c++) t.cols[c] = L.cols[nd.proj[c]];
    return t;
  }
  if (L.cap >= 0xFFFFFFF0ull || R.cap >= 0x7FFFFFFFull) fail(RDFGPU_ERR_UNSUPPORTED, "semi / anti join of %llu x %llu rows", (unsigned long long)L.cap, (unsigned long long)R.cap);
  SemiJoinArgs a{};
  for (u32 c = 0; c < L.n_cols; c++) a.cols[c] = L.cols[c];
  for (u32 c = 0; c < R.n_cols; c++) a.cols[L.n_cols + c] = R.cols[c];
  a.n_left_cols = L.n_cols; a.n_right_cols = R.n_cols;
  a.n_out_cols = nd.n_proj;
  for (u32 c = 0; c < nd.n_proj; c++) { a.proj[c] = nd.proj[c]; a.out[c] = scratch<u32>(L.cap); t.cols[c] = a.out[c]; }
  a.n_keys = hash ? nd.d.n_keys : 0;
  for (u32 k = 0; k < a.n_keys; k++) { a.left_key[k] = L.cols[nd.d.left_keys[k]]; a.right_key[k] = R.cols[nd.d.right_keys[k]]; }
  a.n_left_dev = L.n_dev; a.n_left_cap = L.cap; a.n_right_dev = R.n_dev; a.n_right_cap = R.cap;
  a.tt = typed_table();
  a.n_out_dev = new_counter();
  int filter = kSemiNoFilter;
  u32 left_fcols = 0;   // distinct left columns the filter reads (compulsory bytes)
  if (nd.prog.n) {
    bool used[2 * kMaxCols] = {};
    for (u32 i = 0; i < nd.prog.n; i++) if (nd.prog.nodes[i].op == RDFGPU_EX_COLUMN) used[nd.prog.nodes[i].u] = true;
    for (u32 c = 0; c < L.n_cols; c++) left_fcols += used[c];
    if (nd.shape == 2) {   // `col <ID_EQ | ID_NEQ> col`
      filter = kSemiIdPair;
      a.idp = IdPairFilter{nd.prog.nodes[0].u, nd.prog.nodes[1].u, nd.prog.nodes[2].op == RDFGPU_EX_ID_EQ ? 1u : 0u};
    } else {
      filter = kSemiVm;
      a.prog = upload_program(nd.prog);
    }
  }
  int form = kSemiNested;
  u64 build_bytes = 0;
  if (hash) {
    const u64 lds_max = std::min<u64>(opt.v[RDFGPU_OPT_LDS_MAX_BUILD], kSemiLdsMaxBuild);
    form = R.cap <= lds_max && !opt.on(RDFGPU_OPT_NO_SEMI_LDS) ? kSemiLds : kSemiHbm;
    u64 slots = 64;
    while (slots < 2 * R.cap) slots <<= 1;
    a.tbl_mask = (u32)(slots - 1);
    // build half: the right keys read once, one 8-byte slot written per row
    build_bytes = (4ull * a.n_keys + 8) * R.cap;
    if (form == kSemiHbm) {
      a.gslots = scratch<unsigned long long>(slots);
      RDFGPU_HIP(hipMemsetAsync(a.gslots, 0, slots * sizeof(unsigned long long), stream));
      timed(KC_SEMI_BUILD, 0, R.cap, R.n_dev, 4ull * a.n_keys + 8, nullptr, 0, 0, [&] { launch_semi_build(a, filter == kSemiNoFilter, stream); });
      build_bytes = 0;
    }
  } else {
    build_bytes = 4ull * R.n_cols * R.cap;   // the right rows staged once (re-reads of them come from L2)
  }
  // compulsory bytes: 4·(k + c)·N_left (keys and left filter columns) + 4·c_out·N_out (the survivors' columns, read and written:
  // 8 per cell) + the build's; right columns of candidates are not counted (their number depends on the data)
  timed(semi_join_class(form, anti), build_bytes, L.cap, L.n_dev, 4ull * (a.n_keys + left_fcols), a.n_out_dev, 0, 8ull * nd.n_proj,
        [&] { launch_semi_join(a, form, anti, filter, stream); });
  t.cap = L.cap; t.n_dev = a.n_out_dev;
  return t;
}

// AggregateExec(mode=Single) (aggregate.hip): group pass, one read-back of the group count (it sizes the accumulators and is the
// output's row count), accumulate pass, one lane per group to finish.  Over a zero-key aggregate there is one group and no group pass.
// Compulsory bytes: per input row 4 per key column, 4 + 16 per SUM / AVG input (id + typed value), 4 per COUNT / COUNT
// DISTINCT input; per output group 4 per key column + 24 per aggregate.
DevTable Plan::exec_aggregate(NodeInfo& nd) {
  ChainRequest* const for_this = pending_chain;   // the input is a sub-plan of its own
  pending_chain = nullptr;
  const DevTable in = exec_node((u32)nd.d.left);
  pending_chain = for_this;
  flush_pending_oj();   // a held-back ordered-join write must have happened before the input is read
  if (in.cap >= (1ull << 32)) fail(RDFGPU_ERR_UNSUPPORTED, "AggregateExec over %llu rows (at most 2^32 - 1)", (unsigned long long)in.cap);
  AggArgs a{};
  a.n_keys = nd.d.n_keys;
  for (u32 k = 0; k < a.n_keys; k++) a.key[k] = in.cols[nd.d.left_keys[k]];
  a.n_dev = in.n_dev; a.cap = in.cap;
  a.n_aggs = nd.n_aggs;
  a.n_words = 1;
  a.word_op[0] = kAggAdd;
  u64 accum_row_bytes = 0;
  bool distinct = false;
  for (u32 i = 0; i < a.n_aggs; i++) {
    const u32 fn = nd.agg_fn[i];
    a.fn[i] = fn; a.in[i] = fn == RDFGPU_AGG_COUNT_STAR || nd.agg_prog[i] >= 0 ? nullptr : in.cols[nd.agg_col[i]];
    if (nd.agg_prog[i] >= 0) {   // SUM / AVG over an expression: the VM form of the accumulate pass, over every input column
      a.prog[i] = upload_program(nd.agg_progs[nd.agg_prog[i]]);
      a.exprs = 1;
      for (u32 c = 0; c < in.n_cols; c++) a.col[c] = in.cols[c];
    }
    a.word0[i] = a.n_words;
    const u32 words = fn == RDFGPU_AGG_COUNT_STAR ? 0 : (fn == RDFGPU_AGG_SUM || fn == RDFGPU_AGG_AVG) ? kAggSumWords : 1;
    for (u32 w = 0; w < words; w++) a.word_op[a.n_words + w] = words == 1 ? kAggAdd : w == 0 ? kAggOr : w >= 9 ? kAggAddF64 : kAggAdd;
    a.n_words += words;
    accum_row_bytes += fn == RDFGPU_AGG_COUNT_STAR ? 0 : (fn == RDFGPU_AGG_SUM || fn == RDFGPU_AGG_AVG) ? 20 : 4;
    distinct = distinct || fn == RDFGPU_AGG_COUNT_DISTINCT;
  }
  a.tt = typed_table();
  const u64 cap = in.cap;
  u64 slots = 64;
  while (slots < 2 * cap && slots < (1ull << 32)) slots <<= 1;
  u64 G = 1;
  if (a.n_keys) {
    G = 0;
    if (cap) {
      a.slots = scratch<u32>(slots); a.slot_mask = (u32)(slots - 1);
      a.row_slot = scratch<u32>(cap); a.slot_gid = scratch<u32>(slots); a.rep_row = scratch<u32>(cap);
      a.n_groups_dev = new_counter();
      RDFGPU_HIP(hipMemsetAsync(a.slots, 0, slots * sizeof(u32), stream));
      timed(KC_AGG_GROUPS, 0, cap, in.n_dev, 4ull * a.n_keys, nullptr, 0, 0, [&] { launch_agg_groups(a, stream); });
      G = read_back<u64>(a.n_groups_dev);
    }
  }
  a.n_groups = (u32)G;
  DevTable t;
  t.n_cols = a.n_keys; t.cap = G;
  for (u32 k = 0; k < a.n_keys; k++) { a.out_key[k] = scratch<u32>(G); t.cols[k] = a.out_key[k]; }
  for (u32 i = 0; i < a.n_aggs; i++) a.out[i] = scratch<rdfgpu_agg_value>(G);
  if (&nd == &nodes[root]) agg_out.assign(a.out, a.out + a.n_aggs);
  if (G == 0) return t;
  a.acc = scratch<unsigned long long>(a.n_words * G);
  RDFGPU_HIP(hipMemsetAsync(a.acc, 0, a.n_words * G * sizeof(unsigned long long), stream));
  if (cap) {
    if (distinct) {
      a.dset_mask = (u32)(slots - 1);
      for (u32 i = 0; i < a.n_aggs; i++) {
        if (a.fn[i] != RDFGPU_AGG_COUNT_DISTINCT) continue;
        a.dset[i] = scratch<unsigned long long>(slots);
        RDFGPU_HIP(hipMemsetAsync(a.dset[i], 0, slots * sizeof(unsigned long long), stream));
      }
    }
    a.lds = !opt.on(RDFGPU_OPT_NO_AGG_LDS) && (u64)a.n_words * G * sizeof(unsigned long long) <= kAggLdsBytes;
    timed(a.exprs ? (a.lds ? KC_AGG_ACCUM_EXPR_LDS : KC_AGG_ACCUM_EXPR_HBM) : a.lds ? KC_AGG_ACCUM_LDS : KC_AGG_ACCUM_HBM, 0, cap, in.n_dev, accum_row_bytes, nullptr, 0, 0, [&] { launch_agg_accum(a, stream); });
  }
  timed(KC_AGG_FINAL, 0, 0, nullptr, 0, nullptr, G, 4ull * a.n_keys + 24ull * a.n_aggs, [&] { launch_agg_final(a, stream); });
  return t;
}

// Which input the hash join builds on.  A left join must build on the preserved (left) side.  An inner join builds
// on the smaller input — unless exactly one input is a pure slice of the store (the same rows on every execution
// until the store changes) and the other one is no larger: the slice's join table (direct-address / CSR / hash) is
// built once and cached on the node, so building there costs nothing per execution and the probe is the SMALL side
// (an index nested-loop join against the store's own permutation: `PARAMS JOIN (?s p ?o)` touches |PARAMS| rows,
// not the 5 M-row predicate partition).
bool Plan::choose_build_left(const NodeInfo& nd, const DevTable& L, const DevTable& R, bool left_join, bool lf, bool rf, bool lpost, bool rpost) const {
  if (left_join) {
    // OPTIONAL: HashJoinExec(Left) builds on its left input and probes with the right one — every row of the right input is read, however few
    // left rows there are.  When the right input is a store slice (its join table is cached per store version) and much larger than the left, the
    // join is run the other way round and PRESERVES ITS PROBE SIDE: build = the slice's table, probe = the left rows, a probe row without a match is
    // emitted once with a null right side (LdsJoinArgs::probe_outer).  Same multiset of rows.  Needs: no join filter, no fused filter.
    const bool rs = R.stable_id != 0 && R.n_dev == nullptr && !rf && !lf;
    if (rs && nd.d.kind == RDFGPU_NODE_HASH_JOIN && nd.shape == 0 && !opt.on(RDFGPU_OPT_NO_TABLE_CACHE) && !opt.on(RDFGPU_OPT_NO_INDEX_JOIN) &&
        !opt.on(RDFGPU_OPT_NO_PROBE_OUTER_JOIN) && R.cap > 1024 && L.cap * 4 <= R.cap && L.cap < (1ull << 31))
      return false;
    return true;
  }
  const bool smaller_left = L.cap <= R.cap;
  if (nd.d.kind != RDFGPU_NODE_HASH_JOIN || opt.on(RDFGPU_OPT_NO_TABLE_CACHE) || opt.on(RDFGPU_OPT_NO_INDEX_JOIN)) return smaller_left;
  // (a slice under a `col <=|!=> literal` FilterExec still counts: that filter can run as a conjunct of the join filter)
  const bool ls = L.stable_id != 0 && L.n_dev == nullptr && (!lf || lpost), rs = R.stable_id != 0 && R.n_dev == nullptr && (!rf || rpost);
  if (!ls && !rs) return smaller_left;
  // candidate: build on the slice (the larger one when both inputs are slices), probe with the other input
  const bool slice_left = ls && rs ? !smaller_left : ls;
  const DevTable& S = slice_left ? L : R; const DevTable& O = slice_left ? R : L;
  if (O.cap > S.cap) return smaller_left;                   // the slice is already the smaller side
  if (ls && rs && O.cap * 8 > S.cap) return smaller_left;   // two slices of similar size: nothing to gain
  if (S.cap <= 1024) return smaller_left;                   // LDS-table territory
  // A slice whose keys are not one dense id range (several key columns, or an earlier attempt on this very slice said
  // so) gets a cached HASH table: built once per store version, probed with the fewer rows.  It loses only to a small
  // table built on the other side that stays in L2 while the slice's would not (measured on LUBM Q9's two-key join,
  // 24.6 M rows against a 57 M-row slice: 5.9 ms building on the smaller side every run, 1.3 ms on the cached slice).
  bool hash_only = nd.d.n_keys != 1;
  if (!hash_only) {
    SliceKey sk; sk.n_keys = 1; sk.rows = S.cap; sk.key[0] = S.cols[slice_left ? nd.d.left_keys[0] : nd.d.right_keys[0]];
    const SliceTable* st = store->find_slice_table(sk);
    hash_only = st && st->dense_failed;
  }
  if (hash_only) {
    // The slice is sorted by one of the join keys and the other input is large: building on THAT input inside the step — partition passes
    // over its rows, the slice read in place as id-range partitions (part_join.hip) — beats probing the slice's cached hash table, whose
    // probes are random 64-byte reads of a table far larger than the caches.  Measured on LUBM-8000 Q9's closing two-key join (98 M rows
    // against the 229 M-row takesCourse slice): 3.0 ms with the build in the step, 4.2 - 5.0 ms on the cached table.  The partitioned join
    // walks the whole slice, so it pays only when the other input is a good fraction of it (break-even near a fifth, from those numbers).
    bool sorted_by_key = false;
    for (u32 k = 0; k < nd.d.n_keys; k++) sorted_by_key = sorted_by_key || (S.sorted_col >= 0 && (u32)S.sorted_col == (slice_left ? nd.d.left_keys[k] : nd.d.right_keys[k]));
    if (sorted_by_key && !(ls && rs) && !lf && !rf && nd.d.n_keys <= 2 && S.key_min >= 1 && S.key_max >= S.key_min &&
        !opt.on(RDFGPU_OPT_NO_PARTITIONED_JOIN) && !opt.on(RDFGPU_OPT_NO_RANGE_PARTITION) && !opt.on(RDFGPU_OPT_NO_OWN_PARTITION_PASS) &&
        O.cap >= opt.v[RDFGPU_OPT_PARTITION_MIN_BUILD] && O.cap * 5 >= S.cap && O.cap < (1ull << 31) && S.cap < (1ull << 31))
      return !slice_left;
    if (S.cap > (256ull << 20)) return smaller_left;                             // 32 B per row: keep the footprint sane
    if (O.cap * 8 > S.cap && O.cap <= (1ull << 20)) return smaller_left;
  }
  return slice_left;
}

// Fused lookup chain (R4): walks down from `top` through inner single-key hash joins whose one input is a pure store
// slice with a cached DIRECT-address table and whose other input is a hash join consumed only here.  Only tried on
// speculative re-executions (cardinalities and tables known from the first run).
bool Plan::plan_chain(NodeInfo& top, ChainRequest& req) {
  if (!speculative || !top.has_last || opt.on(RDFGPU_OPT_NO_CHAIN_FUSION) || opt.on(RDFGPU_OPT_NO_TABLE_CACHE)) return false;
  req.top = &top;
  std::vector<ChainLink> down;
  NodeInfo* cur = &top;
  while ((int)down.size() < kMaxChain) {
    const rdfgpu_plan_node& d = cur->d;
    if (d.kind != RDFGPU_NODE_HASH_JOIN || d.join_type != RDFGPU_JOIN_INNER || d.n_keys != 1) break;
    if (cur->prog.n != 0 && cur->shape != 2 && cur->shape != 3) break;
    bool found = false;
    for (int side = 0; side < 2 && !found; side++) {
      const u32 cs = (u32)(side == 0 ? d.left : d.right), co = (u32)(side == 0 ? d.right : d.left);
      const NodeInfo& sn = nodes[cs]; const NodeInfo& on = nodes[co];
      if (sn.d.kind != RDFGPU_NODE_DATA_SOURCE || sources[sn.source].has_residual) continue;
      if (on.d.kind != RDFGPU_NODE_HASH_JOIN || on.d.join_type > RDFGPU_JOIN_LEFT || on.refs != 1) continue;   // (a semi / anti join is no chain base)
      const DevTable S = exec_node(cs);   // a slice: no launch
      if (S.cap == 0 || S.stable_id == 0) continue;
      SliceKey sk; sk.n_keys = 1; sk.rows = S.cap; sk.key[0] = S.cols[side == 0 ? d.left_keys[0] : d.right_keys[0]];
      const SliceTable* st = store->find_slice_table(sk);
      if ((!st || !st->dense_tried) && S.n_dev == nullptr && S.cap > std::min<u64>(opt.v[RDFGPU_OPT_LDS_MAX_BUILD], kLdsJoinMaxBuild) && !opt.on(RDFGPU_OPT_NO_DIRECT_TABLE)) {
        // the store changed since this chain last ran (its history is still good): the slice's table is built here, inside
        // the execution, and the chain stays fused — no un-fused execution just to get the tables back
        SliceTable* fresh = store->slice_table(sk);
        std::unique_lock<std::mutex> building(store->slice_build_mu);
        if (!fresh->dense_tried) build_dense_table(fresh, sk.key[0], S.cap);
        st = fresh;
      }
      if (!st || !st->direct) continue;
      down.push_back(ChainLink{cur, side == 0, S, st});
      cur = &nodes[co];
      found = true;
    }
    if (!found) break;
  }
  if (down.empty()) return false;
  req.links.assign(down.rbegin(), down.rend());   // bottom-up: links[0] sits directly above the base join
  return true;
}

// Resolves the chain against the base join `j` and leaves it in j.a: as a band join where it has that shape (j.use_band, j.band), else with the range index
// of its first stage where that applies.  false (j.a.n_chain stays 0: the stages written so far are not read) if some column cannot be addressed the way the kernel needs.
bool Plan::apply_chain(const ChainRequest& req, LdsJoin& j) {
  if (!resolve_chain(req, j)) return false;
  j.use_band = chain_band_args(req, j);
  if (!j.use_band) chain_range_index(j, j.a.chain[0]);
  j.a.n_chain = (u32)req.links.size(); j.a.n_out_cols = (u32)j.chain_cols.size();
  for (size_t k = 0; k < j.chain_cols.size(); k++) j.a.chain_out[k] = j.chain_cols[k];
  return true;
}

// The chain's stages bottom-up (j.a.chain): each stage's key, table, filter operands and output columns (j.chain_cols) as references to base columns or to its own slice's.
bool Plan::resolve_chain(const ChainRequest& req, LdsJoin& j) {
  const NodeInfo& base = j.nd; std::vector<ColRef>& cur = j.chain_cols;
  cur.resize(base.n_proj);
  for (u32 k = 0; k < base.n_proj; k++) {
    const u32 col = base.proj[k];
    const bool from_left = col < j.L.n_cols;
    cur[k] = ColRef{from_left ? j.L.cols[col] : j.R.cols[col - j.L.n_cols], (from_left == j.build_left) ? 1u : 0u, 0u};
  }
  j.stage_bytes = 0;
  for (size_t t = 0; t < req.links.size(); t++) {
    const ChainLink& ln = req.links[t];
    const NodeInfo& N = *ln.node;
    const u32 wl = nodes[N.d.left].width;
    const u32 prev_w = ln.slice_is_left ? nodes[N.d.right].width : wl;
    if (prev_w != cur.size()) return false;
    bool bad = false;
    auto resolve = [&](u32 col) -> ColRef {
      const bool in_left = col < wl; const u32 local = in_left ? col : col - wl;
      if (in_left == ln.slice_is_left) { if (local >= ln.slice.n_cols) { bad = true; return ColRef{}; } return ColRef{ln.slice.cols[local], 2u + (u32)t, 0u}; }
      if (local >= cur.size()) { bad = true; return ColRef{}; }
      return cur[local];
    };
    ChainStage& st = j.a.chain[t]; std::memset(&st, 0, sizeof st);
    const u32 prev_key = ln.slice_is_left ? N.d.right_keys[0] : N.d.left_keys[0];
    if (prev_key >= cur.size()) return false;
    st.key = cur[prev_key];
    if (st.key.src > 1) return false;                       // the kernel looks a stage up from a BASE column
    st.direct = ln.table->direct; st.kmin = ln.table->kmin; st.kn = ln.table->kn;
    u32 n_fcols = 0;
    if (N.prog.n == 0) st.fs = 0;
    else if (N.shape == 2) {
      st.fs = 2; n_fcols = 2;
      st.f[0] = resolve(N.prog.nodes[0].u); st.f[1] = resolve(N.prog.nodes[1].u);
      st.is_eq = N.prog.nodes[2].op == RDFGPU_EX_ID_EQ;
    } else if (N.shape == 3) {
      const rdfgpu_expr_node* e = N.prog.nodes;
      st.fs = 3; n_fcols = 4;
      st.f[0] = resolve(e[0].u); st.f[1] = resolve(e[2].u); st.f[2] = resolve(e[8].u); st.f[3] = resolve(e[10].u);
      st.l0 = window_literal(e, 0); st.l1 = window_literal(e, 8);
    } else return false;
    for (u32 q = 0; q < n_fcols; q++) if (st.f[q].src > 1 && st.f[q].src != 2u + (u32)t) return false;   // base columns or this stage's
    // integer window whose x operand is a column of this stage's slice and whose y operands are base columns: use the slice's decoded value table
    if (st.fs == 3 && st.f[0].src == 2u + (u32)t && st.f[2].src == st.f[0].src && st.f[2].ptr == st.f[0].ptr && st.f[1].src <= 1 && st.f[3].src <= 1 &&
        !opt.on(RDFGPU_OPT_NO_VALUE_TABLES)) {
      const SliceTable::ValueColumn vc = slice_value_column(ln, st.f[0].ptr);
      if (vc.usable) { st.val = vc.val; j.chain_vc[t] = vc; }
    }
    std::vector<ColRef> next(N.n_proj);
    for (u32 k = 0; k < N.n_proj; k++) next[k] = resolve(N.proj[k]);
    if (bad) return false;
    cur.swap(next);
    j.stage_bytes += base.last_rows * (8ull + 4ull * n_fcols);   // per candidate: key + table slot + filter operands (estimate)
  }
  return cur.size() == req.top->n_proj && cur.size() <= (size_t)kMaxCols;
}

// {min, max} of the i64 values `launch(slots)` folds into two counter slots, read back in one host round trip.
template <class F> void Plan::device_minmax_i64(long long (&got)[2], F&& launch) {
  long long* mm = reinterpret_cast<long long*>(new_counter()); (void)new_counter();   // {min, max}: two slots
  const long long init[2] = {INT64_MAX, INT64_MIN + 1};
  RDFGPU_HIP(hipMemcpyAsync(mm, init, sizeof init, hipMemcpyHostToDevice, stream));
  launch(mm);
  read_back(got, mm, sizeof got);
}

// The decoded value table of column `col` of a chain link's slice: found (one entry per column: pushed only after a failed look-up under the same lock) or built now, once per store version.  A copy: the list may grow.
SliceTable::ValueColumn Plan::slice_value_column(const ChainLink& ln, const u32* col) {
  SliceTable* tab = const_cast<SliceTable*>(ln.table);
  std::unique_lock<std::mutex> building(store->slice_build_mu);
  for (const auto& v : tab->values) if (v.col == col) return v;
  const u32 key_local = ln.slice_is_left ? ln.node->d.left_keys[0] : ln.node->d.right_keys[0];
  long long* val = store->table_alloc<long long>(tab->kn); metrics.tables_built++;
  u32* bad = reinterpret_cast<u32*>(new_counter());
  launch_fill_i64(val, INT64_MIN, tab->kn, stream);
  launch_direct_values(ln.slice.cols[key_local], col, ln.slice.cap, tab->kmin, tab->kn, typed_table(), val, bad, stream);
  if (read_back<u32>(bad)) { store->table_free(val); val = nullptr; }
  SliceTable::ValueColumn fresh{col, val, val != nullptr};
  if (val) {   // value range: the bias of the band join's 32-bit window intervals
    long long got[2]; device_minmax_i64(got, [&](long long* mm) { launch_val_minmax(val, tab->kn, mm, stream); });
    fresh.vmin = got[0]; fresh.vmax = got[1];
  }
  tab->values.push_back(fresh);
  return fresh;
}

// Band join (band_join.hip): when the groups of the CSR base are small, every stage hangs off a BUILD column and the stage filters are integer windows between a stage value
// and probe columns, the chain runs group by group — both sides partitioned by the key, the pair tests in registers — instead of probe row by probe row.  true: j.band is filled.
bool Plan::chain_band_args(const ChainRequest& req, LdsJoin& j) {
  const LdsJoinArgs& a = j.a; BandArgs b{};
  if (!a.csr_off || !j.slice || opt.on(RDFGPU_OPT_NO_BAND_JOIN) || arg_slots_used >= ExecContext::kArgSlots) return false;
  if (a.n_keys != 1 || (a.has_filter != 0 && a.has_filter != 2) || a.has_probe_filter != 0 || a.visited != nullptr) return false;
  if (a.has_filter == 2) {
    const bool ab = on_build_side(a, a.idp.a), bb = on_build_side(a, a.idp.b);
    if (ab == bb) return false;
    b.has_neq = 1; b.neq_is_eq = a.idp.is_eq; b.neq_build = a.cols[ab ? a.idp.a : a.idp.b]; b.neq_probe = a.cols[ab ? a.idp.b : a.idp.a];
  }
  if (a.has_post) {
    if (!on_build_side(a, a.post.col)) return false;
    b.has_post = 1; b.post_col = a.cols[a.post.col]; b.post_lit = a.post.lit; b.post_is_eq = a.post.is_eq;
  }
  b.n_stages = (u32)req.links.size();
  bool pack16 = !opt.on(RDFGPU_OPT_NO_BAND_PACK16);
  for (size_t t = 0; t < req.links.size(); t++) {
    const ChainStage& st = a.chain[t];
    if (st.key.src != 1 || (st.fs != 0 && st.fs != 3)) return false;
    b.stage[t] = BandStage{st.key.ptr, st.direct, st.kmin, st.kn};
    if (st.fs == 0) continue;
    const SliceTable::ValueColumn& vc = j.chain_vc[t];
    if (st.val == nullptr || b.n_win >= 2 || st.f[1].src != 0 || st.f[3].src != 0 || !range_op(st.l0.cmp_op) || !range_op(st.l1.cmp_op) ||
        vc.vmin > vc.vmax || (unsigned long long)vc.vmax - (unsigned long long)vc.vmin >= 0xFFFFFFE0ull) return false;   // (unsigned: the spread of two i64 may exceed i64)
    BandWin& w = b.win[b.n_win++];
    if ((unsigned long long)vc.vmax - (unsigned long long)vc.vmin > 65530ull) pack16 = false;   // biased values 1 .. range + 1 have to fit 16 bits
    w.key_col = st.key.ptr; w.val = st.val; w.vkmin = st.kmin; w.vkn = st.kn; w.vbase = vc.vmin;
    w.y0 = st.f[1].ptr; w.y1 = st.f[3].ptr; w.l0 = st.l0; w.l1 = st.l1; w.stage = (u32)t;
  }
  b.pack16 = pack16 ? 1u : 0u;
  for (size_t k = 0; k < j.chain_cols.size(); k++) {
    const ColRef& col = j.chain_cols[k];
    if (col.src == 0 ? b.n_row_cols >= kBandMaxRowCols : b.n_entry_cols >= kBandMaxSideCols) return false;
    if (col.src == 0) { b.out_from_row[k] = 1; b.out_sel[k] = (u8)b.n_row_cols; b.row_col[b.n_row_cols++] = col.ptr; }
    else { b.out_from_row[k] = 0; b.out_sel[k] = (u8)(2 + b.n_entry_cols); b.entry_col[b.n_entry_cols++] = col; }
  }
  // group sizes: the largest decides (one wave joins a whole group)
  if (csr_max_group(j.slice, a) > kBandMaxGroup || j.B.cap < 4ull * a.direct_n || j.P.cap * 4 < a.direct_n || j.P.cap >= (1ull << 31)) return false;
  j.band = b;
  return true;
}

// Rows of the largest group of a slice's CSR table: measured once per table, under the lock.
u32 Plan::csr_max_group(SliceTable* tab, const LdsJoinArgs& a) {
  std::unique_lock<std::mutex> building(store->slice_build_mu);
  if (tab->csr_max_group) return tab->csr_max_group;
  u32* mx = reinterpret_cast<u32*>(new_counter());
  launch_csr_max_group(a.csr_off, a.direct_n, mx, stream);
  return tab->csr_max_group = std::max(1u, read_back<u32>(mx));
}

// Range index: a CSR base whose first stage `s0` is an integer window (GT / LT / GEQ / LEQ) between the stage's decoded value and probe-side columns expands, per probe row,
// only the part of the key's group whose value can pass — the group is kept sorted by that value (found on the CSR table or built now, once per store version, under the lock).
void Plan::chain_range_index(LdsJoin& j, const ChainStage& s0) {
  LdsJoinArgs& a = j.a;
  if (!a.csr_off || !j.slice || !s0.val || s0.fs != 3 || s0.key.src != 1 || s0.f[1].src != 0 || s0.f[3].src != 0 ||
      !range_op(s0.l0.cmp_op) || !range_op(s0.l1.cmp_op) || opt.on(RDFGPU_OPT_NO_RANGE_INDEX)) return;
  std::unique_lock<std::mutex> building(store->slice_build_mu);
  SliceTable::RangeIndex* ri = nullptr;
  for (auto& r : j.slice->ranges) if (r.val == s0.val && r.link_col == s0.key.ptr) ri = &r;
  if (!ri) {
    SliceTable::RangeIndex fresh{s0.val, s0.key.ptr, nullptr, nullptr, 0, nullptr, false};
    const u64 n = j.B.cap;
    long long got[2]; device_minmax_i64(got, [&](long long* mm) { launch_range_minmax(s0.key.ptr, a.csr_rows, n, s0.val, s0.kmin, s0.kn, mm, stream); });
    if (got[0] <= got[1] && (unsigned long long)got[1] - (unsigned long long)got[0] < 0xFFFFFFF0ull && n < (1ull << 32)) {
      u64* key_in = scratch<u64>(n); u64* key_out = scratch<u64>(n); u32* rows_in = scratch<u32>(n);
      fresh.rows = store->table_alloc<u32>(n); fresh.vals = store->table_alloc<u32>(n);
      metrics.tables_built++; fresh.vbase = got[0];
      launch_range_keys(a.build_key[0], a.direct_min, s0.key.ptr, a.csr_rows, n, s0.val, s0.kmin, s0.kn, got[0], key_in, rows_in, stream);
      const size_t tb = sort_temp_bytes(n); void* temp = scratch<unsigned char>(tb);
      sort_pairs_u64_u32(key_in, key_out, rows_in, fresh.rows, n, temp, tb, stream);
      launch_range_decode(key_out, n, fresh.vals, stream);
      fresh.link = store->table_alloc<u32>(n);
      launch_gather_u32(s0.key.ptr, fresh.rows, fresh.link, n, stream);   // the link column in index order
      RDFGPU_HIP(hipStreamSynchronize(stream)); metrics.host_syncs++;
      fresh.usable = true;
    }
    j.slice->ranges.push_back(fresh);
    ri = &j.slice->ranges.back();
  }
  if (ri->usable) { a.range_rows = ri->rows; a.range_vals = ri->vals; a.range_vbase = ri->vbase; a.range_link = ri->link; a.range_link_col = ri->link_col; }
}

// The held-back write pass of an ordered slice join runs before anything reads its table, except the band join that consumes
// it: it may stay pending into a join only while the table is that join's probe side — an inner LDS join whose band join took
// the records last time (the sides as exec_join chooses them below).  exec_lds_join then hands it on to the band join or runs
// it just before the probe side is read.
bool Plan::keeps_pending_oj(const NodeInfo& nd, const DevTable& L, const DevTable& R, bool left_join, bool lf, bool rf) const {
  if (!nd.band.takes_records || nd.d.kind != RDFGPU_NODE_HASH_JOIN || left_join || lf || rf || opt.on(RDFGPU_OPT_NO_LDS_JOIN)) return false;
  const bool build_left = choose_build_left(nd, L, R, false, false, false);
  const DevTable& B = build_left ? L : R; const DevTable& P = build_left ? R : L;
  return (B.cap <= kLdsJoinMaxBuild || !opt.on(RDFGPU_OPT_NO_GLOBAL_TABLE_JOIN)) && P.cols[0] == pending_oj.first_col && B.cols[0] != pending_oj.first_col;
}

// The held-back write pass of an ordered slice join, run after all: its consumer turned out not to take the band join's records.
void Plan::flush_pending_oj() {
  if (!pending_oj.active) return;
  count_pending_oj();
  pending_oj.active = false;
  const OrderedJoinArgs& o = pending_oj.o;
  timed(KC_OJ_WRITE, 0, pending_oj.n_build, nullptr, 4, o.n_out_dev, 0, 8ull * o.n_out_cols, [&] { launch_ordered_join_write(o, stream); });
}

// The count pass of an ordered slice join and the scan of its per-tile counts: where every match goes.
void Plan::count_ordered_join(OrderedJoinArgs& o) {
  const u64 tiles = ordered_join_tiles(o.n_build);
  o.tile_count = scratch<u32>(tiles + 1); o.tile_off = scratch<u32>(tiles + 1);
  o.row_head = scratch<u32>(o.n_build); o.row_cnt = scratch<unsigned char>(o.n_build);
  const size_t tb = scan_temp_bytes(tiles + 1);
  void* temp = scratch<unsigned char>(tb);
  timed(KC_OJ_COUNT, 0, o.n_build, nullptr, 4, nullptr, 0, 0, [&] { launch_ordered_join_count(o, stream); });
  timed(scan_class(tiles + 1), 0, tiles + 1, nullptr, 8, nullptr, 0, 0, [&] { exclusive_scan_u32(o.tile_count, o.tile_off, tiles + 1, temp, tb, stream); });
}
// The held-back ordered slice join skipped its count pass for an in-place band join that does not take it after all: it runs now,
// and so does the check of the count its write pass will write.
void Plan::count_pending_oj() {
  if (!pending_oj.active || pending_oj.counted) return;
  pending_oj.counted = true;
  count_ordered_join(pending_oj.o);
  spec_checks.push_back(pending_oj.check);
}

DevTable Plan::exec_join(NodeInfo& nd) {
  const bool left_join = nd.d.join_type == RDFGPU_JOIN_LEFT;
  if (!pending_chain) {
    ChainRequest req;
    if (plan_chain(nd, req)) {
      NodeInfo* base = req.links.front().slice_is_left ? &nodes[req.links.front().node->d.right] : &nodes[req.links.front().node->d.left];
      req.base = base;
      pending_chain = &req;
      const DevTable fused = exec_node((u32)(base - nodes.data()));
      pending_chain = nullptr;
      if (req.consumed) return fused;      // `fused` already has this node's schema
      // not taken (the base join ran normally and is memoised): continue the ordinary way
    }
  }
  // Pipeline fusion: a FilterExec child (identity projection, consumed by this join only) is not
  // materialised when it ends up on the probe side of the LDS join — its predicate runs inside the probe.
  auto fusable = [&](int32_t ci) {
    if (nd.d.kind != RDFGPU_NODE_HASH_JOIN || opt.on(RDFGPU_OPT_NO_FILTER_FUSION) || opt.on(RDFGPU_OPT_NO_LDS_JOIN)) return false;
    const NodeInfo& c = nodes[ci];
    if (c.d.kind != RDFGPU_NODE_FILTER || c.prog.n == 0 || c.refs != 1 || c.n_proj != nodes[c.d.left].width) return false;
    for (u32 k = 0; k < c.n_proj; k++) if (c.proj[k] != k) return false;
    return true;
  };
  bool lf = !left_join && fusable(nd.d.left), rf = fusable(nd.d.right);
  // the inputs are sub-plans of their own: a chain request pending for THIS join must not keep the joins below from
  // planning theirs (the batched Q5 has two: the constants' look-ups by X, and window 1 / window 2 / label above the
  // candidate join)
  ChainRequest* const for_this_join = pending_chain;
  pending_chain = nullptr;
  DevTable L = lf ? exec_node((u32)nodes[nd.d.left].d.left) : exec_node((u32)nd.d.left);
  DevTable R = rf ? exec_node((u32)nodes[nd.d.right].d.left) : exec_node((u32)nd.d.right);
  pending_chain = for_this_join;
  if (pending_oj.active && !keeps_pending_oj(nd, L, R, left_join, lf, rf)) flush_pending_oj();
  const NodeInfo* post = nullptr;   // a build-side FilterExec kept as a conjunct of the join filter (see below)
  if (lf || rf) {
    // `col <=|!=> literal` over a store slice: if the join builds on that slice (index join through the slice's cached
    // table) the FilterExec is neither materialised nor fused into the probe — it becomes one more conjunct of the
    // join filter, evaluated on the candidate pairs
    auto postable = [&](bool has, int32_t ci, const DevTable& in) {
      return has && nodes[ci].shape == 1 && in.stable_id != 0 && in.n_dev == nullptr && in.cap > 1024 && nd.d.n_keys == 1 && !opt.on(RDFGPU_OPT_NO_INDEX_JOIN);
    };
    const bool lpost = postable(lf, nd.d.left, L), rpost = postable(rf, nd.d.right, R);
    const bool build_left = choose_build_left(nd, L, R, left_join, lf, rf, lpost, rpost);
    const bool lds = ((build_left ? L.cap : R.cap) <= kLdsJoinMaxBuild || !opt.on(RDFGPU_OPT_NO_GLOBAL_TABLE_JOIN)) && L.cap && R.cap;
    if (lds && lf && build_left && lpost) { post = &nodes[nd.d.left]; lf = false; }
    else if (lds && rf && !build_left && rpost) { post = &nodes[nd.d.right]; rf = false; }
    // a fused filter survives only on the probe side of the LDS join; anything else is materialised now
    if (lf && (!lds || build_left)) { L = apply_filter(nodes[nd.d.left], L); lf = false; }
    if (rf && (!lds || !build_left)) { R = apply_filter(nodes[nd.d.right], R); rf = false; }
  }
  DevTable t;
  t.n_cols = nd.n_proj;

  if (nd.d.kind == RDFGPU_NODE_CROSS_JOIN) {
    const u64 cap = L.cap * R.cap;
    if (cap == 0) { t.cap = 0; return t; }
    if (cap >= (1ull << 40)) fail(RDFGPU_ERR_UNSUPPORTED, "cross join of %llu x %llu rows", (unsigned long long)L.cap, (unsigned long long)R.cap);
    CrossArgs a{};
    for (u32 c = 0; c < L.n_cols; c++) a.left[c] = L.cols[c];
    for (u32 c = 0; c < R.n_cols; c++) a.right[c] = R.cols[c];
    a.n_left_cols = L.n_cols; a.n_right_cols = R.n_cols; a.n_out_cols = nd.n_proj;
    for (u32 c = 0; c < nd.n_proj; c++) { a.proj[c] = nd.proj[c]; a.out[c] = scratch<u32>(cap); t.cols[c] = a.out[c]; }
    a.n_left_dev = L.n_dev; a.n_left_cap = L.cap; a.n_right_dev = R.n_dev; a.n_right_cap = R.cap;
    const bool dyn = L.n_dev || R.n_dev;
    a.n_out_dev = dyn ? new_counter() : nullptr;
    // CrossJoinExec bytes: 4·c·N (both inputs read once) + 4·c_o·m·N (every output cell written)
    timed(KC_CROSS, 4ull * R.n_cols * R.cap, L.cap, L.n_dev, 4ull * L.n_cols, a.n_out_dev, dyn ? 0 : cap, 4ull * nd.n_proj,
          [&] { launch_cross(a, stream); });
    t.cap = cap; t.n_dev = a.n_out_dev;
    return t;
  }

  // HashJoinExec / NestedLoopJoinExec
  if (L.cap == 0 || (R.cap == 0 && !left_join)) { t.cap = 0; return t; }
  const bool hash = nd.d.kind == RDFGPU_NODE_HASH_JOIN;
  if (hash && !opt.on(RDFGPU_OPT_NO_LDS_JOIN)) {
    const bool build_left = choose_build_left(nd, L, R, left_join, lf, rf);
    if ((build_left ? L.cap : R.cap) <= kLdsJoinMaxBuild || !opt.on(RDFGPU_OPT_NO_GLOBAL_TABLE_JOIN)) {
      const NodeInfo* pf = lf ? &nodes[nd.d.left] : rf ? &nodes[nd.d.right] : nullptr;
      if (post && build_left != (post == &nodes[nd.d.left])) fail(RDFGPU_ERR_DEVICE, "join: build side changed under a residual filter");
      return exec_lds_join(nd, L, R, build_left, pf, post);
    }
  }
  JoinArgs a{};
  for (u32 c = 0; c < L.n_cols; c++) a.left[c] = L.cols[c];
  for (u32 c = 0; c < R.n_cols; c++) a.right[c] = R.cols[c];
  a.n_left_cols = L.n_cols; a.n_right_cols = R.n_cols; a.n_out_cols = nd.n_proj;
  for (u32 c = 0; c < nd.n_proj; c++) a.proj[c] = nd.proj[c];
  a.n_keys = hash ? nd.d.n_keys : 0;
  for (u32 k = 0; k < a.n_keys; k++) { a.left_keys[k] = nd.d.left_keys[k]; a.right_keys[k] = nd.d.right_keys[k]; }
  a.n_left_dev = L.n_dev; a.n_left_cap = L.cap; a.n_right_dev = R.n_dev; a.n_right_cap = R.cap;
  a.has_filter = nd.prog.n ? 1 : 0;
  a.prog = nd.prog;
  a.tt = typed_table();
  if (L.cap >= 0xFFFFFFF0ull) fail(RDFGPU_ERR_UNSUPPORTED, "build side of %llu rows", (unsigned long long)L.cap);
  if (left_join) { a.visited = scratch<u8>(L.cap); if (!hash) RDFGPU_HIP(hipMemsetAsync(a.visited, 0, L.cap, stream)); }
  if (hash) {
    const u32 nb = pow2_at_least(2 * L.cap);
    a.heads = scratch<u32>(nb); a.bucket_mask = nb - 1;
    a.next = scratch<u32>(L.cap);
    RDFGPU_HIP(hipMemsetAsync(a.heads, 0xFF, (size_t)nb * 4, stream));
    // build: 4·k·N_b keys read + 8·N_b (one head/next slot written per row)   (build half)
    timed(KC_JOIN_BUILD, 0, L.cap, L.n_dev, 4ull * a.n_keys + 8, nullptr, 0, 0, [&] { launch_join_build(a, stream); });
  }
  // columns of the probe side the write pass has to read: keys ∪ projected right columns ∪ filter columns
  u32 probe_cols = 0;
  {
    bool used[kMaxCols] = {};
    for (u32 k = 0; k < a.n_keys; k++) used[a.right_keys[k]] = true;
    for (u32 c = 0; c < nd.n_proj; c++) if (nd.proj[c] >= L.n_cols) used[nd.proj[c] - L.n_cols] = true;
    for (u32 i = 0; i < nd.prog.n; i++) if (nd.prog.nodes[i].op == RDFGPU_EX_COLUMN && nd.prog.nodes[i].u >= L.n_cols) used[nd.prog.nodes[i].u - L.n_cols] = true;
    for (bool b : used) probe_cols += b;
  }
  u64 total = 0;
  u32* offs = nullptr;
  if (R.cap) {
    u32* counts = scratch<u32>(R.cap);
    offs = scratch<u32>(R.cap);
    const size_t tb = scan_temp_bytes(R.cap);
    void* temp = scratch<u8>(tb);
    a.counts = counts;
    // count pass: 4·k·N_p keys + 8·N_p (head + first chain slot read per probe row)
    timed(hash ? KC_JOIN_COUNT : KC_NLJ_COUNT, 0, R.cap, R.n_dev, 4ull * a.n_keys + 8, nullptr, 0, 0,
          [&] { if (hash) launch_join_count(a, stream); else launch_nlj_count(a, stream); });
    timed(scan_class(R.cap), 0, R.cap, nullptr, 8, nullptr, 0, 0, [&] { inclusive_scan_u32(counts, offs, R.cap, temp, tb, stream); });
    total = read_back<u32>(offs + R.cap - 1);
  }
  const u64 cap = total + (left_join ? L.cap : 0);
  if (cap == 0) { t.cap = 0; return t; }
  for (u32 c = 0; c < nd.n_proj; c++) { a.out[c] = scratch<u32>(cap); t.cols[c] = a.out[c]; }
  if (total) {
    a.counts = offs;
    // write pass: 4·(k+p_p)·N_p + 8·N_p + 4·c_o·N_o   (probe half)
    timed(hash ? KC_JOIN_WRITE : KC_NLJ_WRITE, 0, R.cap, R.n_dev, 4ull * probe_cols + 8, nullptr, total, 4ull * nd.n_proj,
          [&] { if (hash) launch_join_write(a, stream); else launch_nlj_write(a, stream); });
  }
  t.cap = cap;
  if (left_join) {
    u64* n_out = new_counter();
    RDFGPU_HIP(hipMemcpyAsync(n_out, &total, sizeof(u64), hipMemcpyHostToDevice, stream));
    RDFGPU_HIP(hipStreamSynchronize(stream)); metrics.host_syncs++;   // `total` is a stack variable
    left_join_tail(nd, L, R, a.out, a.visited, n_out, 0);
    t.n_dev = n_out;
  }
  return t;
}

// The two kernels both direct-address forms start with: min / max of the single key column (one read-back) and, when the id
// range is at most `max_range` ids, one store per row into a table of one slot per id with a duplicate flag (a second
// read-back).  The table is kept with the store's tables (`cached`) or is scratch of this execution; `direct` is set only when
// the keys turned out unique.
Plan::DirectTable Plan::build_direct(const u32* key, u64 n, u64 max_range, bool cached) {
  DirectTable d;
  u32* mm = reinterpret_cast<u32*>(new_counter());   // {min, max}
  d.flags = reinterpret_cast<u32*>(new_counter());   // {duplicate seen, unsorted seen (build_dense_table)}
  const u32 init[2] = {0xFFFFFFFFu, 0u};
  RDFGPU_HIP(hipMemcpyAsync(mm, init, sizeof(init), hipMemcpyHostToDevice, stream));
  timed(KC_MINMAX, 4ull * n, 0, nullptr, 0, nullptr, 0, 0, [&] { launch_minmax_u32(key, n, mm, stream); });
  u32 got[2];
  read_back(got, mm, sizeof got);
  const u64 range = got[0] <= got[1] ? (u64)(got[1] - got[0]) + 1 : ~0ull;
  if (range > max_range) return d;
  d.dense = true; d.kmin = got[0]; d.kn = got[1] - got[0] + 1;
  // more rows than ids in the range: some key repeats (pigeonhole: null keys only make it more so when they are few; with many nulls the
  // attempt below would have succeeded — then the CSR form is merely the more general table for the same join) — no direct-address attempt
  if (n > (u64)d.kn) return d;
  u32* direct = cached ? store->table_alloc<u32>(d.kn) : scratch<u32>(d.kn);
  RDFGPU_HIP(hipMemsetAsync(direct, 0xFF, (size_t)d.kn * sizeof(u32), stream));
  timed(KC_GDIRECT_BUILD, 0, n, nullptr, 8, nullptr, 0, 0, [&] { launch_gdirect_build(key, n, direct, d.kmin, d.kn, d.flags, stream); });
  if (!read_back<u32>(d.flags)) d.direct = direct;
  else if (cached) store->table_free(direct);
  return d;
}

// The dense join tables of a single-key store slice (decided once per slice and store version, with `slice_build_mu` held):
// direct-address if the keys are unique, CSR (offsets + row ids grouped by key; the identity when the slice is sorted by the
// key) if not; `dense_failed` when the id range is not worth a 4-byte-per-id table.  Costs a few small kernels and host
// syncs at that time, nothing afterwards.
void Plan::build_dense_table(SliceTable* st, const u32* key, u64 n) {
  // "dense" = the id range is worth a 4-B-per-id table: up to 4 ids per row outright; up to 64 ids per row while
  // the table stays small (16 M ids = 64 MB) — a subject-hash shard of a slice keeps the slice's id range with
  // 1/G of its rows, and must not fall off the index-join path for that
  const DirectTable d = build_direct(key, n, std::max<u64>(4 * n + 1024, std::min<u64>(64 * n + 1024, 16ull << 20)), true);
  if (!d.dense) { st->dense_failed = true; st->dense_tried = true; return; }
  metrics.tables_built++;
  const u32 kmin = d.kmin, kn = d.kn;
  st->kmin = kmin; st->kn = kn;
  if (d.direct) { st->direct = d.direct; st->dense_tried = true; return; }
  // duplicates: CSR (offsets + row ids grouped by key) — by boundary searches when the slice is sorted by the key, by one radix sort otherwise
  u32* off = store->table_alloc<u32>((u64)kn + 2); u32* rows = nullptr;
  if (n >= (1ull << 32)) fail(RDFGPU_ERR_UNSUPPORTED, "CSR table of %llu rows", (unsigned long long)n);
  u32* rel = scratch<u32>(n);
  timed(KC_CSR_HIST, 0, n, nullptr, 8, nullptr, 0, 0, [&] { launch_csr_rel_keys(key, n, kmin, kn, rel, d.flags + 1, stream); });
  const u32* grouped = rel;
  if (read_back<u32>(d.flags + 1)) {   // unsorted; else the slice is sorted by the key: rows[] is the identity and is never materialised
    rows = store->table_alloc<u32>(n);
    u32 bits = 1;
    while ((1ull << bits) <= kn) bits++;             // keys 0 .. kn (kn = joins nothing: sorts to the end)
    u32* rel_s = scratch<u32>(n); u32* iota = scratch<u32>(n);
    const size_t stb = sort_u32_temp_bytes(n, bits);
    void* stemp = scratch<unsigned char>(stb);
    launch_iota_u32(iota, n, stream);
    timed(KC_CSR_SCATTER, 0, n, nullptr, 12, nullptr, 0, 0, [&] { sort_pairs_u32_u32(rel, rel_s, iota, rows, n, bits, stemp, stb, stream); });
    grouped = rel_s;
  }
  launch_sorted_bounds(grouped, n, kn, off, stream);   // off[k] = first position with rel >= k, k = 0 .. kn (off[kn] = the rows that join something)
  RDFGPU_HIP(hipStreamSynchronize(stream)); metrics.host_syncs++;   // complete before other plans may see it
  st->csr_rows = rows; st->csr_off = off;
  st->dense_tried = true;
}

// HashJoinExec whose build side is one table — a copy per workgroup in LDS, a store slice's cached table, a table built in this
// execution, or one per partition: one fused kernel, optimistic output capacity.
DevTable Plan::exec_lds_join(NodeInfo& nd, const DevTable& L, const DevTable& R, bool build_left, const NodeInfo* probe_filter, const NodeInfo* post_filter) {
  LdsJoin j(nd, L, R, build_left, probe_filter, post_filter);
  LdsJoinArgs& a = j.a;
  if (j.B.cap >= (1ull << 30)) fail(RDFGPU_ERR_UNSUPPORTED, "build side of %llu rows", (unsigned long long)j.B.cap);
  lds_join_args(j);
  j.table = choose_join_table(j);
  if (j.P.cap >= (1ull << 32)) fail(RDFGPU_ERR_UNSUPPORTED, "probe side of %llu rows", (unsigned long long)j.P.cap);
  size_wave_queue(j);
  if (j.left_join) a.visited = scratch<u8>(L.cap);
  a.n_out_dev = new_counter();
  a.overflow = reinterpret_cast<u32*>(new_counter());
  j.tail = j.left_join ? L.cap : 0;
  if (j.table == JoinTable::ScratchHash)   // build pass: keys read + one 8-byte slot written per build row
    timed(KC_GJOIN_BUILD, 0, j.B.cap, j.B.n_dev, 4ull * a.n_keys + 8, nullptr, 0, 0, [&] { launch_gjoin_build(a, stream); });
  // Speculative mode (re-execution of a plan whose previous run is known): the output is sized from the
  // previous cardinality of this operator and NOTHING is waited for — the exact count stays on the device,
  // the overflow flag is checked once at the end of the plan (Plan::execute), which re-runs exactly if any
  // speculation failed.
  // First execution of a plan (DataFusion compiles a fresh plan per query): no history, but the table form bounds or
  // estimates the output — a direct-address table yields at most one match per probe row (exact bound), a CSR table
  // about its mean rows per key, a hash table is assumed unique-ish — so the join can run without a host round
  // trip as well; the overflow flag at the end of the plan catches a wrong guess (exact re-run).
  u64 first_guess = 0;
  if (speculative && !nd.has_last && !j.left_join && !opt.on(RDFGPU_OPT_NO_FIRST_RUN_SPECULATION)) {
    if (a.direct) first_guess = j.P.cap;
    else if (a.csr_off) first_guess = 2 * j.P.cap * ((j.B.cap + a.direct_n - 1) / (a.direct_n ? a.direct_n : 1)) + 1024;
    else first_guess = j.P.cap + 1024;
  }
  const bool spec = speculative && (nd.has_last || first_guess);
  // a fusable run of follow-up lookups above this join (Plan::plan_chain) executes inside this join's resolve
  // phase: the output is then the TOP node's, sized from the top node's history
  NodeInfo* size_node = &nd;
  if (spec && pending_chain && pending_chain->base == &nd && !pending_chain->consumed && j.global_table && j.table != JoinTable::Partitioned && !j.left_join &&
      !j.probe_outer && !probe_filter && nd.shape != 1 && apply_chain(*pending_chain, j)) {
    pending_chain->consumed = true;
    size_node = pending_chain->top;
    j.t.n_cols = a.n_out_cols;
  }
  // the probe side is read from here on: only the band join takes an ordered slice join's held-back write pass (exec_band_join)
  if (!j.use_band) flush_pending_oj();
  if (j.table == JoinTable::Partitioned) {
    // output of the previous execution (none: single pass): above ~50 M rows the reservations of a single pass (one
    // same-address atomic per 256 rows, ~88 per microsecond) cost more than walking every partition twice
    const u64 expect_out = nd.has_last ? nd.last_rows : 0;
    j.part.two_pass = expect_out >= opt.v[RDFGPU_OPT_PARTITION_TWO_PASS_ROWS] ? 1u : 0u;
    if (j.part.two_pass && nd.shape == 2 && !j.left_join) {   // `build column <=|!=> probe column`: decided during the walk (part_join.hip, INL)
      const u32 ca = nd.prog.nodes[0].u, cb = nd.prog.nodes[1].u;
      if (on_build_side(a, ca) != on_build_side(a, cb)) { j.part.inl_build = a.cols[on_build_side(a, ca) ? ca : cb]; j.part.inl_probe = a.cols[on_build_side(a, ca) ? cb : ca]; }
    }
    prepare_partitions(a, j.B, j.P, j.part);   // the build half of this HashJoinExec: inside the operator, every execution
  }
  return spec ? run_speculative(j, first_guess, *size_node) : run_exact(j);
}

// The kernel arguments that do not depend on the build side's table: both inputs' columns, the keys, the join filter, the fused
// probe-side filter, the build-side filter kept as a conjunct, and the columns each side reads (bytes).
void Plan::lds_join_args(LdsJoin& j) {
  const NodeInfo& nd = j.nd; const DevTable& L = j.L; const DevTable& R = j.R;
  LdsJoinArgs& a = j.a;
  j.t.n_cols = nd.n_proj;
  for (u32 c = 0; c < L.n_cols; c++) a.cols[c] = L.cols[c];
  for (u32 c = 0; c < R.n_cols; c++) a.cols[L.n_cols + c] = R.cols[c];
  a.n_left_cols = L.n_cols; a.n_out_cols = nd.n_proj;
  for (u32 c = 0; c < nd.n_proj; c++) a.proj[c] = nd.proj[c];
  a.build_is_left = j.build_left ? 1 : 0;
  a.probe_outer = j.probe_outer ? 1u : 0u;
  a.n_keys = nd.d.n_keys;
  for (u32 k = 0; k < a.n_keys; k++) {
    j.build_keys[k] = j.build_left ? nd.d.left_keys[k] : nd.d.right_keys[k];
    j.probe_keys[k] = j.build_left ? nd.d.right_keys[k] : nd.d.left_keys[k];
    a.build_key[k] = j.B.cols[j.build_keys[k]];
    a.probe_key[k] = j.P.cols[j.probe_keys[k]];
  }
  a.n_build_dev = j.B.n_dev; a.n_build_cap = j.B.cap; a.n_probe_dev = j.P.n_dev; a.n_probe_cap = j.P.cap;
  a.probe_col_base = j.build_left ? L.n_cols : 0;
  a.has_filter = (u32)nd.shape;   // 0 none / 1 generic VM / 2 id (in)equality / 3 window
  if (nd.shape == 1) a.prog = upload_program(nd.prog);
  if (nd.shape == 2) { a.idp.a = nd.prog.nodes[0].u; a.idp.b = nd.prog.nodes[1].u; a.idp.is_eq = nd.prog.nodes[2].op == RDFGPU_EX_ID_EQ; }
  if (nd.shape == 3) {
    const rdfgpu_expr_node* e = nd.prog.nodes;
    a.win.x0 = e[0].u; a.win.y0 = e[2].u; a.win.x1 = e[8].u; a.win.y1 = e[10].u;
    a.win.l0 = window_literal(e, 0); a.win.l1 = window_literal(e, 8);
  }
  const NodeInfo* pf = j.probe_filter;
  a.has_probe_filter = pf ? (pf->shape == 1 ? 1u : 2u) : 0u;
  if (pf) {
    if (pf->shape == 1) {
      const rdfgpu_expr_node* e = pf->prog.nodes;
      a.pid.col = a.probe_col_base + e[0].u; a.pid.lit = e[1].u; a.pid.is_eq = e[2].op == RDFGPU_EX_ID_EQ;
    } else a.probe_prog = upload_program(pf->prog);
  }
  if (j.post_filter) {   // FilterExec of the build side's input, columns relative to that input
    const rdfgpu_expr_node* e = j.post_filter->prog.nodes;
    a.has_post = 1;
    a.post.col = (j.build_left ? 0 : L.n_cols) + e[0].u; a.post.lit = e[1].u; a.post.is_eq = e[2].op == RDFGPU_EX_ID_EQ;
  }
  a.tt = typed_table();
  a.stream_direct = opt.on(RDFGPU_OPT_NO_STREAM_JOIN) ? 0u : 1u;
  // columns the kernel reads on the probe side: keys ∪ projected ∪ filter columns
  bool pu[kMaxCols] = {}, bu[kMaxCols] = {};
  auto mark = [&](u32 c) { (on_build_side(a, c) ? bu : pu)[c < L.n_cols ? c : c - L.n_cols] = true; };
  for (u32 k = 0; k < a.n_keys; k++) pu[j.probe_keys[k]] = true;
  for (u32 c = 0; c < nd.n_proj; c++) mark(nd.proj[c]);
  for (u32 i = 0; i < nd.prog.n; i++) if (nd.prog.nodes[i].op == RDFGPU_EX_COLUMN) mark(nd.prog.nodes[i].u);
  if (pf) for (u32 i = 0; i < pf->prog.n; i++) if (pf->prog.nodes[i].op == RDFGPU_EX_COLUMN) pu[pf->prog.nodes[i].u] = true;
  for (u32 k = 0; k < a.n_keys; k++) bu[j.build_keys[k]] = false;
  for (bool b : pu) j.probe_cols += b;
  for (bool b : bu) j.build_payload += b;
  j.build_bytes = (4ull * (a.n_keys + j.build_payload) + 8) * j.B.cap;
}

// Which table the join probes, built now where it has to be: the kernels this triggers run here, before the probe.
JoinTable Plan::choose_join_table(LdsJoin& j) {
  const NodeInfo& nd = j.nd;
  const DevTable& B = j.B; const DevTable& P = j.P;
  LdsJoinArgs& a = j.a;
  u32& slots = j.slots;
  while (slots < 2 * B.cap) slots <<= 1;
  // LDS copy per workgroup vs ONE table in HBM/L2: the LDS form pays the build once per workgroup and, above
  // ~16 KiB of table, costs occupancy (a 128 KiB table = one workgroup per CU = latency-bound probes).
  const u64 lds_limit = std::min<u64>(opt.v[RDFGPU_OPT_LDS_MAX_BUILD], kLdsJoinMaxBuild);
  j.global_table = B.cap > lds_limit;
  // Every lane of a wave waits for the longest chain among its 64 probes, so short chains matter more than a
  // small table: LDS tables get load <= 0.25 and at least 2048 slots (16 KiB), HBM tables under 1 MiB load <= 0.125.
  if (!j.global_table) { while ((slots < 4 * B.cap || slots < 2048) && slots < 2 * kLdsJoinMaxBuild) slots <<= 1; }
  else { while (slots < 8 * B.cap && (u64)slots * sizeof(uint2) < (1u << 20)) slots <<= 1; }
  a.tbl_mask = slots - 1;
  if (!j.global_table) return JoinTable::Lds;
  // The HBM table of a build side that is a pure slice of the store (a param-free scan: label, simProperty…) is the
  // same for every plan until the store changes: it is built once per store version and kept on the store.
  if (B.stable_id != 0 && B.n_dev == nullptr && !opt.on(RDFGPU_OPT_NO_TABLE_CACHE)) {
    SliceKey sk; sk.n_keys = a.n_keys; sk.rows = B.cap;
    for (u32 k = 0; k < a.n_keys; k++) sk.key[k] = a.build_key[k];
    SliceTable* st = store->slice_table(sk);
    j.slice = st;
    std::unique_lock<std::mutex> building(store->slice_build_mu);
    // Dense forms first (one single key over a dense id range): direct-address if the keys are unique, CSR if not.
    // Decided once per slice; costs a few small kernels and host syncs at that time, nothing afterwards.
    if (!st->dense_tried && a.n_keys == 1 && !opt.on(RDFGPU_OPT_NO_DIRECT_TABLE)) build_dense_table(st, a.build_key[0], B.cap);
    if (st->csr_off) {
      a.csr_off = st->csr_off; a.csr_rows = st->csr_rows; a.direct_min = st->kmin; a.direct_n = st->kn;
      // lanes per probe row: a small probe side with a large fan-out is spread over the chip
      // (first execution: the table's mean rows per key stands in for the unknown fan-out)
      const u64 fan = nd.has_last ? nd.last_rows / (P.cap ? P.cap : 1) : B.cap / (st->kn ? st->kn : 1);
      // measured on the BSBM candidate join (fan-out 111): 8 lanes per row is best at 75 k and at 1.2 M probe rows alike
      // (a tiny probe side — a single query's constants — is latency-bound instead: spread each row over up to a whole wave)
      const bool tiny = P.cap < 4096;
      u32 rl = 0;
      while (rl < (tiny ? 6u : 3u) && ((tiny ? 2ull : 16ull) << rl) <= fan && (P.cap << (rl + 1)) <= (1ull << 25)) rl++;
      if (opt.v[RDFGPU_OPT_CSR_ROW_LANES_LOG2]) rl = (u32)std::min<u64>(6, opt.v[RDFGPU_OPT_CSR_ROW_LANES_LOG2] - 1);
      if (j.probe_outer) rl = 0;   // (one lane per probe row: the row's null-extended candidate is produced once)
      a.row_lanes_log2 = rl;
      return JoinTable::SliceCsr;
    }
    if (st->direct) { a.direct = st->direct; a.direct_min = st->kmin; a.direct_n = st->kn; return JoinTable::SliceDirect; }
    if (!st->slots || st->mask != a.tbl_mask) {   // build the hash form now, under the lock, and publish it only when complete
      if (st->slots) { store->table_free(st->slots); st->slots = nullptr; }
      void* mem = store->table_alloc<uint2>(slots);
      metrics.tables_built++;
      a.gslots = static_cast<uint2*>(mem);
      RDFGPU_HIP(hipMemsetAsync(a.gslots, 0xFF, (size_t)slots * sizeof(uint2), stream));
      timed(KC_GJOIN_BUILD, 0, B.cap, B.n_dev, 4ull * a.n_keys + 8, nullptr, 0, 0, [&] { launch_gjoin_build(a, stream); });
      RDFGPU_HIP(hipStreamSynchronize(stream)); metrics.host_syncs++;
      st->slots = mem; st->mask = a.tbl_mask;
    }
    a.gslots = static_cast<uint2*>(st->slots);
    return JoinTable::SliceHash;
  }
  if (a.n_keys <= 2 && !j.probe_filter && !j.post_filter && !opt.on(RDFGPU_OPT_NO_PARTITIONED_JOIN) && B.cap >= opt.v[RDFGPU_OPT_PARTITION_MIN_BUILD] &&
      B.cap < (1ull << 31) && P.cap < (1ull << 31))
    return JoinTable::Partitioned;
  // The direct-address form for a build side that is NOT cached (RDFGPU_OPT_NO_TABLE_CACHE, or an intermediate with a host-known row
  // count): built inside this execution, in scratch memory, when the single key turns out unique over a dense id range.  4 bytes per ID
  // instead of 8 bytes per SLOT at load <= 0.5: the 285 k-row property slices of BSBM-100M are 1.1 MB (resident in every XCD's L2)
  // instead of an 8 MB hash table that 0.54 G random probes fetch from the Infinity Cache line by line.  A large probe side pays for
  // the two host round trips with every probe that hits a 4-byte entry in L2 instead of an 8-byte slot beyond it.
  if (a.n_keys == 1 && B.n_dev == nullptr && B.cap >= 4096 && P.cap >= (1ull << 22) && !j.nd.transient_direct_failed && !opt.on(RDFGPU_OPT_NO_DIRECT_TABLE)) {
    const DirectTable d = build_direct(a.build_key[0], B.cap, 4 * B.cap + 1024, false);   // (sparse ids: not even tried)
    j.nd.transient_direct_failed = !d.direct;
    if (d.direct) { metrics.tables_built++; a.direct = d.direct; a.direct_min = d.kmin; a.direct_n = d.kn; return JoinTable::TransientDirect; }
  }
  a.gslots = scratch<uint2>(slots);   // (filled by the build pass in exec_lds_join)
  RDFGPU_HIP(hipMemsetAsync(a.gslots, 0xFF, (size_t)slots * sizeof(uint2), stream));
  return JoinTable::ScratchHash;
}

// Candidate queue per wave: a full queue costs one output reservation (a same-address atomic, ~88 per
// microsecond chip-wide), an oversized one costs occupancy (8 queues x 8 B x entries of LDS per workgroup).
// Sized from the matches a wave can expect out of one tile (64 x rows-per-lane probe rows), which is what a
// workgroup of an HBM-table join sees in its whole life; "expected" = the previous execution's cardinality
// when known, else one match per probe row.  A direct-address table has at most one match per row.
void Plan::size_wave_queue(LdsJoin& j) {
  const NodeInfo& nd = j.nd;
  const u64 np = j.P.cap;
  LdsJoinArgs& a = j.a;
  const u32 q_env = (u32)opt.v[RDFGPU_OPT_JOIN_WAVE_Q];
  const u64 per_tile = 64ull * (u64)lds_join_items(np << a.row_lanes_log2, j.global_table);
  const u64 expect = nd.has_last ? nd.last_rows : np;
  const u64 want = a.direct ? per_tile : (expect * per_tile * 3 / 2) / (np ? np : 1);
  u32 q = 256;
  while (q < want && q < 1024) q <<= 1;
  if (!j.global_table && (size_t)j.slots * sizeof(uint2) > 64 * 1024) q = 256;
  a.wave_q = q_env ? q_env : q;
  // partitioned join: a sparse output (the previous execution found less than one match per 8 probe rows) needs no deep queues —
  // 52 KB of LDS per workgroup instead of 64: three workgroups per CU instead of two
  if (j.table == JoinTable::Partitioned) a.wave_q = nd.has_last && !nd.last_scaled && nd.last_rows * 8 < np ? 64 : 256;
}

// One launch of the join kernel: the partitioned join, the streaming form over a direct table, or lds_join_kernel.  Bytes: the
// build side's when every workgroup builds the table, `stage_bytes` of a fused chain, `out_bytes_per_row` per output row.
void Plan::run_join_kernel(LdsJoin& j, u64 stage_bytes, u64 out_bytes_per_row) {
  LdsJoinArgs& a = j.a;
  const DevTable& B = j.B; const DevTable& P = j.P;
  // SURVEY 8d hash-join bytes of a partitioned join: both sides' key + payload columns and one 8-byte slot per row, the output;
  // the partition passes are in the time of the operator, not in its bytes
  if (j.table == JoinTable::Partitioned) {
    timed(KC_PART_JOIN, j.build_bytes, P.cap, P.n_dev, 4ull * j.probe_cols + 8, a.n_out_dev, 0, out_bytes_per_row, [&] { launch_part_join(a, j.part, stream); });
    return;
  }
  const bool streamed = a.stream_direct && direct_stream_join_ok(a);
  // the streaming form over a direct table, window filter on ONE build column against probe columns, a probe side large enough to pay
  // for a kernel and a host round trip: that column decoded per KEY (a.key_vals), once per execution
  if (streamed && !j.stream_values_tried && a.direct && a.has_filter == 3 && a.has_probe_filter == 0 && B.n_dev == nullptr && a.tt.n_ids != 0 &&
      direct_stream_join_items(P.cap) == 8 && P.cap >= (1ull << 22) && !opt.on(RDFGPU_OPT_NO_VALUE_TABLES)) {
    j.stream_values_tried = true;
    if (a.win.x0 == a.win.x1 && on_build_side(a, a.win.x0) && !on_build_side(a, a.win.y0) && !on_build_side(a, a.win.y1)) {
      long long* vals = scratch<long long>(a.direct_n);
      u32* bad = reinterpret_cast<u32*>(new_counter());
      launch_fill_i64(vals, INT64_MIN, a.direct_n, stream);
      launch_direct_values(a.build_key[0], a.cols[a.win.x0], B.cap, a.direct_min, a.direct_n, a.tt, vals, bad, stream);
      if (!read_back<u32>(bad)) {
        a.key_vals = vals; metrics.tables_built++;
        a.stream_need_build_row = (a.has_post && on_build_side(a, a.post.col)) ? 1u : 0u;
        for (u32 c = 0; c < j.nd.n_proj; c++) if (on_build_side(a, j.nd.proj[c])) a.stream_need_build_row = 1u;
      }
    }
  }
  const int kc = streamed ? (int)KC_STREAM_JOIN
                          : lds_join_class(a.has_filter, a.has_probe_filter, lds_join_items(P.cap << a.row_lanes_log2, j.global_table), lds_join_mode(a), a.n_chain != 0);
  timed(kc, (j.global_table ? 0 : j.build_bytes) + stage_bytes, P.cap, P.n_dev, 4ull * j.probe_cols + 8, a.n_out_dev, 0, out_bytes_per_row, [&] { launch_lds_join(a, stream); });
}

// Speculative mode: the output sized from history (`size_node`: this join's, or the top node's of a fused chain) or from the
// table form's guess; nothing is waited for.  j.use_band: the fused chain runs as a band join.
DevTable Plan::run_speculative(LdsJoin& j, u64 first_guess, NodeInfo& size_node) {
  LdsJoinArgs& a = j.a;
  DevTable& t = j.t;
  const u64 spec_cap = j.nd.has_last ? std::max<u64>(1024, size_node.last_rows + size_node.last_rows / (size_node.last_scaled ? 2 : 4) + 256)   // 25 % head room over the previous run (50 % over an extrapolation)
                                     : std::max<u64>(1024, first_guess);
  a.out_cap = spec_cap;
  for (u32 c = 0; c < a.n_out_cols; c++) { a.out[c] = scratch<u32>(spec_cap + j.tail); t.cols[c] = a.out[c]; }
  if (j.left_join) RDFGPU_HIP(hipMemsetAsync(a.visited, 0, j.L.cap, stream));
  if (j.use_band) exec_band_join(j);
  else if (!run_ordered_join(j, size_node, spec_cap)) run_join_kernel(j, j.stage_bytes, 4ull * a.n_out_cols);
  const SpecCheck check{&size_node, (u32)(a.n_out_dev - counters), j.left_join};
  if (pending_oj.active && !pending_oj.counted && pending_oj.o.n_out_dev == a.n_out_dev) pending_oj.check = check;   // nothing writes that count unless the count pass runs after all
  else spec_checks.push_back(check);
  t.cap = spec_cap + j.tail; t.n_dev = a.n_out_dev;
  if (j.left_join) left_join_tail(j.nd, j.L, j.R, a.out, a.visited, a.n_out_dev, spec_cap + j.tail);
  return t;
}

// A small table against a CSR slice that is sorted by another column, with an output about as large as the slice:
// the matches are emitted in the slice's order (ordered_join.hip) — what consumes them partitioned by that column
// (the band join above) then has nothing to sort; the chain's look-ups by table columns run once per table row.
// false: the join does not have that shape (nothing launched).
bool Plan::run_ordered_join(LdsJoin& j, const NodeInfo& size_node, u64 spec_cap) {
  const LdsJoinArgs& a = j.a;
  const DevTable& B = j.B; const DevTable& P = j.P;
  if (j.probe_outer || opt.on(RDFGPU_OPT_NO_ORDERED_JOIN) || !a.csr_off || a.range_rows || j.left_join || a.has_filter != 0 || a.has_probe_filter || a.has_post ||
      a.n_keys != 1 || B.sorted_col < 0 || (u32)B.sorted_col == j.build_keys[0] || B.n_dev || !B.stable_id || B.cap >= (1ull << 32) || P.cap > (1ull << 24) ||
      !size_node.has_last || size_node.last_rows * 8 < B.cap)
    return false;
  for (u32 s = 0; s < a.n_chain; s++) if (a.chain[s].key.src != 0 || a.chain[s].fs != 0) return false;
  u32 from_table = 0;   // output columns taken from the table row or a stage row travel in its packed record: at most 8
  for (u32 c = 0; c < a.n_out_cols; c++) from_table += a.n_chain ? a.chain_out[c].src != 1 : !on_build_side(a, a.proj[c]);
  if (from_table > 8 || a.n_out_cols > kOjMaxOutCols) return false;
  DevTable& t = j.t;
  OrderedJoinArgs o{};
  o.build_key = a.build_key[0]; o.n_build = B.cap;
  o.probe_key = a.probe_key[0]; o.n_probe_dev = P.n_dev; o.n_probe_cap = P.cap;
  o.kmin = a.direct_min; o.kn = a.direct_n;
  o.head = scratch<uint2>(a.direct_n); o.next = scratch<u32>(P.cap);
  RDFGPU_HIP(hipMemsetAsync(o.head, 0xFF, (size_t)a.direct_n * sizeof(uint2), stream));
  o.n_stages = a.n_chain;
  for (u32 s = 0; s < a.n_chain; s++) o.stage[s] = OrderedJoinStage{a.chain[s].key.ptr, a.chain[s].direct, a.chain[s].kmin, a.chain[s].kn, scratch<u32>(P.cap)};
  o.n_out_cols = a.n_out_cols;
  u32 n_words = 0;
  for (u32 c = 0; c < a.n_out_cols; c++) {
    if (a.n_chain) o.out_ref[c] = a.chain_out[c];
    else { const u32 pc = a.proj[c]; o.out_ref[c] = ColRef{a.cols[pc], on_build_side(a, pc) ? 1u : 0u, 0u}; }
    o.out[c] = a.out[c];
    o.out_slot[c] = o.out_ref[c].src == 1 ? (u8)0xFF : (u8)n_words++;
    if (o.out_ref[c].src == 1 && o.out_ref[c].ptr == B.cols[B.sorted_col] && t.sorted_col < 0) { t.sorted_col = (int)c; t.key_min = B.key_min; t.key_max = B.key_max; }
  }
  o.n_rec = n_words > 4 ? 2u : 1u;
  o.trec = scratch<uint4>(P.cap * o.n_rec);
  o.out_cap = spec_cap; o.n_out_dev = a.n_out_dev; o.overflow = a.overflow;
  // the consumer is a band join that (last time) found this output sorted by its key and needed nothing else of it: the write
  // pass is held back — that join has it write its row records instead of this table (exec_band_join), anything else flushes it.
  // If that join also read the slice's rows in place last time and no key had two table rows, the count pass waits as well:
  // the in-place records do not need it (OjInPlace); whatever else takes the table runs it first (count_pending_oj)
  const int consumer = size_node.parent;
  const bool held = consumer >= 0 && nodes[consumer].band.takes_records && !pending_oj.active && t.sorted_col >= 0;
  // (NO_BAND_COMPACT switches it off: the in-place records are the 16-byte ones)
  const bool in_place = held && nodes[consumer].band.in_place && nodes[consumer].band.multi_rows == 0 && !opt.on(RDFGPU_OPT_NO_BAND_COMPACT);
  if (held) o.multi_rows = reinterpret_cast<u32*>(new_counter());
  // (.. and with the rows' windows cached on the slice last time, only the table rows' output values travel by key)
  if (in_place && nodes[consumer].band.row_cache && !opt.on(RDFGPU_OPT_NO_BAND_ROW_CACHE)) o.key_val = scratch<u32>(a.direct_n);
  else if (in_place) o.key_rec = scratch<uint4>(a.direct_n);
  timed(KC_OJ_PROBE, 0, P.cap, P.n_dev, 8 + 12ull * a.n_chain, nullptr, 0, 0, [&] { launch_ordered_join_probe(o, stream); });
  if (!in_place) count_ordered_join(o);
  if (held) {
    pending_oj.active = true; pending_oj.o = o; pending_oj.first_col = a.out[0]; pending_oj.n_build = B.cap;
    pending_oj.counted = !in_place; pending_oj.rows_seen = size_node.last_rows;
  } else timed(KC_OJ_WRITE, 0, B.cap, nullptr, 4, a.n_out_dev, 0, 8ull * a.n_out_cols, [&] { launch_ordered_join_write(o, stream); });
  return true;
}

// Exact mode: the output sized from the table form, the count read back; a second attempt with room for all if it did not fit.
DevTable Plan::run_exact(LdsJoin& j) {
  NodeInfo& nd = j.nd;
  LdsJoinArgs& a = j.a;
  const DevTable& B = j.B; const DevTable& P = j.P;
  DevTable& t = j.t;
  u64 out_cap = P.cap < 1024 ? 1024 : P.cap;   // optimistic: at most one match per probe row on average
  if (a.csr_off) out_cap = std::max<u64>(out_cap, 2 * P.cap * ((B.cap + a.direct_n - 1) / (a.direct_n ? a.direct_n : 1)) + 1024);   // CSR: twice the mean rows per key
  u64 total = 0;
  for (int attempt = 0; attempt < 2; attempt++) {
    a.out_cap = out_cap;
    for (u32 c = 0; c < nd.n_proj; c++) { a.out[c] = scratch<u32>(out_cap + j.tail); t.cols[c] = a.out[c]; }
    if (j.left_join) RDFGPU_HIP(hipMemsetAsync(a.visited, 0, j.L.cap, stream));
    run_join_kernel(j, 0, 4ull * nd.n_proj);
    const u32 i0 = (u32)(a.n_out_dev - counters);
    read_back(ctx->counters_host + i0, counters + i0, 2 * sizeof(u64));
    total = ctx->counters_host[i0];
    const bool ovf = (ctx->counters_host[i0 + 1] & 0xFFFFFFFFull) != 0;
    if (!ovf) break;
    if (attempt == 1) fail(RDFGPU_ERR_DEVICE, "LDS join overflowed its exact-size output");
    out_cap = total;   // the count is exact even when the writes did not fit: run again with room for all
    RDFGPU_HIP(hipMemsetAsync(a.n_out_dev, 0, 2 * sizeof(u64), stream));
  }
  nd.last_rows = total; nd.has_last = true; nd.last_scaled = false;   // history for the next (speculative) execution
  t.cap = total + j.tail;
  if (!j.left_join) { if (total == 0) t.cap = 0; return t; }
  left_join_tail(nd, j.L, j.R, a.out, a.visited, a.n_out_dev, 0);
  t.n_dev = a.n_out_dev;
  return t;
}

// Left join tail: the build (left) rows no probe row visited, nulls on the right, appended at the device count `n_out_dev`.
// `matched_total`: the capacity of the output columns when the count is not known on the host (0 = unchecked).
void Plan::left_join_tail(const NodeInfo& nd, const DevTable& L, const DevTable& R, u32* const* out, u8* visited, u64* n_out_dev, u64 matched_total) {
  JoinArgs ja{};
  for (u32 c = 0; c < L.n_cols; c++) ja.left[c] = L.cols[c];
  ja.n_left_cols = L.n_cols; ja.n_right_cols = R.n_cols; ja.n_out_cols = nd.n_proj;
  for (u32 c = 0; c < nd.n_proj; c++) { ja.proj[c] = nd.proj[c]; ja.out[c] = out[c]; }
  ja.n_left_dev = L.n_dev; ja.n_left_cap = L.cap;
  ja.visited = visited; ja.n_out_dev = n_out_dev; ja.matched_total = matched_total;
  timed(KC_LEFT_TAIL, 0, L.cap, L.n_dev, 1, nullptr, 0, 0, [&] { launch_join_left_unmatched(ja, stream); });
}

// Radix partitioning of both sides of a HashJoinExec by the top bits of the key hash (part_join.hip): per side one pass
// that computes (partition, {row, key0, key1}) per row, one rocPRIM radix sort moving the 12-byte records, one pass that
// finds the partition boundaries.  Rows with a null key (NullEqualsNothing) or beyond the live row count ride in the last
// partition, marked (row = kNil) so that the join skips them.
void Plan::prepare_partitions(const LdsJoinArgs& a, const DevTable& B, const DevTable& P, PartArgs& pa) {
  u32 bits = 0;
  u32 target_rows = kPartTargetRows, part_slots = kPartSlots;
  // a join with a large output is bound by the latency of its gathers (part_join.hip, BIG): a 2048-slot table (24 KB) lets three
  // workgroups share a CU instead of two — 8.25 -> 7.5 ms on the 0.54 G-row candidate join of BSBM Q5 (profiles/tools/nc_variants.py)
  if (pa.two_pass) { part_slots = 2048; target_rows = 512; }
  if (opt.v[RDFGPU_OPT_PARTITION_SLOTS]) {
    const u64 v = opt.v[RDFGPU_OPT_PARTITION_SLOTS];
    if (v < 1024 || v > 8192 || (v & (v - 1))) fail(RDFGPU_ERR_INVALID, "PARTITION_SLOTS = %llu (a power of two from 1024 to 8192)", (unsigned long long)v);
    part_slots = (u32)v; target_rows = part_slots / 4;
  }
  if (opt.v[RDFGPU_OPT_PARTITION_ROWS]) target_rows = (u32)std::min<u64>(opt.v[RDFGPU_OPT_PARTITION_ROWS], part_slots / 2);
  while (bits < 16 && (B.cap >> bits) > target_rows) bits++;   // <= 16 bits = two radix passes; larger partitions are joined chunk by chunk
  const u32 n_parts = 1u << bits;
  pa.n_parts = n_parts; pa.chunk = part_slots / 2; pa.tbl_mask = part_slots - 1;
  // The probe side is a store slice sorted by one of the join keys (and every row of it is live): its partitions are KEY RANGES
  // of that column — contiguous pieces of the slice, found by one binary search per partition and read in place; only the
  // build side goes through the partition sort (LUBM Q9's closing join: 98 M of 327 M rows).
  PartKeyRange kr{-1, 0u, 0u, 0u, 0u, nullptr};
  if (!opt.on(RDFGPU_OPT_NO_RANGE_PARTITION) && P.sorted_col >= 0 && !P.n_dev && P.cap && P.key_min >= 1 && P.key_max >= P.key_min && n_parts >= 4)
    for (u32 k = 0; k < a.n_keys && kr.range < 0; k++)
      if (P.cols[P.sorted_col] == a.probe_key[k]) {
        // id ranges are not row ranges (LUBM: undergraduate and graduate courses share the slice, at different rows per id):
        // a coarse directory over the id range hands every bucket partitions in proportion to the slice rows in it
        const u64 span = (u64)P.key_max - P.key_min + 1;
        const u32 n_coarse = std::min<u32>(4096u, n_parts / 4);
        u32 cshift = 0;
        while (((span - 1) >> cshift) >= n_coarse) cshift++;
        uint2* dir = scratch<uint2>((u64)n_coarse + 1);
        kr = PartKeyRange{(int)k, P.key_min, P.key_max, cshift, n_coarse, dir};
        timed(KC_BAND_BOUNDS, 0, n_coarse, nullptr, 0, nullptr, 0, 0, [&] { launch_part_equalise(a.probe_key[k], P.cap, kr, n_parts, dir, stream); });
      }
  auto side = [&](const DevTable& T, const u32* const* keys, const PartRec*& recs, const u32*& start, PartKeyRange r) {
    const u64 n = T.cap;
    u32* st = scratch<u32>((u64)n_parts + 2);
    if (!opt.on(RDFGPU_OPT_NO_OWN_PARTITION_PASS)) {   // hand-written MSD passes that recompute the partition from the keys (part_pass.hip)
      const PartPassPlan pl = part_pass_plan(n, bits);
      PartPassBuffers w{};
      w.recs = scratch<PartRec>(n); w.recs_a = pl.two ? scratch<PartRec>(n) : nullptr;
      w.pid16 = scratch<unsigned short>(n); w.digit = pl.two ? scratch<unsigned char>(n) : nullptr;
      w.hist_a = scratch<u32>(pl.hist_a);
      w.total = scratch<u32>((u64)std::max<u32>(pl.nb_a, n_parts) + 2); w.base_a = scratch<u32>((u64)pl.nb_a + 2);
      if (pl.two) {
        w.hist_b = scratch<u32>(pl.hist_b);
        w.tiles_b = scratch<unsigned char>(pl.tile_desc_bytes); w.n_tiles_b = scratch<u32>(1);
      }
      w.tb = scratch<u32>((u64)pl.nb_a + 2);
      w.start = st;
      const size_t tb = scan_temp_bytes((u64)n_parts + 2);
      void* temp = scratch<unsigned char>(tb);
      timed(KC_PART_PASS, 0, n, T.n_dev, 0, nullptr, 0, 0, [&] { part_pass_run(w, pl, keys[0], a.n_keys > 1 ? keys[1] : nullptr, a.n_keys, T.n_dev, n, bits, n_parts, r, temp, tb, stream); });
      recs = w.recs; start = st;
      return;
    }
    u32* skey_in = scratch<u32>(n); u32* skey = scratch<u32>(n);
    PartRec* sval_in = scratch<PartRec>(n); PartRec* sval = scratch<PartRec>(n);
    const size_t tb = part_sort_temp_bytes(n, bits ? bits : 1);
    void* temp = scratch<unsigned char>(tb);
    timed(KC_PART_KEYS, 0, n, T.n_dev, 0, nullptr, 0, 0, [&] { launch_part_keys(keys[0], a.n_keys > 1 ? keys[1] : nullptr, a.n_keys, T.n_dev, n, bits, n_parts, r, skey_in, sval_in, stream); });
    timed(KC_RADIX_SORT, 0, n, nullptr, 0, nullptr, 0, 0, [&] { part_sort(skey_in, skey, sval_in, sval, n, bits ? bits : 1, temp, tb, stream); });
    timed(KC_BAND_BOUNDS, 0, n_parts, nullptr, 0, nullptr, 0, 0, [&] { launch_sorted_bounds(skey, n, n_parts, st, stream); });
    recs = sval; start = st;
  };
  side(B, a.build_key, pa.bpart, pa.bstart, kr);
  if (kr.range >= 0) {
    u32* st = scratch<u32>((u64)n_parts + 2);
    timed(KC_BAND_BOUNDS, 0, n_parts, nullptr, 0, nullptr, 0, 0, [&] { launch_part_range_bounds(a.probe_key[kr.range], P.cap, kr, n_parts, st, stream); });
    pa.ppart = nullptr; pa.pstart = st; pa.pcol0 = a.probe_key[0]; pa.pcol1 = a.n_keys > 1 ? a.probe_key[1] : nullptr;
  } else side(P, a.probe_key, pa.ppart, pa.pstart, kr);
}

// The fused chain as a key-partitioned band join (band_join.hip).  j.a is complete (chain, output columns, out_cap, counters), j.band holds what apply_chain
// resolved; everything allocated here is scratch of this execution.  Bytes recorded per kernel = what that kernel has to move once (compulsory).  The route flags
// (BandJoin says what each means) are all set here, before the first launch; in_place alone has to wait for band_slice_tables, which finds or builds the layout it needs.
void Plan::exec_band_join(LdsJoin& j) {
  BandJoin bj(j);
  BandHistory& hist = j.nd.band; const DevTable& P = j.P; const bool ordered = !opt.on(RDFGPU_OPT_NO_ORDERED_JOIN);
  bj.presorted = ordered && P.sorted_col >= 0 && P.cols[P.sorted_col] == j.a.probe_key[0] && P.key_min >= std::max<u32>(1u, j.a.direct_min);
  bj.skip_slow = speculative && hist.ran && hist.slow_rows == 0;   // a row that needs the pass after all is caught at the end of the plan like any failed speculation
  const u64 runs_seen = hist.run_stats & 0xFFFFFFFFull, run_rows = hist.run_stats >> 32;
  bj.counting = !bj.presorted && ordered && (bj.np <= (1ull << 21) || (runs_seen && run_rows >= 4 * runs_seen));
  bj.cache_entries = j.B.stable_id != 0 && !opt.on(RDFGPU_OPT_NO_TABLE_CACHE);
  // the packed pair test reads 8 bytes of window, the id operand and at most one output value per row: 16 bytes per row instead of 32 whenever no full-semantics pass will want the flags
  j.band.compact = (j.band.pack16 && j.band.n_row_cols <= 1 && bj.skip_slow && !opt.on(RDFGPU_OPT_NO_BAND_COMPACT)) ? 1u : 0u;
  bj.fused = take_pending_oj(bj);     // not fused: that join's write pass has run by now
  hist.takes_records = bj.presorted && bj.skip_slow && ordered;
  band_probe_side(bj);
  band_slice_tables(bj);
  hist.in_place = bj.lay.boff != nullptr;   // the layout exists: next time the ordered join below may leave its matches uncounted
  // In place: the ordered join below skipped its count pass, and the slice it streamed IS this join's build side.  Anything else counts the matches now and compacts them (the write-band pass).
  hist.row_cache = bj.row_win != nullptr;   // .. and its probe pass may prepare the values by key instead of the 16-byte records
  // (the ordered join prepared what the last execution's flags said: values by key when the windows were cached, records by key otherwise — a step whose
  // cached windows are gone, a non-integer operand having entered the store, counts and compacts once)
  bj.row_static = bj.fused && bj.row_win && pending_oj.o.key_val;
  bj.in_place = bj.fused && !pending_oj.counted && bj.fuse.self_index && hist.in_place && (bj.row_static || pending_oj.o.key_rec);
  bj.row_static = bj.row_static && bj.in_place;
  if (bj.fused && !bj.in_place) count_pending_oj();
  band_row_records(bj);
  band_blocks_and_emit(bj);
}

// The probe side is the held-back output of an ordered slice join (Plan::pending_oj).  true: everything this join reads of it travels in that join's packed
// table record and its key is the slice's sorted column, so that join writes this join's row records itself (bj.fuse).  Otherwise its write pass runs now.
bool Plan::take_pending_oj(BandJoin& bj) {
  if (!pending_oj.active) return false;
  const LdsJoinArgs& a = bj.j.a; const DevTable& B = bj.j.B; const DevTable& P = bj.j.P; BandArgs& b = bj.j.band; OjBandFuse& fuse = bj.fuse; const OrderedJoinArgs& o = pending_oj.o;
  bool ok = bj.presorted && bj.skip_slow && P.cols[0] == pending_oj.first_col && P.n_cols == o.n_out_cols;
  auto slot_of = [&](const u32* col, u8& slot) {      // the word of the packed record that holds output column `col`
    slot = 0xFFu;
    for (u32 c = 0; c < o.n_out_cols; c++) if (o.out[c] == col && o.out_slot[c] != 0xFFu) { slot = o.out_slot[c]; return true; }
    return false;
  };
  fuse.y0_slot[0] = fuse.y0_slot[1] = fuse.y1_slot[0] = fuse.y1_slot[1] = fuse.neq_slot = fuse.row_slot[0] = fuse.row_slot[1] = 0xFFu;
  for (u32 w = 0; ok && w < b.n_win; w++) ok = slot_of(b.win[w].y0, fuse.y0_slot[w]) && slot_of(b.win[w].y1, fuse.y1_slot[w]);
  if (ok && b.has_neq) ok = slot_of(b.neq_probe, fuse.neq_slot);
  for (u32 u = 0; ok && u < b.n_row_cols; u++) ok = slot_of(b.row_col[u], fuse.row_slot[u]);
  for (u32 c = 0; ok && c < o.n_out_cols; c++) if (o.out[c] == a.probe_key[0] && o.out_slot[c] == 0xFFu && o.out_ref[c].src == 1) fuse.key_col = o.out_ref[c].ptr;
  if (!ok || fuse.key_col == nullptr) { flush_pending_oj(); return false; }
  fuse.compact = b.compact;   // (16 bytes per match instead of 32)
  // self_index, `entry id != row id` by entry index: the band join's groups are the rows of the very slice the ordered join streamed (same sorted column, same rows, identity CSR),
  // the entry's id is that join's build key, the row's id its probe key — equal keys are what made the match, and a store slice holds every (key, sorted column) pair once:
  // the only entry of the group whose id equals the row's is the slice row the match came from
  if (fuse.compact && b.has_neq && !b.neq_is_eq && a.csr_rows == nullptr && a.build_key[0] == fuse.key_col && B.cap == pending_oj.n_build &&
      b.neq_build == o.build_key && B.stable_id != 0 && !opt.on(RDFGPU_OPT_NO_BAND_COMPACT))
    for (u32 c = 0; c < o.n_out_cols; c++)
      if (o.out[c] == b.neq_probe && o.out_slot[c] != 0xFFu && o.out_ref[c].src == 0 && o.out_ref[c].ptr == o.probe_key) fuse.self_index = 1;
  b.neq_self = fuse.self_index;
  return true;
}

// The kernel arguments that repeat the LDS join's (table, probe side, output), and what partitions the probe rows by the key: the counting
// sort's key histogram or the radix sort's pairs and temp, the unsorted rows' records, the two counts the row passes leave behind.
void Plan::band_probe_side(BandJoin& bj) {
  const LdsJoinArgs& a = bj.j.a; BandArgs& b = bj.j.band;
  if (bj.counting) {
    b.key_hist = scratch<u32>((u64)bj.kn + 2); b.key_cursor = scratch<u32>((u64)bj.kn + 2);
    RDFGPU_HIP(hipMemsetAsync(b.key_hist, 0, ((size_t)bj.kn + 2) * sizeof(u32), stream));
  }
  b.presorted = bj.presorted ? 1u : 0u; b.tt = a.tt;
  b.csr_off = a.csr_off; b.csr_rows = a.csr_rows; b.kmin = a.direct_min; b.kn = bj.kn; b.n_entries = bj.nb;
  b.probe_key = a.probe_key[0]; b.n_probe_dev = bj.j.P.n_dev; b.n_probe_cap = bj.np;
  b.n_out_cols = a.n_out_cols; b.out_cap = a.out_cap; b.n_out_dev = a.n_out_dev; b.overflow = a.overflow; for (u32 c = 0; c < a.n_out_cols; c++) b.out[c] = a.out[c];
  b.skey = bj.skey = scratch<u32>(bj.np); b.perm = bj.perm = scratch<u32>(bj.np);
  if (bj.presorted) { b.skey_in = bj.skey; b.sval_in = bj.perm; b.rec = nullptr; }
  else { b.skey_in = scratch<u32>(bj.np); b.sval_in = scratch<u32>(bj.np); b.rec = scratch<uint4>((b.compact ? 1 : 2) * bj.np); }
  b.slow_rows = reinterpret_cast<u32*>(new_counter()); b.run_stats = reinterpret_cast<unsigned long long*>(new_counter());
  while ((1ull << bj.sort_bits) <= bj.kn) bj.sort_bits++;            // keys 0 .. kn (kn = joins nothing)
  bj.sort_temp_bytes = sort_u32_temp_bytes(bj.np, bj.sort_bits); bj.sort_temp = scratch<unsigned char>(bj.sort_temp_bytes);
}

// The two tables a band join keeps on its build slice's SliceTable (per store version, like every other join table): found or built under
// ONE hold of the lock, taken only when they are kept at all; each is published only once the stream has been waited for, and the layout is
// copied before the lock goes.  bj.ekey: the bytes the decoded entries depend on, the store's slices and the chain's constants.
void Plan::band_slice_tables(BandJoin& bj) {
  const BandArgs& b = bj.j.band;
  auto put = [&](const void* p, size_t n) { bj.ekey.append(reinterpret_cast<const char*>(p), n); };
  put(&b.csr_off, sizeof b.csr_off); put(&b.csr_rows, sizeof b.csr_rows); put(&b.kmin, 4); put(&b.kn, 4); put(&b.n_stages, 4); put(&b.n_win, 4);
  for (u32 t = 0; t < b.n_stages; t++) put(&b.stage[t], sizeof(BandStage));
  for (u32 w = 0; w < b.n_win; w++) { put(&b.win[w].key_col, sizeof(void*)); put(&b.win[w].val, sizeof(void*)); put(&b.win[w].vkmin, 4); put(&b.win[w].vkn, 4); put(&b.win[w].vbase, 8); }
  put(&b.has_post, 4); put(&b.post_lit, 4); put(&b.post_is_eq, 4); put(&b.post_col, sizeof(void*)); put(&b.has_neq, 4); put(&b.neq_build, sizeof(void*));
  put(&b.n_entry_cols, 4); for (u32 u = 0; u < b.n_entry_cols; u++) { put(&b.entry_col[u].ptr, sizeof(void*)); put(&b.entry_col[u].src, 4); }
  put(&bj.nb, 8);
  std::unique_lock<std::mutex> building(store->slice_build_mu, std::defer_lock);
  if (bj.cache_entries) building.lock();
  band_entries(bj);
  if (const SliceTable::BandEntries* layout = band_layout(bj)) bj.lay = *layout;
  band_row_windows(bj);
}

// The build side's decoded entries (the pair test's operands, the entries' output values), found on the slice's table (keys are unique there: an entry is
// pushed only after a failed look-up under the same lock) or built: a steady-state step does not decode 5.4 M build rows again.  The caller holds the lock when bj.cache_entries.
void Plan::band_entries(BandJoin& bj) {
  const LdsJoinArgs& a = bj.j.a; BandArgs& b = bj.j.band; SliceTable* tab = bj.j.slice;
  if (bj.cache_entries) for (const auto& e : tab->band_entries) if (e.key == bj.ekey) { b.et = e.et; for (u32 u = 0; u < b.n_entry_cols; u++) b.eo[u] = e.eo[u]; return; }
  // stages all keyed by one build column: their look-ups once per distinct key value instead of once per entry
  const u32* kc = a.n_chain ? b.stage[0].key_col : nullptr;
  bool same = kc != nullptr; u64 lo = ~0ull, hi = 0;
  for (u32 t = 0; t < b.n_stages; t++) { same = same && b.stage[t].key_col == kc; lo = std::min<u64>(lo, b.stage[t].kmin); hi = std::max<u64>(hi, (u64)b.stage[t].kmin + b.stage[t].kn); }
  for (u32 w = 0; w < b.n_win; w++) same = same && b.win[w].key_col == kc;
  if (same && hi > lo && hi - lo <= (64ull << 20) && hi - lo <= 8 * bj.nb + 1024) {
    b.pt_min = (u32)lo; b.pt_n = (u32)(hi - lo); b.pt_key_col = kc; b.pt = scratch<uint4>(2ull * b.pt_n);
    timed(KC_BAND_PT, 0, b.pt_n, nullptr, 4ull * b.n_stages + 8ull * b.n_win + 4ull * b.n_entry_cols + 32, nullptr, 0, 0, [&] { launch_band_pt(b, stream); });
  }
  // the build side, once: per row its columns + stage look-ups read, 16 B of operands + the output values written
  u64 entry_bytes = 4ull * (1 + bj.j.build_payload) + (a.csr_rows ? 4 : 0) + (a.has_post ? 4 : 0);
  for (u32 t = 0; t < a.n_chain; t++) entry_bytes += 4 + (a.chain[t].val ? 8 : 0);
  const bool own_entries = bj.cache_entries && tab->band_entries.size() < 8;   // kept on the slice, else scratch of this execution
  b.et = own_entries ? store->table_alloc<uint4>(bj.nb + 64) : scratch<uint4>(bj.nb + 64);   // padded: the pair test reads whole groups of 8 entries
  for (u32 u = 0; u < b.n_entry_cols; u++) b.eo[u] = own_entries ? store->table_alloc<u32>(bj.nb) : scratch<u32>(bj.nb);
  timed(KC_BAND_ENTRIES, 0, bj.nb, bj.j.B.n_dev, entry_bytes + 4ull * b.n_entry_cols + 16 + 4ull * b.n_entry_cols, nullptr, 0, 0, [&] { launch_band_entries(b, stream); });
  if (own_entries) {   // publish only when complete
    RDFGPU_HIP(hipStreamSynchronize(stream)); metrics.host_syncs++; metrics.tables_built++;
    SliceTable::BandEntries e{bj.ekey, b.et, {nullptr, nullptr, nullptr, nullptr}};
    for (u32 u = 0; u < b.n_entry_cols; u++) e.eo[u] = b.eo[u];
    tab->band_entries.push_back(e);
  }
}

// In place: the band join's rows of key k are the CSR group k itself (poff = csr_off), so its blocks depend on the slice alone — laid out once per store version beside the
// entries (same key, same lock), their exact number read back, published when complete; by the first execution that could take the route, so that the first one that does finds
// them.  The route pays for every slice row, matched or not, and for ceil(E/64)² blocks per key: it is taken when the ordered join's last measured rows cover at least half of the
// slice, and when the block count, bounded here in 64 bits (sum over keys of ceil(E/64)² <= cmax · (rows / 64 + keys)), stays below 2^31 — the device counts in 32.
// Null: the route is not available (entries that could not be cached among the reasons: the counted route); a layout returned has its boff.
SliceTable::BandEntries* Plan::band_layout(BandJoin& bj) {
  const LdsJoinArgs& a = bj.j.a; const u32 kn = bj.kn;
  SliceTable::BandEntries* layout = nullptr;
  if (bj.fused && bj.fuse.self_index && bj.cache_entries && bj.cmax * (bj.nb / 64 + kn) < (1ull << 31) && pending_oj.rows_seen * 2 >= bj.nb)
    for (auto& e : bj.j.slice->band_entries) if (e.key == bj.ekey) layout = &e;
  if (layout && !layout->boff) {
    u32* boff = store->table_alloc<u32>((u64)kn + 1);
    const size_t tb = band_blocks_scan_temp_bytes(kn); void* temp = scratch<unsigned char>(tb);
    timed(scan_class((u64)kn + 1), 12ull * kn, (u64)kn + 1, nullptr, 4, nullptr, 0, 0, [&] { band_blocks_scan(a.csr_off, a.csr_off, kn, boff, temp, tb, stream); });
    const u32 n = read_back<u32>(boff + kn);
    BandArgs d = bj.j.band; d.poff = const_cast<u32*>(a.csr_off); d.boff = boff; d.bdesc = store->table_alloc<uint4>(n); d.max_blocks = n; d.n_blocks_out = nullptr;
    timed(KC_BAND_DESC, 12ull * kn, 0, nullptr, 0, nullptr, 0, 0, [&] { launch_band_desc(d, stream); });
    RDFGPU_HIP(hipStreamSynchronize(stream)); metrics.host_syncs++;
    layout->boff = boff; layout->bdesc = d.bdesc; layout->n_blocks = n; metrics.tables_built++;
  }
  return layout;
}

// In place, the ROW side of the pair test as a table of the slice: when both operands of every window are reached from the ordered join's key alone
// (host_logic.hpp, band_row_cache_eligible) a slice row's windows are a function of the store and the plan's literals — decoded once per store version beside
// the entries (same lock; built where the layout is, by the first execution that could take the route; fewer than 8 per slice), not gathered as 16-byte records
// by key every step.  Its key = the entries' key + everything band_row_record reads.  A store in which some key's operands are not plain xsd:integers declines
// the form: remembered as an entry without a table.  The caller holds the lock (the layout exists only when bj.cache_entries).
void Plan::band_row_windows(BandJoin& bj) {
  const BandArgs& b = bj.j.band; const OjBandFuse& fuse = bj.fuse; const OrderedJoinArgs& o = pending_oj.o; SliceTable* tab = bj.j.slice;
  if (!bj.lay.boff) return;                              // the in-place route is closed
  BandRowWinArgs w{}; BandRowCacheShape shape;
  shape.in_place = true; shape.compact = fuse.compact != 0 && b.compact != 0; shape.pack16 = b.pack16 != 0;
  shape.option_off = !opt.on(RDFGPU_OPT_NO_BAND_ROW_CACHE); shape.n_win = b.n_win;
  auto operand = [&](u8 slot, BandRowOperand& op, BandRowOperandShape& sh) {   // the ordered join's output column held in word `slot` of its packed record
    for (u32 c = 0; c < o.n_out_cols; c++) {
      if (slot == 0xFFu || o.out_slot[c] != slot) continue;
      const ColRef ref = o.out_ref[c];
      sh.src = ref.src;
      if (ref.src >= 2 && ref.src - 2 < o.n_stages) {
        const OrderedJoinStage& st = o.stage[ref.src - 2];
        sh.stage_keyed_by_join_key = st.key_col == o.probe_key;
        op = BandRowOperand{st.direct, st.kmin, st.kn, ref.ptr};
      }
      return;
    }
  };
  for (u32 k = 0; k < b.n_win && k < 2; k++) { operand(fuse.y0_slot[k], w.y0[k], shape.y0[k]); operand(fuse.y1_slot[k], w.y1[k], shape.y1[k]); }
  if (!band_row_cache_eligible(shape)) return;
  std::string key = bj.ekey;
  auto put = [&](const void* p, size_t n) { key.append(reinterpret_cast<const char*>(p), n); };
  for (u32 k = 0; k < b.n_win; k++) {
    put(&b.win[k].l0, sizeof(TvLiteral)); put(&b.win[k].l1, sizeof(TvLiteral)); put(&b.win[k].vbase, 8);
    for (const BandRowOperand* op : {&w.y0[k], &w.y1[k]}) { put(&op->direct, sizeof(void*)); put(&op->kmin, 4); put(&op->kn, 4); put(&op->val, sizeof(void*)); }
  }
  put(&b.pack16, 4); put(&b.has_neq, 4); put(&b.tt.tv, sizeof(void*)); put(&b.tt.n_ids, sizeof b.tt.n_ids);
  put(&o.build_key, sizeof(void*)); put(&o.kmin, 4); put(&o.kn, 4);
  for (const auto& e : tab->band_row_windows) if (e.key == key) { bj.row_win = e.row_win; return; }
  if (tab->band_row_windows.size() >= 8) return;
  w.kmin = o.kmin; w.kn = o.kn; w.by_key = scratch<uint2>(o.kn); w.slow_keys = reinterpret_cast<u32*>(new_counter());
  w.build_key = o.build_key; w.n_rows = bj.nb; w.row_win = store->table_alloc<uint2>(bj.nb + 64);
  // per key: two look-ups, two ids and two typed values per window read, 8 B written; per slice row: its key read, 8 B gathered and written
  timed(KC_BAND_ROW_WIN_KEYS, 0, o.kn, nullptr, 48ull * b.n_win + 8, nullptr, 0, 0, [&] { launch_band_row_win_keys(b, w, stream); });
  timed(KC_BAND_ROW_WIN_ROWS, 0, bj.nb, nullptr, 4 + 8 + 8, nullptr, 0, 0, [&] { launch_band_row_win_rows(w, stream); });
  const u32 slow = read_back<u32>(w.slow_keys);          // (the wait: published only when complete)
  if (slow) { store->table_free(w.row_win); w.row_win = nullptr; } else metrics.tables_built++;
  tab->band_row_windows.push_back(SliceTable::BandRowWindows{key, w.row_win});
  bj.row_win = w.row_win;
}

// The probe rows' records in key order, with the rows per key (poff) and the blocks' counts zeroed: written by the ordered slice join below (fused; in place: one per slice row), else decoded from the probe columns.
void Plan::band_row_records(BandJoin& bj) {
  const LdsJoinArgs& a = bj.j.a; BandArgs& b = bj.j.band; OjBandFuse& fuse = bj.fuse;
  const u32 kn = bj.kn; const u64 np = bj.np, nb = bj.nb; const bool in_place = bj.in_place;
  bj.nrows = in_place ? nb : np; b.rec_s = bj.row_static ? nullptr : scratch<uint4>(bj.nrows); b.aux_s = b.compact ? nullptr : scratch<uint4>(bj.nrows);
  b.poff = in_place ? const_cast<u32*>(a.csr_off) : scratch<u32>((u64)kn + 2);
  // blocks: sum over keys of ceil(E/64) * ceil(R/64) <= cmax * (rows / 64) + sum of ceil(E/64) over the keys
  bj.max_blocks = in_place ? bj.lay.n_blocks : bj.cmax * (np / 64 + 1) + nb / 64 + kn + 1;
  if (bj.max_blocks >= (1ull << 31)) fail(RDFGPU_ERR_UNSUPPORTED, "band join of %llu blocks", (unsigned long long)bj.max_blocks);
  b.max_blocks = (u32)bj.max_blocks; b.bcount = scratch<u32>(bj.max_blocks + 1); b.bofs = scratch<u32>(bj.max_blocks + 1);   // (bcount is zeroed by the decode pass: a memset is two more launches, ~10 us of launch gap each on this part)
  // decode, per probe row: key + the window operands + the id operand read, 24 B of record + 8 B of sort pair written
  if (!bj.fused) return timed(KC_BAND_DECODE, 0, np, bj.j.P.n_dev, 4 + 4ull * (b.n_win + b.has_neq) + 9ull * b.n_win + 24 + 8, nullptr, 0, 0, [&] { launch_band_decode(b, stream); });
  const OrderedJoinArgs& o = pending_oj.o; pending_oj.active = false;
  fuse.key_rec = in_place && !bj.row_static ? o.key_rec : nullptr;
  if (bj.row_static) { u32* row_val = scratch<u32>(nb); fuse.key_val = o.key_val; fuse.row_val = row_val; b.row_win = bj.row_win; b.row_val = row_val; }
  fuse.brec = in_place ? nullptr : scratch<uint4>((fuse.compact ? 1 : 2) * o.n_probe_cap);
  fuse.rec_s = b.rec_s; fuse.aux_s = b.aux_s; fuse.poff = b.poff; fuse.bcount = b.bcount; fuse.max_blocks = b.max_blocks; fuse.kmin = b.kmin; fuse.kn = b.kn;
  // per table row: its packed record read + two typed-value gathers + 32 B written; per slice row the count pass's 5 bytes + its key; per match a 32-byte record gathered and stored (in place: per slice row its key read, its key's 16-byte record gathered and stored)
  // (the rows' windows cached: per table row its packed record read and 4 B written by key; per slice row its key read, 4 B gathered, 4 B written)
  const u64 rec_bytes = fuse.compact ? 16 : 32;
  timed(KC_OJ_BAND_RECORDS, 0, o.n_probe_cap, o.n_probe_dev, bj.row_static ? 16ull * o.n_rec + 4 : 16ull * o.n_rec + 9ull * b.n_win + rec_bytes, nullptr, 0, 0, [&] { launch_oj_band_records(o, b, fuse, stream); });
  if (in_place) timed(KC_OJ_WRITE_BAND_IN_PLACE, 0, nb, nullptr, bj.row_static ? 4 + 4 + 4 : 4 + 2 * rec_bytes, nullptr, 0, 0, [&] { launch_ordered_join_write_band(o, fuse, OjInPlace{}, stream); });
  else timed(KC_OJ_WRITE_BAND, 0, pending_oj.n_build, nullptr, 4 + 1 + 4, a.n_probe_dev, 0, 2 * rec_bytes, [&] { launch_ordered_join_write_band(o, fuse, stream); });
}

// The blocks (64 entries x 64 rows) and what runs over them.  First the radix sort of a probe side that came neither sorted nor small (in the time, not in the algorithmic bytes:
// SURVEY 8d), the blocks' buffers, the launch of the block kernels sized from the previous execution's count (+ 25 %), not from the upper bound (in place: exactly), where this execution
// leaves its own counts, the rows per key and the blocks of every key laid out; then the pair test, the full-semantics pass where rows may need it, the scan of the blocks' counts, the output rows.
void Plan::band_blocks_and_emit(BandJoin& bj) {
  const LdsJoinArgs& a = bj.j.a; BandArgs& b = bj.j.band;
  const u32 kn = bj.kn; const u64 np = bj.np, nb = bj.nb, max_blocks = bj.max_blocks;
  if (!bj.presorted && !bj.counting) timed(KC_RADIX_SORT, 0, np, nullptr, 0, nullptr, 0, 0, [&] { sort_pairs_u32_u32(b.skey_in, bj.skey, b.sval_in, bj.perm, np, bj.sort_bits, bj.sort_temp, bj.sort_temp_bytes, stream); });
  b.boff = bj.in_place ? bj.lay.boff : scratch<u32>((u64)kn + 1); b.n_blocks_out = new_counter();
  // the multi-row count is the ordered join's (pending_oj.o stays as it was when that join was taken over); a band join that was not fused has none
  band_feedback.push_back({&bj.j.nd, (u32)(b.n_blocks_out - counters), (u32)(reinterpret_cast<u64*>(b.slow_rows) - counters), (u32)(reinterpret_cast<u64*>(b.run_stats) - counters),
                           bj.fused ? (int)(reinterpret_cast<u64*>(pending_oj.o.multi_rows) - counters) : -1, bj.skip_slow, bj.in_place, bj.in_place ? max_blocks : 0});
  const u64 hist = bj.j.nd.band.blocks; b.launch_blocks = (u32)(bj.in_place ? max_blocks : std::min<u64>(max_blocks, hist ? hist + hist / 4 + 1024 : max_blocks));
  b.bdesc = bj.in_place ? bj.lay.bdesc : scratch<uint4>(max_blocks); b.masks = scratch<u64>(max_blocks * 64);
  const size_t tb = std::max(scan_temp_bytes(std::max<u64>((u64)kn + 1, max_blocks + 1)), band_blocks_scan_temp_bytes(kn)); void* temp = scratch<unsigned char>(tb);
  if (bj.counting) {   // poff = exclusive scan of the rows per key (entry kn = the rows that join something); then the scatter
    timed(scan_class((u64)kn + 1), 0, (u64)kn + 1, nullptr, 8, nullptr, 0, 0, [&] { exclusive_scan_u32(b.key_hist, b.poff, (u64)kn + 1, temp, tb, stream); });
    RDFGPU_HIP(hipMemcpyAsync(b.key_cursor, b.poff, ((size_t)kn + 1) * sizeof(u32), hipMemcpyDeviceToDevice, stream));
    timed(KC_BAND_ROWS, 0, np, bj.j.P.n_dev, 8 + 32 + 32, nullptr, 0, 0, [&] { launch_band_scatter(b, stream); });
  } else if (!bj.presorted) timed(KC_BAND_BOUNDS, 0, np, nullptr, 4, nullptr, 0, 0, [&] { launch_band_bounds(bj.skey, np, kn, b.poff, stream); });   // (presorted: the decode pass wrote poff)
  if (!bj.in_place) {
    timed(scan_class((u64)kn + 1), 12ull * kn, (u64)kn + 1, nullptr, 4, nullptr, 0, 0, [&] { band_blocks_scan(a.csr_off, b.poff, kn, b.boff, temp, tb, stream); });   // (blocks per key: the scan's input iterator)
    timed(KC_BAND_DESC, 12ull * kn, 0, nullptr, 0, nullptr, 0, 0, [&] { launch_band_desc(b, stream); });
  }
  if (!bj.presorted && !bj.counting) timed(KC_BAND_ROWS, 0, np, bj.j.P.n_dev, 4 + 32 + 32, nullptr, 0, 0, [&] { launch_band_rows(b, stream); });
  // pair test, per probe row 4 (sorted position) + 24 (record) read, per entry 16 B read, per pair one bit written; the pair count is not known on the host
  const u64* const nrows_dev = bj.in_place ? nullptr : bj.j.P.n_dev;
  timed(KC_BAND_MASK, 16ull * nb, bj.nrows, nrows_dev, bj.row_static ? 8 + 4 : b.compact ? 16 : 4 + 24, nullptr, 0, 0, [&] { launch_band_mask(b, stream); });
  if (!bj.skip_slow) {
    // the full-semantics pass needs the chain's literals and columns: the fused join kernel's argument block, by pointer
    static_assert(sizeof(LdsJoinArgs) <= ExecContext::kArgBytes, "argument staging slot too small");
    const u32 slot = arg_slots_used++;
    LdsJoinArgs* a_host = reinterpret_cast<LdsJoinArgs*>(ctx->args_host + (size_t)slot * ExecContext::kArgBytes);
    LdsJoinArgs* a_dev = reinterpret_cast<LdsJoinArgs*>(ctx->args_dev + (size_t)slot * ExecContext::kArgBytes);
    *a_host = a; RDFGPU_HIP(hipMemcpyAsync(a_dev, a_host, sizeof(LdsJoinArgs), hipMemcpyHostToDevice, stream));
    timed(KC_BAND_SLOW, 0, 0, nullptr, 0, nullptr, 0, 0, [&] { launch_band_slow(a_dev, b, stream); });
  }
  timed(scan_class(max_blocks + 1), 0, max_blocks + 1, nullptr, 8, nullptr, 0, 0, [&] { exclusive_scan_u32(b.bcount, b.bofs, max_blocks + 1, temp, tb, stream); });
  timed(KC_BAND_EMIT, 4ull * b.n_entry_cols * nb, bj.nrows, nrows_dev, 4 + 4ull * b.n_row_cols, a.n_out_dev, 0, 4ull * a.n_out_cols, [&] { launch_band_emit(b, stream); });
}

void Plan::ensure_host_copy() {
  if (host_valid) return;
  if (!executed) fail(RDFGPU_ERR_INVALID, "plan has not been executed");
  store->activate();
  host_cols.assign(result.n_cols, std::vector<u32>());
  for (u32 c = 0; c < result.n_cols; c++) {
    host_cols[c].resize(result_rows);
    if (result_rows) RDFGPU_HIP(hipMemcpyAsync(host_cols[c].data(), result.cols[c], result_rows * 4, hipMemcpyDeviceToHost, stream));
  }
  host_aggs.assign(agg_out.size(), std::vector<rdfgpu_agg_value>());
  for (size_t i = 0; i < agg_out.size(); i++) {
    host_aggs[i].resize(result_rows);
    if (result_rows) RDFGPU_HIP(hipMemcpyAsync(host_aggs[i].data(), agg_out[i], result_rows * sizeof(rdfgpu_agg_value), hipMemcpyDeviceToHost, stream));
  }
  RDFGPU_HIP(hipStreamSynchronize(stream));
  host_valid = true;
}

}  // namespace rdfgpu
