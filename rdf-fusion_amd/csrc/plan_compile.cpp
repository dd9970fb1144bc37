// plan_compile.cpp — plan compilation (host): the description is checked, its string table compiled, the join order rewritten.
//
// What replaces what (reference paths relative to the rdf-fusion tree):
//   plan_compile            MemQuadStorePlanner::plan_extension  lib/storage/src/memory/planner.rs:31-64
//                           + plan_pattern_evaluation             storage/snapshot.rs:84-131
#include "plan_exec.hpp"
#include "regex_compile.hpp"

namespace rdfgpu {

namespace {

// Type-checks a postfix program against `n_cols` input columns; returns the kind it leaves.  `value_cols`: bit c = input column c is an
// aggregate value column (RDFGPU_PLAN_AGG_COLUMNS) — COLUMN of it is a VK_VALUE, which only ENC_TV and BOUND take: its u32 is an index, so
// whatever compares or prints ids (ID_EQ, ID_NEQ, IS_COMPATIBLE, STR) would answer about the index.
u32 check_program(const rdfgpu_expr_node* p, u32 n, u32 n_cols, u32 n_regexes = 0, u32 value_cols = 0) {
  if (n > (u32)kMaxExpr) fail(RDFGPU_ERR_UNSUPPORTED, "expression has %u nodes (max %d)", n, kMaxExpr);
  u32 st[kMaxStack]; bool no_bytes[kMaxStack]; int sp = 0;
  bool views = false, rank_only_string = false;   // computed strings (an op with kOpView) / a string literal given by its rank in the dictionary only
  bool out_no_bytes = false;                      // the value being pushed is such a literal: it has no lexical form on the device
  auto pop = [&](u32 kind, const char* what) {
    if (sp < 1) fail(RDFGPU_ERR_INVALID, "expression: stack underflow at %s", what);
    if (st[sp - 1] == VK_VALUE && kind == VK_ID) fail(RDFGPU_ERR_INVALID, "expression: %s got an aggregate value column, whose entries are not object ids (ENC_TV and BOUND read one)", what);
    if (st[--sp] != kind) fail(RDFGPU_ERR_INVALID, "expression: %s got an operand of the wrong kind", what);
  };
  // an operand whose BYTES the op reads (REGEX / CONTAINS / STRSTARTS / STRENDS / STRLEN / SUBSTR / UCASE / LCASE): a string literal
  // that came with its rank only would be the error value on every row — refused here, loudly, instead
  auto pop_id_or_value = [&](const char* what) {   // ENC_TV / BOUND: an object id, or a value column's entry
    if (sp >= 1 && st[sp - 1] == VK_VALUE) { --sp; return; }
    pop(VK_ID, what);
  };
  auto pop_bytes = [&](const char* what) {
    if (sp >= 1 && no_bytes[sp - 1]) fail(RDFGPU_ERR_UNSUPPORTED, "%s over a string literal given by its dictionary rank only: it has no lexical form on the device (pass it as RDFGPU_EX_LIT_STR)", what);
    pop(VK_TV, what);
  };
  for (u32 i = 0; i < n; i++) {
    const rdfgpu_expr_node& e = p[i];
    u32 out;
    out_no_bytes = false;
    if (op_is(e.op, kOpSlot) && e.u >= n_regexes) {   // a slot of the plan's string table: the text names what the op keeps there
      const bool constant = e.op == RDFGPU_EX_LIT_STR, langs = e.op == RDFGPU_EX_LANG_IN;
      fail(RDFGPU_ERR_INVALID, "expression: %s %u out of range (%u %s)", constant ? "string constant" : langs ? "language table" : "REGEX pattern", e.u, n_regexes,
           constant ? "entries" : langs ? "tables" : "patterns");
    }
    views = views || op_is(e.op, kOpView);
    switch (e.op) {
      case RDFGPU_EX_COLUMN: if (e.u >= n_cols) fail(RDFGPU_ERR_INVALID, "expression: column %u out of range (%u columns)", e.u, n_cols);
        out = e.u < 32 && ((value_cols >> e.u) & 1u) ? VK_VALUE : VK_ID; break;
      case RDFGPU_EX_LIT_ID: out = VK_ID; break;
      case RDFGPU_EX_LIT_TV: if (e.tag > RDFGPU_TV_OTHER) fail(RDFGPU_ERR_INVALID, "expression: bad literal tag %u", e.tag); out = VK_TV;
        out_no_bytes = e.tag == RDFGPU_TV_STRING && e.hi == 0;
        rank_only_string = rank_only_string || out_no_bytes; break;
      case RDFGPU_EX_LIT_BOOL: out = VK_BOOL; break;
      case RDFGPU_EX_ENC_TV: pop_id_or_value("ENC_TV"); out = VK_TV; break;
      case RDFGPU_EX_GT: case RDFGPU_EX_LT: case RDFGPU_EX_GEQ: case RDFGPU_EX_LEQ: case RDFGPU_EX_EQ: case RDFGPU_EX_NEQ:
      case RDFGPU_EX_ADD: case RDFGPU_EX_SUB: case RDFGPU_EX_MUL: case RDFGPU_EX_DIV: pop(VK_TV, "binary typed op"); pop(VK_TV, "binary typed op"); out = VK_TV; break;
      case RDFGPU_EX_NEG: case RDFGPU_EX_PLUS: case RDFGPU_EX_ABS: case RDFGPU_EX_ROUND: case RDFGPU_EX_CEIL: case RDFGPU_EX_FLOOR:
        pop(VK_TV, "unary numeric op"); out = VK_TV; break;
      case RDFGPU_EX_YEAR: case RDFGPU_EX_MONTH: case RDFGPU_EX_DAY: case RDFGPU_EX_HOURS: case RDFGPU_EX_MINUTES: case RDFGPU_EX_SECONDS:
        pop(VK_TV, "date part (YEAR .. SECONDS)"); out = VK_TV; break;
      case RDFGPU_EX_CAST: case RDFGPU_EX_CAST_LEX: {   // CAST_LEX reads the bytes of a simple literal, CAST none
        const bool lex = e.op == RDFGPU_EX_CAST_LEX;
        const char* what = lex ? "CAST_LEX" : "CAST";
        if (!is_cast_target(e.u)) fail(RDFGPU_ERR_UNSUPPORTED, "expression: %s to tag %u (on the device: boolean, int, integer, decimal, float, double)", what, e.u);
        if (lex) pop_bytes(what); else pop(VK_TV, what);
        out = VK_TV; break; }
      case RDFGPU_EX_CAST_STRING: pop(VK_ID, "CAST_STRING (xsd:string)"); out = VK_TV; break;
      // IF / COALESCE hand an operand on: a string literal given by rank among them still has no bytes where the result is read
      case RDFGPU_EX_IF:
        out_no_bytes = sp >= 2 && (no_bytes[sp - 1] || no_bytes[sp - 2]);
        pop(VK_TV, "IF branch"); pop(VK_TV, "IF branch"); pop(VK_TV, "IF test (a typed value: BOOLEAN_AS_TERM(EBV(..)) for the EBV)"); out = VK_TV; break;
      case RDFGPU_EX_COALESCE: {   // `u` operands of one kind, typed values or object ids
        if (e.u < 1 || e.u > (u32)kMaxStack) fail(RDFGPU_ERR_INVALID, "expression: COALESCE takes 1 to %d operands, not %u", kMaxStack, e.u);
        if ((u32)sp < e.u) fail(RDFGPU_ERR_INVALID, "expression: stack underflow at COALESCE");
        const u32 kind = st[sp - 1] == VK_TV ? VK_TV : VK_ID;
        for (u32 k = 0; k < e.u; k++) {
          if (st[sp - 1] == VK_VALUE) pop(VK_ID, "COALESCE");   // (refused with the text of a value column read as an object id)
          if (st[sp - 1] != kind) fail(RDFGPU_ERR_INVALID, "expression: COALESCE mixes operand kinds (all typed values or all object ids)");
          out_no_bytes = out_no_bytes || no_bytes[sp - 1];
          pop(kind, "COALESCE");
        }
        out = kind; break; }
      case RDFGPU_EX_IS_IRI: case RDFGPU_EX_IS_BLANK: case RDFGPU_EX_IS_LITERAL: case RDFGPU_EX_IS_NUMERIC:
        pop(VK_TV, "term test (isIRI / isBlank / isLiteral / isNumeric)"); out = VK_TV; break;
      case RDFGPU_EX_EBV: pop(VK_TV, "EBV"); out = VK_BOOL; break;
      case RDFGPU_EX_REGEX: case RDFGPU_EX_CONTAINS: case RDFGPU_EX_STRSTARTS: case RDFGPU_EX_STRENDS:
        // (the operand is any string value: ENC_TV of a column, or a view — STR / SUBSTR / UCASE / LCASE / a constant with bytes)
        pop_bytes("REGEX / CONTAINS / STRSTARTS / STRENDS"); out = VK_TV; break;
      case RDFGPU_EX_STR: pop(VK_ID, "STR"); out = VK_TV; break;
      case RDFGPU_EX_LIT_STR: out = VK_TV; break;
      case RDFGPU_EX_STRLEN: pop_bytes("STRLEN"); out = VK_TV; break;
      case RDFGPU_EX_SUBSTR:
        if (e.u != 2 && e.u != 3) fail(RDFGPU_ERR_INVALID, "expression: SUBSTR takes 2 or 3 operands, not %u", e.u);
        for (u32 k = 0; k + 1 < e.u; k++) pop(VK_TV, "SUBSTR position / length");
        pop_bytes("SUBSTR");
        out = VK_TV; break;
      case RDFGPU_EX_UCASE: case RDFGPU_EX_LCASE: pop_bytes("UCASE / LCASE"); out = VK_TV; break;
      case RDFGPU_EX_STRBEFORE: case RDFGPU_EX_STRAFTER: pop_bytes("STRBEFORE / STRAFTER"); pop_bytes("STRBEFORE / STRAFTER"); out = VK_TV; break;
      case RDFGPU_EX_REGEX_VAR:
        if (e.lo < 1 || (u64)e.u + (u64)e.lo > n_regexes) fail(RDFGPU_ERR_INVALID, "expression: REGEX pattern table %u .. +%lld out of range (%u patterns)", e.u, (long long)e.lo, n_regexes);
        pop(VK_TV, "REGEX pattern"); pop_bytes("REGEX"); out = VK_TV; break;
      case RDFGPU_EX_LANG_IN: pop(VK_TV, "LANGMATCHES(LANG())"); out = VK_TV; break;
      case RDFGPU_EX_ID_EQ: case RDFGPU_EX_ID_NEQ: case RDFGPU_EX_IS_COMPATIBLE: pop(VK_ID, "id comparison"); pop(VK_ID, "id comparison"); out = VK_BOOL; break;
      case RDFGPU_EX_AND: case RDFGPU_EX_OR: pop(VK_BOOL, "AND/OR"); pop(VK_BOOL, "AND/OR"); out = VK_BOOL; break;
      case RDFGPU_EX_NOT: pop(VK_BOOL, "NOT"); out = VK_BOOL; break;
      case RDFGPU_EX_BOUND: pop_id_or_value("BOUND"); out = VK_BOOL; break;
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

// A program with a value load, a lexical cast, a date part, a functional form (IF / COALESCE) or a term test in it runs in the generic VM:
// the specialised forms gather from the typed-value table by object id and know the ops of their shape only.
bool needs_generic_vm(const ExprProgram& pr) { return program_has(pr, kOpGenericVm); }

int detect_shape(const ExprProgram& pr, bool force_vm) {
  if (force_vm || needs_generic_vm(pr)) return 0;
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
  if (force_vm || needs_generic_vm(pr)) return 1;
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

// The schema an operator's program and projection see: its input's columns (a join's: left, then right) with their value origins.
struct InputSchema {
  u32 n = 0; ValueOrigin origin[2 * kMaxCols];
  void append(const NodeInfo& c) { for (u32 k = 0; k < c.width && n < 2u * kMaxCols; k++) origin[n++] = c.origin[k]; }
  u32 value_cols() const { u32 m = 0; for (u32 k = 0; k < n; k++) if (origin[k].node >= 0) m |= 1u << k; return m; }
};

// ENC_TV of a value column becomes the value load of its origin.  (The operand of ENC_TV is a leaf, COLUMN or LIT_ID: the node before it.)
void rewrite_value_loads(ExprProgram& pr, const InputSchema& in) {
  for (u32 i = 1; i < pr.n; i++) {
    rdfgpu_expr_node& e = pr.nodes[i];
    const rdfgpu_expr_node& c = pr.nodes[i - 1];
    if (e.op != RDFGPU_EX_ENC_TV || c.op != RDFGPU_EX_COLUMN || c.u >= in.n || in.origin[c.u].node < 0) continue;
    e.op = kExAggValue; e.u = ((u32)in.origin[c.u].node << 8) | in.origin[c.u].agg;
  }
}

// `len` checked nodes as a program of the plan: the plan's string table attached, the ENC_TV of a value column made its value load.
ExprProgram load_value_program(const Plan* plan, const InputSchema& in, const rdfgpu_expr_node* nodes, u32 len) {
  ExprProgram pr{};
  pr.n = len;
  std::memcpy(pr.nodes, nodes, len * sizeof(rdfgpu_expr_node));
  pr.regex = plan->regex_dev; pr.str_consts = plan->str_consts_dev;
  rewrite_value_loads(pr, in);
  return pr;
}

// The predicate of a FilterExec or a join (none: an empty program).
void load_program(NodeInfo& nd, const Plan* plan, const rdfgpu_plan_desc* d, const InputSchema& in, const char* what) {
  const rdfgpu_plan_node& r = nd.d;
  nd.prog.n = 0;
  if (r.expr_len == 0) return;
  if ((u64)r.expr_off + r.expr_len > d->n_exprs) fail(RDFGPU_ERR_INVALID, "%s: expression outside the expression array", what);
  if (check_program(d->exprs + r.expr_off, r.expr_len, in.n, d->n_regexes, in.value_cols()) != VK_BOOL) fail(RDFGPU_ERR_INVALID, "%s: predicate does not yield a boolean", what);
  nd.prog = load_value_program(plan, in, d->exprs + r.expr_off, r.expr_len);
}

void load_projection(NodeInfo& nd, const rdfgpu_plan_desc* d, const InputSchema& in, const char* what) {
  const rdfgpu_plan_node& r = nd.d;
  const u32 full = in.n;
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
  for (u32 i = 0; i < nd.n_proj; i++) nd.origin[i] = in.origin[nd.proj[i]];   // a projected value column keeps its origin
}

// The operators that compare, sort, chain or decode ids refuse a value column: equal values have different indexes.
void refuse_value_column(const ValueOrigin& o, u32 node, const char* role, u32 column) {
  if (o.node >= 0 && o.mark)
    fail(RDFGPU_ERR_UNSUPPORTED, "node %u: %s column %u is a mark column (of the LeftMark join, node %d): its entries index values (1 = false, 2 = true), they are not object ids", node, role, column, o.node);
  if (o.node >= 0 && o.extend)
    fail(RDFGPU_ERR_UNSUPPORTED, "node %u: %s column %u is a computed value column (expression %u of the ProjectionExec with expressions, node %d): its entries index values, equal values have different indexes", node, role, column, o.agg, o.node);
  if (o.node >= 0)
    fail(RDFGPU_ERR_UNSUPPORTED, "node %u: %s column %u is an aggregate value column (aggregate %u of node %d): its entries index values, equal values have different indexes", node, role, column, o.agg, o.node);
}

// The op that uses each entry of the plan's string table (-1: none): the use decides how the entry is compiled.
std::vector<int> string_table_uses(const rdfgpu_plan_desc* d) {
  std::vector<int> use(d->n_regexes, -1);
  for (u32 i = 0; i < d->n_exprs; i++) {
    const rdfgpu_expr_node& e = d->exprs[i];
    if (e.op == RDFGPU_EX_REGEX_VAR) {   // a table of per-row patterns: entries u .. u + lo, all REGEX patterns
      for (int64_t k = 0; k < e.lo && (u64)e.u + (u64)k < d->n_regexes; k++) use[e.u + k] = RDFGPU_EX_REGEX;
      continue;
    }
    if (!op_is(e.op, kOpSlot)) continue;
    if (e.u >= d->n_regexes) fail(RDFGPU_ERR_INVALID, "expression: string pattern %u out of range", e.u);
    if (use[e.u] >= 0 && use[e.u] != (int)e.op) fail(RDFGPU_ERR_INVALID, "string pattern %u is used by two different functions", e.u);
    use[e.u] = (int)e.op;
  }
  return use;
}

// Entry `r` as a matcher: REGEX (and an unused entry) = a pattern with its flags; CONTAINS / STRSTARTS / STRENDS = a literal needle (like
// the `q` flag), anchored at the start / end for the latter two.
void compile_pattern(u32 r, const rdfgpu_regex& rx, int use, RegexProg& prog) {
  std::string why;
  const bool literal = use >= 0 && op_is((u32)use, kOpNeedle);
  const char* flags = literal ? "q" : (rx.flags ? rx.flags : "");
  const size_t n_flags = literal ? 1 : (rx.flags ? rx.flags_len : 0);
  if (regex_compile(rx.pattern ? rx.pattern : "", rx.pattern_len, flags, n_flags, prog, why) != REGEX_OK)
    fail(RDFGPU_ERR_UNSUPPORTED, "string pattern %u: %s", r, why.c_str());
  prog.pattern_id = rx.pattern_id;
  if (use == RDFGPU_EX_STRSTARTS) prog.anchor_start = 1;
  if (use == RDFGPU_EX_STRENDS) prog.anchor_end = 1;
}

// The plan's string table (REGEX patterns, needles, language sets, string constants): compiled by use, kept as texts, uploaded.
void compile_string_table(Plan* plan, const rdfgpu_plan_desc* d) {
  Store* store = plan->store;
  if (!d->regexes) fail(RDFGPU_ERR_INVALID, "plan_compile: %u regexes but no table", d->n_regexes);
  const std::vector<int> use = string_table_uses(d);
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
    compile_pattern(r, rx, use[r], progs[r]);
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

// String functions that need no table entry still need the store's strings.
void check_string_functions(const Store* store, const rdfgpu_plan_desc* d) {
  for (u32 i = 0; i < d->n_exprs; i++) {
    if (op_is(d->exprs[i].op, kOpStoreStrings) && !store->str_off)
      fail(RDFGPU_ERR_INVALID, "plan uses string functions but the store has no strings (rdfgpu_store_set_strings)");
  }
}

// Input `c` of node `i`: an earlier node, and — unless aggregate values are columns (RDFGPU_PLAN_AGG_COLUMNS) — no AggregateExec that carries them.
const NodeInfo& child(const Plan* plan, u32 i, int32_t c, const char* what) {
  if (c < 0 || (u32)c >= i) fail(RDFGPU_ERR_INVALID, "node %u: %s child %d must precede the node", i, what, c);
  if (!plan->agg_columns && plan->nodes[c].d.kind == RDFGPU_NODE_AGGREGATE && plan->nodes[c].n_aggs)   // aggregate values are not object ids
    fail(RDFGPU_ERR_UNSUPPORTED, "node %u: input %d is an AggregateExec with aggregates, which must be the plan's root", i, c);
  return plan->nodes[c];
}

// HashJoinExec / CrossJoinExec / NestedLoopJoinExec: join type, keys, widths, filter, projection.
void compile_join(Plan* plan, const rdfgpu_plan_desc* d, u32 i) {
  NodeInfo& nd = plan->nodes[i];
  const rdfgpu_plan_node& r = nd.d;
  const NodeInfo& l = child(plan, i, r.left, "left");
  const NodeInfo& rr = child(plan, i, r.right, "right");
  const bool semi = r.join_type == RDFGPU_JOIN_LEFT_SEMI || r.join_type == RDFGPU_JOIN_LEFT_ANTI;
  const bool mark = r.join_type == RDFGPU_JOIN_LEFT_MARK && r.kind != RDFGPU_NODE_CROSS_JOIN;
  if (r.join_type != RDFGPU_JOIN_INNER && r.join_type != RDFGPU_JOIN_LEFT && !semi && r.join_type != RDFGPU_JOIN_LEFT_MARK) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: join type %u", i, r.join_type);
  if (mark && !plan->agg_columns) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: a LeftMark join outputs its mark as a value column, which is not an object id: the plan must be compiled with RDFGPU_PLAN_AGG_COLUMNS", i);
  if (r.kind == RDFGPU_NODE_HASH_JOIN) {
    if (r.n_keys == 0 || r.n_keys > RDFGPU_MAX_KEYS) fail(RDFGPU_ERR_INVALID, "node %u: HashJoinExec needs 1..%u keys", i, RDFGPU_MAX_KEYS);
    for (u32 k = 0; k < r.n_keys; k++) {
      if (r.left_keys[k] >= l.width || r.right_keys[k] >= rr.width) fail(RDFGPU_ERR_INVALID, "node %u: join key out of range", i);
      refuse_value_column(l.origin[r.left_keys[k]], i, "left join key", r.left_keys[k]);
      refuse_value_column(rr.origin[r.right_keys[k]], i, "right join key", r.right_keys[k]);
    }
  }
  if (r.kind == RDFGPU_NODE_CROSS_JOIN && (r.expr_len || r.join_type != RDFGPU_JOIN_INNER)) fail(RDFGPU_ERR_INVALID, "node %u: CrossJoinExec takes no filter / join type", i);
  if (l.width + rr.width > 2u * kMaxCols) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: too many columns", i);
  InputSchema both, left;
  both.append(l); both.append(rr); left.append(l);
  load_program(nd, plan, d, both, "join filter");
  // a semi / anti join outputs the left columns only: its projection indexes them (the filter still sees both sides)
  // .. and a mark join the left columns and the mark: a value column whose origin is this node
  if (mark) {
    if (left.n >= 2u * kMaxCols) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: too many columns", i);
    left.origin[left.n] = ValueOrigin{(int)i, 0, false, true};
    left.n++;
  }
  load_projection(nd, d, semi || mark ? left : both, "join");
  nd.shape = detect_join_filter_shape(nd.prog, plan->opt.on(RDFGPU_OPT_FORCE_GENERIC_VM));
  if (l.width > (u32)kMaxCols || rr.width > (u32)kMaxCols) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: too many columns", i);
}

// TopK: sort keys, fetch, group column; the output may carry only what DISTINCT is over.
void compile_topk(Plan* plan, const rdfgpu_plan_desc* d, u32 i) {
  NodeInfo& nd = plan->nodes[i];
  const rdfgpu_plan_node& r = nd.d;
  const NodeInfo& c = child(plan, i, r.left, "input");
  if (r.n_keys < 1 || r.n_keys > RDFGPU_MAX_KEYS) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: TopK with %u sort keys (1 to %u)", i, r.n_keys, RDFGPU_MAX_KEYS);
  if (r.table_cols < 1 || r.table_cols > 1024) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: TopK fetch = %u", i, r.table_cols);
  for (u32 k = 0; k < r.n_keys; k++) {
    if (r.left_keys[k] >= c.width) fail(RDFGPU_ERR_INVALID, "node %u: sort key column %u out of range", i, r.left_keys[k]);
    if (r.right_keys[k] > RDFGPU_SORT_BY_DOUBLE) fail(RDFGPU_ERR_INVALID, "node %u: unknown sort mode %u", i, r.right_keys[k]);
    refuse_value_column(c.origin[r.left_keys[k]], i, "TopK sort key", r.left_keys[k]);
  }
  if (r.table_slot > c.width) fail(RDFGPU_ERR_INVALID, "node %u: group column out of range", i);
  if (r.table_slot != 0) refuse_value_column(c.origin[r.table_slot - 1], i, "TopK group", r.table_slot - 1);
  InputSchema in; in.append(c);
  load_projection(nd, d, in, "TopK");
  for (u32 q = 0; q < nd.n_proj; q++) refuse_value_column(nd.origin[q], i, "TopK output", nd.proj[q]);
  for (u32 q = 0; q < nd.n_proj; q++) {   // DISTINCT is over (group, keys): the output may not carry anything else
    bool covered = r.table_slot != 0 && nd.proj[q] == r.table_slot - 1;
    for (u32 k = 0; k < r.n_keys; k++) covered = covered || (nd.proj[q] == r.left_keys[k] && r.right_keys[k] == RDFGPU_SORT_BY_ID);
    if (!covered) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: TopK output column %u is neither the group nor a sort key by id", i, nd.proj[q]);
  }
  nd.width = nd.n_proj;
}

// AggregateExec: group columns, then every aggregate's function and input (a column, or an expression that is loaded here).
void compile_aggregate(Plan* plan, const rdfgpu_plan_desc* d, u32 i) {
  NodeInfo& nd = plan->nodes[i];
  const rdfgpu_plan_node& r = nd.d;
  const NodeInfo& c = child(plan, i, r.left, "input");
  // RDFGPU_PLAN_VALUE_KEYS: up to RDFGPU_MAX_GROUP_KEYS group columns (4.. in right_keys[]), value columns among them; without the flag every
  // refusal is what it was
  const u32 max_keys = plan->value_keys ? RDFGPU_MAX_GROUP_KEYS : RDFGPU_MAX_KEYS;
  if (r.n_keys > max_keys) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: AggregateExec with %u group columns (at most %u)", i, r.n_keys, max_keys);
  if (r.table_cols > RDFGPU_MAX_AGGREGATES) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: AggregateExec with %u aggregates (at most %u)", i, r.table_cols, RDFGPU_MAX_AGGREGATES);
  if (r.n_proj != RDFGPU_NO_PROJECTION) fail(RDFGPU_ERR_INVALID, "node %u: AggregateExec takes no projection", i);
  if (r.n_keys + r.table_cols == 0) fail(RDFGPU_ERR_INVALID, "node %u: AggregateExec without group columns and aggregates", i);
  InputSchema in; in.append(c);
  for (u32 k = 0; k < r.n_keys; k++) {
    const u32 col = agg_key_col(r, k);
    if (col >= c.width) fail(RDFGPU_ERR_INVALID, "node %u: group column %u out of range", i, col);
    if (!plan->value_keys) refuse_value_column(c.origin[col], i, "group", col);
    else nd.origin[k] = c.origin[col];   // a value key stays a value column with its input's origin: the representative row's entry indexes the same array
  }
  if (r.table_cols && ((u64)r.table_slot + 2ull * r.table_cols > d->n_pool || !d->pool)) fail(RDFGPU_ERR_INVALID, "node %u: aggregate list outside the pool", i);
  for (u32 a = 0; a < r.table_cols; a++) {
    const u32 fn = d->pool[r.table_slot + 2 * a], col = d->pool[r.table_slot + 2 * a + 1];
    const bool expr = fn != RDFGPU_AGG_COUNT_STAR && (col & RDFGPU_AGG_INPUT_EXPR) != 0;
    switch (fn) {
      case RDFGPU_AGG_COUNT_STAR: break;
      case RDFGPU_AGG_COUNT: case RDFGPU_AGG_COUNT_DISTINCT:
        if (expr) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: aggregate %u: COUNT / COUNT DISTINCT over an expression is not on the device (SUM and AVG are)", i, a);
        [[fallthrough]];
      case RDFGPU_AGG_MIN: case RDFGPU_AGG_MAX:   // with value columns only (RDFGPU_PLAN_AGG_COLUMNS), like RDFGPU_NODE_EXTEND: an input like SUM's
      case RDFGPU_AGG_SUM: case RDFGPU_AGG_AVG:
        if ((fn == RDFGPU_AGG_MIN || fn == RDFGPU_AGG_MAX) && !plan->agg_columns)
          fail(RDFGPU_ERR_UNSUPPORTED, "node %u: aggregate %u: MIN / MAX / SAMPLE / GROUP_CONCAT are not on the device (MIN / MAX keep the first "
                                       "value's error state, min.rs:42-53: their result depends on row order)", i, a);   // (the text every plan without the flag has always met)
        if (expr) {   // (expr_off, expr_len) in the pool: a program over the input's columns that leaves a typed value
          const u32 at = col & ~RDFGPU_AGG_INPUT_EXPR;
          if ((u64)at + 2 > d->n_pool) fail(RDFGPU_ERR_INVALID, "node %u: aggregate %u: expression input at pool offset %u of %u", i, a, at, d->n_pool);
          const u32 off = d->pool[at], len = d->pool[at + 1];
          if (len == 0 || (u64)off + len > d->n_exprs) fail(RDFGPU_ERR_INVALID, "node %u: aggregate %u: expression outside the expression array", i, a);
          if (any_op_is(d->exprs + off, len, kOpPattern))   // the pattern ops get their per-node preparation in FilterExec and the joins only
            fail(RDFGPU_ERR_UNSUPPORTED, "node %u: aggregate %u: REGEX / CONTAINS / STRSTARTS / STRENDS / LANGMATCHES in an aggregate's input expression are not on the device", i, a);
          if (check_program(d->exprs + off, len, c.width, d->n_regexes, in.value_cols()) != VK_TV) fail(RDFGPU_ERR_INVALID, "node %u: aggregate %u: the input expression does not yield a typed value", i, a);
          nd.agg_prog[a] = (int)nd.agg_progs.size();
          nd.agg_progs.push_back(load_value_program(plan, in, d->exprs + off, len));
        } else if (col >= c.width) fail(RDFGPU_ERR_INVALID, "node %u: aggregate %u reads column %u of %u", i, a, col, c.width);
        else if (fn == RDFGPU_AGG_COUNT_DISTINCT) refuse_value_column(c.origin[col], i, "COUNT DISTINCT input", col);
        else if (c.origin[col].node >= 0 && fn != RDFGPU_AGG_COUNT) {
          // SUM / AVG / MIN / MAX of a value column: the two-node program [COLUMN, value load], so the EXPR form of the accumulate pass runs it.
          // (COUNT needs nothing: an entry of 0 is "not counted" already.)
          rdfgpu_expr_node load[2] = {};
          load[0].op = RDFGPU_EX_COLUMN; load[0].u = col;
          load[1].op = RDFGPU_EX_ENC_TV;
          nd.agg_prog[a] = (int)nd.agg_progs.size();
          nd.agg_progs.push_back(load_value_program(plan, in, load, 2));
        }
        break;
      case RDFGPU_AGG_SAMPLE: case RDFGPU_AGG_GROUP_CONCAT:
        if (plan->agg_columns) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: aggregate %u: SAMPLE / GROUP_CONCAT are not on the device", i, a);
        fail(RDFGPU_ERR_UNSUPPORTED, "node %u: aggregate %u: MIN / MAX / SAMPLE / GROUP_CONCAT are not on the device (MIN / MAX keep the first "
                                     "value's error state, min.rs:42-53: their result depends on row order)", i, a);
      case RDFGPU_AGG_SUM_DISTINCT: case RDFGPU_AGG_AVG_DISTINCT: case RDFGPU_AGG_COUNT_DISTINCT_STAR:
        fail(RDFGPU_ERR_UNSUPPORTED, "node %u: aggregate %u: SUM / AVG with DISTINCT and COUNT(DISTINCT *) are not on the device", i, a);
      default: fail(RDFGPU_ERR_INVALID, "node %u: aggregate %u: unknown function %u", i, a, fn);
    }
    nd.agg_fn[a] = fn; nd.agg_col[a] = fn == RDFGPU_AGG_COUNT_STAR || expr ? 0 : col;
  }
  nd.n_aggs = r.table_cols;
  if (!plan->agg_columns) {
    if (nd.n_aggs && i != d->root) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: an AggregateExec with aggregates must be the plan's root (node %u)", i, d->root);
    nd.width = r.n_keys;   // the id columns; the aggregates leave through rdfgpu_plan_agg_*
    return;
  }
  // RDFGPU_PLAN_AGG_COLUMNS: the keys, then one value column per aggregate, each its own origin
  nd.width = r.n_keys + nd.n_aggs;
  if (nd.width > (u32)kMaxCols) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: AggregateExec with %u output columns (max %d)", i, nd.width, kMaxCols);
  for (u32 a = 0; a < nd.n_aggs; a++) nd.origin[r.n_keys + a] = ValueOrigin{(int)i, a};
}

// ProjectionExec with expressions (RDFGPU_NODE_EXTEND): the kept columns, then one value column per program — each checked like an
// aggregate's input expression, over all of the input's columns.
void compile_extend(Plan* plan, const rdfgpu_plan_desc* d, u32 i) {
  NodeInfo& nd = plan->nodes[i];
  const rdfgpu_plan_node& r = nd.d;
  if (!plan->agg_columns) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: a ProjectionExec with expressions outputs value columns, which are not object ids: the plan must be compiled with RDFGPU_PLAN_AGG_COLUMNS", i);
  const NodeInfo& c = child(plan, i, r.left, "input");
  const u32 k = r.table_cols;
  if (k < 1 || k > RDFGPU_MAX_AGGREGATES) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: ProjectionExec with %u expressions (1 to %u)", i, k, RDFGPU_MAX_AGGREGATES);
  InputSchema in; in.append(c);
  load_projection(nd, d, in, "ProjectionExec with expressions");
  if (nd.n_proj + k > (u32)kMaxCols) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: ProjectionExec with expressions: %u output columns (max %d)", i, nd.n_proj + k, kMaxCols);
  if ((u64)r.table_slot + 2ull * k > d->n_pool || !d->pool) fail(RDFGPU_ERR_INVALID, "node %u: expression list outside the pool", i);
  for (u32 q = 0; q < k; q++) {
    const u32 off = d->pool[r.table_slot + 2 * q], len = d->pool[r.table_slot + 2 * q + 1];
    if (len == 0 || (u64)off + len > d->n_exprs) fail(RDFGPU_ERR_INVALID, "node %u: expression %u: program outside the expression array", i, q);
    // the pattern ops get their per-node preparation in FilterExec and the joins only; a string view has no 24-byte form
    if (any_op_is(d->exprs + off, len, kOpPattern | kOpStringFn))
      fail(RDFGPU_ERR_UNSUPPORTED, "node %u: expression %u: REGEX / CONTAINS / STRSTARTS / STRENDS / LANGMATCHES and the string functions in a computed column are not on the device", i, q);
    const u32 kind = check_program(d->exprs + off, len, c.width, d->n_regexes, in.value_cols());
    if (kind == VK_BOOL) fail(RDFGPU_ERR_INVALID, "node %u: expression %u leaves a boolean verdict, not a typed value: wrap it in BOOLEAN_AS_TERM", i, q);
    if (kind != VK_TV) fail(RDFGPU_ERR_INVALID, "node %u: expression %u leaves an id, not a typed value: a plain column is a projection", i, q);
    nd.agg_progs.push_back(load_value_program(plan, in, d->exprs + off, len));
  }
  nd.width = nd.n_proj + k;
  for (u32 q = 0; q < k; q++) nd.origin[nd.n_proj + q] = ValueOrigin{(int)i, q, true};
}

// SortExec (RDFGPU_NODE_SORT): the keys typed against the input's columns — an id form reads object ids, BY_VALUE a value column — the width
// of the key record they make (sort.hip: one 64-bit word per id key, kSortValueWords per value key, one for the row index), the projection.
void compile_sort(Plan* plan, const rdfgpu_plan_desc* d, u32 i) {
  NodeInfo& nd = plan->nodes[i];
  const rdfgpu_plan_node& r = nd.d;
  const NodeInfo& c = child(plan, i, r.left, "input");
  if (r.n_keys < 1 || r.n_keys > RDFGPU_MAX_KEYS) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: SortExec with %u sort keys (1 to %u)", i, r.n_keys, RDFGPU_MAX_KEYS);
  u32 words = 1;
  for (u32 k = 0; k < r.n_keys; k++) {
    const u32 col = r.left_keys[k], how = r.right_keys[k] & ~RDFGPU_SORT_DESC;
    if (col >= c.width) fail(RDFGPU_ERR_INVALID, "node %u: sort key column %u out of range", i, col);
    if (how > RDFGPU_SORT_BY_VALUE) fail(RDFGPU_ERR_INVALID, "node %u: unknown sort mode %u", i, r.right_keys[k]);
    if (how == RDFGPU_SORT_BY_VALUE) {
      if (!plan->agg_columns) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: SortExec key %u sorts a value column (RDFGPU_SORT_BY_VALUE): value columns exist only in a plan compiled with RDFGPU_PLAN_AGG_COLUMNS", i, k);
      if (c.origin[col].node < 0) fail(RDFGPU_ERR_INVALID, "node %u: SortExec key %u: RDFGPU_SORT_BY_VALUE of column %u, which holds object ids (RDFGPU_SORT_BY_ID / _BY_TERM / _BY_DOUBLE sort those)", i, k, col);
      words += kSortValueWords;
    } else {
      refuse_value_column(c.origin[col], i, "SortExec key by id / term / double", col);   // (RDFGPU_SORT_BY_VALUE sorts it)
      words += 1;
    }
  }
  if (words > kSortMaxWords)
    fail(RDFGPU_ERR_UNSUPPORTED, "node %u: SortExec key record of %u 64-bit words (at most %u: a tile of %u records has to fit 64 KB of LDS; a key by value takes %u words, any other one, the row index one)",
         i, words, kSortMaxWords, kSortTile, kSortValueWords);
  nd.sort_words = words;
  InputSchema in; in.append(c);
  load_projection(nd, d, in, "SortExec");   // a projected value column keeps its origin: its entries leave unchanged
}

// Every node of the description, in order (an input precedes its consumer): checked, typed, its program and projection loaded.  Only a
// DataSourceExec touches the store.
void compile_nodes(Plan* plan, const rdfgpu_plan_desc* d) {
  for (u32 i = 0; i < d->n_nodes; i++) {
    NodeInfo& nd = plan->nodes[i];
    nd.d = d->nodes[i];
    const rdfgpu_plan_node& r = nd.d;
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
        InputSchema in; in.append(child(plan, i, r.left, "input"));
        load_program(nd, plan, d, in, "FilterExec");
        load_projection(nd, d, in, "FilterExec");
        nd.shape = detect_shape(nd.prog, plan->opt.on(RDFGPU_OPT_FORCE_GENERIC_VM));
        break;
      }
      case RDFGPU_NODE_PROJECTION: {
        InputSchema in; in.append(child(plan, i, r.left, "input"));
        load_projection(nd, d, in, "ProjectionExec");
        break;
      }
      case RDFGPU_NODE_HASH_JOIN: case RDFGPU_NODE_CROSS_JOIN: case RDFGPU_NODE_NESTED_LOOP_JOIN: compile_join(plan, d, i); break;
      case RDFGPU_NODE_CLOSURE: {
        const NodeInfo& c = child(plan, i, r.left, "inner paths");
        if (c.width != 3) fail(RDFGPU_ERR_INVALID, "node %u: KleenePlusClosureExec input has %u columns, not (graph, start, end)", i, c.width);
        if (r.join_type > 1) fail(RDFGPU_ERR_INVALID, "node %u: allow_cross_graph_paths is 0 or 1", i);
        for (u32 k = 0; k < 3; k++) refuse_value_column(c.origin[k], i, "KleenePlusClosureExec input", k);
        InputSchema in; in.append(c);
        load_projection(nd, d, in, "KleenePlusClosureExec");
        break;
      }
      case RDFGPU_NODE_UNION: {
        const NodeInfo& l = child(plan, i, r.left, "left");
        const NodeInfo& rr = child(plan, i, r.right, "right");
        if (l.width != rr.width) fail(RDFGPU_ERR_INVALID, "node %u: UnionExec inputs have %u and %u columns", i, l.width, rr.width);
        for (u32 k = 0; k < l.width; k++) { refuse_value_column(l.origin[k], i, "UnionExec left input", k); refuse_value_column(rr.origin[k], i, "UnionExec right input", k); }
        InputSchema in; in.append(l);
        load_projection(nd, d, in, "UnionExec");
        break;
      }
      case RDFGPU_NODE_TABLE: {
        if (r.table_cols > (u32)kMaxCols) fail(RDFGPU_ERR_UNSUPPORTED, "node %u: table with %u columns", i, r.table_cols);
        nd.width = r.table_cols;
        if (plan->tables.size() <= r.table_slot) plan->tables.resize(r.table_slot + 1);
        break;
      }
      case RDFGPU_NODE_TOPK: compile_topk(plan, d, i); break;           // DISTINCT + TopK(fetch) per group, ..Q5 (Execution Plan).snap:5-9
      case RDFGPU_NODE_AGGREGATE: compile_aggregate(plan, d, i); break;   // AggregateExec(mode=Single), ..Business Intelligence - Q8 (Execution Plan).snap
      case RDFGPU_NODE_EXTEND: compile_extend(plan, d, i); break;         // ProjectionExec: expr=[.., DIV(..) as ratio], ..Business Intelligence - Q3 (Execution Plan).snap
      case RDFGPU_NODE_SORT: compile_sort(plan, d, i); break;             // SortExec: TopK(fetch=10), expr=[.. DESC, .. ASC], ..Business Intelligence - Q3 (Execution Plan).snap:6
      default: fail(RDFGPU_ERR_INVALID, "node %u: unknown kind %u", i, r.kind);
    }
  }
}

// Join reordering (physical rewrite, results unchanged): an inner HashJoinExec whose build child is a
// CrossJoinExec(A, B) and whose equi-keys come partly from A and partly from B
//     (A x B) JOIN C ON a = c1 AND b = c2          (Q5 (Execution Plan).snap:18-26: label x features(X))
// is the join graph A - C - B; it runs as  A JOIN (B JOIN C ON b = c2) ON a = c1  without ever
// materialising |A| x |B| rows.  Column order [A, B, C] is preserved, so filter and projection stay valid.
void reorder_cross_joins(Plan* plan) {
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
    for (u32 k = 0; k < wB + wC; k++) { t.proj[k] = k; t.origin[k] = k < wB ? plan->nodes[bi].origin[k] : plan->nodes[cri].origin[k - wB]; }
    plan->nodes.push_back(t);
    NodeInfo& j = plan->nodes[i];
    j.d.left = (int32_t)ai; j.d.right = (int32_t)(plan->nodes.size() - 1);
    j.d.n_keys = nA;
    for (u32 k = 0; k < nA; k++) { j.d.left_keys[k] = la[k]; j.d.right_keys[k] = ra[k]; }
  }
}

// consumers per node (`refs`), counted over the operators reachable from the root only (a rewritten-away
// CrossJoinExec must not keep its former inputs "shared"); then `parent`, the one consumer of a node consumed once
void count_consumers(Plan* plan) {
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
      const bool binary = is_binary(nd.d.kind);
      if (nd.d.left >= 0) { plan->nodes[nd.d.left].refs++; stack.push_back((u32)nd.d.left); }
      if (binary && nd.d.right >= 0) { plan->nodes[nd.d.right].refs++; stack.push_back((u32)nd.d.right); }
    }
  }
  for (u32 i = 0; i < plan->nodes.size(); i++) {   // the one consumer of a node consumed once
    const NodeInfo& nd = plan->nodes[i];
    if (nd.d.kind == RDFGPU_NODE_DATA_SOURCE || nd.d.kind == RDFGPU_NODE_TABLE) continue;
    const bool binary = is_binary(nd.d.kind);
    if (i != plan->root && nd.refs == 0) continue;   // (rewritten away: not an operator of this plan any more)
    if (nd.d.left >= 0 && plan->nodes[nd.d.left].refs == 1) plan->nodes[nd.d.left].parent = (int)i;
    if (binary && nd.d.right >= 0 && plan->nodes[nd.d.right].refs == 1) plan->nodes[nd.d.right].parent = (int)i;
  }
}

// per-node byte accounting inputs: distinct columns read, typed gathers per row
void account_columns_read(Plan* plan) {
  for (NodeInfo& nd : plan->nodes) {
    nd.lex = program_has_lex(nd.prog);
    for (const ExprProgram& pr : nd.agg_progs) nd.lex = nd.lex || program_has_lex(pr);
    u32 used = columns_read(nd.prog);
    for (u32 i = 0; i < nd.prog.n; i++) if (nd.prog.nodes[i].op == RDFGPU_EX_ENC_TV) nd.n_enc_tv++;
    if (nd.d.kind == RDFGPU_NODE_FILTER) for (u32 c = 0; c < nd.n_proj; c++) used |= 1u << nd.proj[c];
    if (nd.d.kind == RDFGPU_NODE_EXTEND)   // the programs of the computed columns (the kept columns are handed on, not read)
      for (const ExprProgram& pr : nd.agg_progs) {
        used |= columns_read(pr);
        for (u32 i = 0; i < pr.n; i++) if (pr.nodes[i].op == RDFGPU_EX_ENC_TV || pr.nodes[i].op == kExAggValue) nd.n_enc_tv++;
      }
    nd.n_cols_read += (u32)__builtin_popcount(used);
  }
}

}  // namespace

// rdfgpu_plan_desc.flags: RDFGPU_PLAN_VALUE_KEYS groups by value columns, which exist only when aggregate values are columns.
void check_plan_flags(u32 flags) {
  if ((flags & RDFGPU_PLAN_VALUE_KEYS) && !(flags & RDFGPU_PLAN_AGG_COLUMNS))
    fail(RDFGPU_ERR_INVALID, "plan_compile: RDFGPU_PLAN_VALUE_KEYS is valid only together with RDFGPU_PLAN_AGG_COLUMNS (value columns exist only in such a plan)");
}

Plan* plan_compile(Store* store, const rdfgpu_plan_desc* d) {
  if (!store) fail(RDFGPU_ERR_INVALID, "plan_compile: null store");
  if (!d || !d->nodes || d->n_nodes == 0) fail(RDFGPU_ERR_INVALID, "plan_compile: empty plan");
  if (d->root >= d->n_nodes) fail(RDFGPU_ERR_INVALID, "plan_compile: root %u out of range", d->root);
  std::unique_ptr<Plan> plan(new Plan());
  plan->store = store;
  plan->opt = store->opt;
  store->retain();
  plan->root = d->root;
  check_plan_flags(d->flags);
  plan->agg_columns = (d->flags & RDFGPU_PLAN_AGG_COLUMNS) != 0;
  plan->value_keys = (d->flags & RDFGPU_PLAN_VALUE_KEYS) != 0;
  plan->nodes.resize(d->n_nodes);
  if (d->n_regexes) compile_string_table(plan.get(), d);   // REGEX patterns are plan constants: compiled here, simulated per row on the device
  check_string_functions(store, d);
  compile_nodes(plan.get(), d);
  if (!plan->opt.on(RDFGPU_OPT_NO_JOIN_REORDER)) reorder_cross_joins(plan.get());
  count_consumers(plan.get());
  account_columns_read(plan.get());

  static_assert(sizeof(LocateJob) <= 128, "ExecContext staging assumes LocateJob <= 128 bytes");
  plan->ctx = store->acquire_context((u32)plan->sources.size());
  plan->stream = plan->ctx->stream;
  plan->counters = plan->ctx->counters;
  plan->upload_pool();
  return plan.release();
}

}  // namespace rdfgpu
