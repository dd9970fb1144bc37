// expr_ops.hpp — what the host knows about each expression op, once (plain C++, nothing of HIP).
//
// Plan compilation asks "is this op of kind X" in many places: which ops index the string table, which are refused in an aggregate's
// input, which send a program to the generic VM, which kernel instantiation runs it.  Each such list is one trait bit here, with the
// membership it has always had; tests/host/plan_compile_checks.cpp pins every list op by op.  A new op gets its line in op_traits, and
// with it its place in every list ("Adding an expression op").
#pragma once
#include <stdint.h>

#include "../../include/rdfgpu.h"

namespace rdfgpu {

// Internal op (never accepted from a description: check_program knows RDFGPU_EX_* only).  plan_compile writes it in place of the ENC_TV of
// an aggregate value column (RDFGPU_PLAN_AGG_COLUMNS): u = origin node << 8 | aggregate (of an AggregateExec) or expression (of a
// ProjectionExec with expressions, RDFGPU_NODE_EXTEND); Plan::bind_values fills in, per execution, lo = the device address of that
// rdfgpu_agg_value array and hi = its length.
constexpr uint8_t kExAggValue = 250;
static_assert(kExAggValue >= RDFGPU_EX__COUNT, "the internal op must lie outside the ABI's ops");

// The traits.  Lists that look alike stay apart where they differ by an op: kOpView has CAST_STRING and no STRLEN (STRLEN yields an
// integer), kOpStringFn has STRLEN and no CAST_STRING (a computed column may hold the cast: its host prepares nothing for it), and
// kOpStoreStrings is neither (no LIT_STR: a constant's bytes come with the plan).  kOpExtended is kOpGenericVm without CAST_STRING and
// the value load.  kOpSlot is kOpPattern with LIT_STR and without REGEX_VAR, whose `u` starts a range of `lo` slots.  No two are equal.
enum : uint32_t {
  kOpKnown = 1u << 0,          // the op has an entry: every RDFGPU_EX_* that check_program accepts, and kExAggValue
  kOpCmp = 1u << 1,            // a typed comparison (GT .. NEQ): the specialised filter and join-filter shapes match on it
  kOpSlot = 1u << 2,           // `u` indexes the plan's string table (rdfgpu_plan_desc.regexes): range-checked, the entry compiled by this use
  kOpNeedle = 1u << 3,         // .. and the entry is a literal needle, compiled like a pattern with the `q` flag
  kOpPattern = 1u << 4,        // a pattern op: prepared per node in FilterExec and the joins only, so refused in an aggregate's input and a computed column
  kOpView = 1u << 5,           // yields a string view (a computed string): such a program may hold no string literal given by rank only
  kOpStringFn = 1u << 6,       // a string function: refused in a computed column, whose 24-byte record has no form for a view
  kOpStoreStrings = 1u << 7,   // reads lexical forms: the store must have its strings (rdfgpu_store_set_strings)
  kOpGenericVm = 1u << 8,      // the specialised filter shapes do not know it: a program that holds it runs in the generic VM
  kOpExtended = 1u << 9,       // .. in the instantiation with the extended cases compiled in (eval_program<LEX = true>; NodeInfo::lex)
  kOpDatePart = 1u << 10,      // YEAR .. SECONDS
  kOpForm = 1u << 11,          // the functional forms and term tests, IF .. IS_NUMERIC
};

constexpr uint32_t op_traits(uint32_t op) {
  switch (op) {
    case RDFGPU_EX_COLUMN: case RDFGPU_EX_LIT_ID: case RDFGPU_EX_LIT_TV: case RDFGPU_EX_LIT_BOOL: case RDFGPU_EX_ENC_TV:
    case RDFGPU_EX_ADD: case RDFGPU_EX_SUB: case RDFGPU_EX_MUL: case RDFGPU_EX_DIV:
    case RDFGPU_EX_NEG: case RDFGPU_EX_PLUS: case RDFGPU_EX_ABS: case RDFGPU_EX_ROUND: case RDFGPU_EX_CEIL: case RDFGPU_EX_FLOOR: case RDFGPU_EX_CAST:
    case RDFGPU_EX_EBV: case RDFGPU_EX_ID_EQ: case RDFGPU_EX_ID_NEQ: case RDFGPU_EX_IS_COMPATIBLE:
    case RDFGPU_EX_AND: case RDFGPU_EX_OR: case RDFGPU_EX_NOT: case RDFGPU_EX_BOUND: case RDFGPU_EX_BOOL_AS_TV:
      return kOpKnown;
    case RDFGPU_EX_GT: case RDFGPU_EX_LT: case RDFGPU_EX_GEQ: case RDFGPU_EX_LEQ: case RDFGPU_EX_EQ: case RDFGPU_EX_NEQ:
      return kOpKnown | kOpCmp;
    case RDFGPU_EX_REGEX: return kOpKnown | kOpSlot | kOpPattern;
    case RDFGPU_EX_CONTAINS: case RDFGPU_EX_STRSTARTS: case RDFGPU_EX_STRENDS: return kOpKnown | kOpSlot | kOpNeedle | kOpPattern;
    case RDFGPU_EX_LANG_IN: return kOpKnown | kOpSlot | kOpPattern;
    case RDFGPU_EX_REGEX_VAR: return kOpKnown | kOpPattern;
    case RDFGPU_EX_LIT_STR: return kOpKnown | kOpSlot | kOpView | kOpStringFn;
    case RDFGPU_EX_STR: case RDFGPU_EX_SUBSTR: case RDFGPU_EX_UCASE: case RDFGPU_EX_LCASE: case RDFGPU_EX_STRBEFORE: case RDFGPU_EX_STRAFTER:
      return kOpKnown | kOpView | kOpStringFn | kOpStoreStrings;
    case RDFGPU_EX_STRLEN: return kOpKnown | kOpStringFn | kOpStoreStrings;
    case RDFGPU_EX_CAST_STRING: return kOpKnown | kOpView | kOpStoreStrings | kOpGenericVm;
    case RDFGPU_EX_CAST_LEX: return kOpKnown | kOpStoreStrings | kOpGenericVm | kOpExtended;
    case RDFGPU_EX_YEAR: case RDFGPU_EX_MONTH: case RDFGPU_EX_DAY: case RDFGPU_EX_HOURS: case RDFGPU_EX_MINUTES: case RDFGPU_EX_SECONDS:
      return kOpKnown | kOpGenericVm | kOpExtended | kOpDatePart;
    case RDFGPU_EX_IF: case RDFGPU_EX_COALESCE: case RDFGPU_EX_IS_IRI: case RDFGPU_EX_IS_BLANK: case RDFGPU_EX_IS_LITERAL: case RDFGPU_EX_IS_NUMERIC:
      return kOpKnown | kOpGenericVm | kOpExtended | kOpForm;
    case kExAggValue: return kOpKnown | kOpGenericVm;
    default: return 0;   // no entry: not an op
  }
}

constexpr bool op_is(uint32_t op, uint32_t trait) { return (op_traits(op) & trait) != 0; }
constexpr bool is_cmp(uint32_t op) { return op_is(op, kOpCmp); }
constexpr bool is_date_part_op(uint32_t op) { return op_is(op, kOpDatePart); }
constexpr bool is_form_op(uint32_t op) { return op_is(op, kOpForm); }

// The targets of CAST and CAST_LEX on the device.
constexpr bool is_cast_target(uint32_t tag) {
  return tag == RDFGPU_TV_BOOLEAN || tag == RDFGPU_TV_INT || tag == RDFGPU_TV_INTEGER || tag == RDFGPU_TV_DECIMAL || tag == RDFGPU_TV_FLOAT || tag == RDFGPU_TV_DOUBLE;
}

// Whether one of `n` nodes / a program (an ExprProgram: `n` nodes in `nodes`) holds an op with one of the traits.
inline bool any_op_is(const rdfgpu_expr_node* nodes, uint32_t n, uint32_t traits) {
  for (uint32_t i = 0; i < n; i++) if (op_is(nodes[i].op, traits)) return true;
  return false;
}
template <class Program>
bool program_has(const Program& pr, uint32_t traits) { return any_op_is(pr.nodes, pr.n, traits); }
// A program that holds a lexical cast of a literal (CAST_LEX), a date part, IF, COALESCE or a term test: its host launches the
// instantiation of its kernel that compiles those cases in (LEX = true).
template <class Program>
bool program_has_lex(const Program& pr) { return program_has(pr, kOpExtended); }

}  // namespace rdfgpu
