// expr_device.hpp — per-row evaluation of SPARQL FILTER / join-filter programs on gfx950.
//
// Device restatement of the reference's typed-value semantics (one row = one lane; the program is
// wave-uniform, so every branch on the opcode is a scalar branch):
//   ENC_TV   lib/functions/src/builtin/encoding/with_typed_value_encoding.rs:71-79
//            (id -> typed value; here ONE aligned 16-byte gather from the HBM side table)
//   GT/LT/.. lib/functions/src/scalar/comparison/*.rs via PartialOrd lib/model/src/typed_value.rs:162-261
//   promotion lib/model/src/xsd/numeric.rs:127-201
//   ADD/SUB  lib/functions/src/scalar/numeric/add.rs:40-86 (checked int/decimal, IEEE float/double)
//   MUL/DIV  scalar/numeric/mul.rs:50-76, div.rs:51-80 over Decimal::checked_mul / checked_div (lib/model/src/xsd/decimal.rs:93-163)
//   NEG/PLUS/ABS  unary_minus.rs, unary_plus.rs, abs.rs (lib/model/src/xsd/numeric.rs:20-38)
//   ROUND/CEIL/FLOOR  round.rs:48-60, ceil.rs:48-60, floor.rs (decimal.rs:211-254; f32 / f64 round, ceil, floor)
//   CAST     scalar/conversion/cast_{boolean,int,integer,decimal,float,double}.rs:48-62 and the From / TryFrom impls they call
//   CAST_STRING  scalar/conversion/cast_string.rs:51-76 (the lexical form of a term that has one as written: a view, nothing copied)
//   CAST_LEX     the same casts with the simple-literal arm: the FromStr impls of lib/model/src/xsd, restated in lex_parse.hpp
//   YEAR .. SECONDS  scalar/dates_and_times/{year,month,day,hours,minutes,seconds}.rs over Timestamp::{year_month_day, hour, minute, second}
//            (lib/model/src/xsd/date_time.rs:1731-1839), restated in date_parts.hpp
//   EBV      lib/functions/src/builtin/native/effective_boolean_value.rs:99-119
//   IF       scalar/functional_form/sparql_if.rs:38-61 (Boolean::try_from of the test, lib/model/src/xsd/boolean.rs:93-102: not the EBV)
//   COALESCE lib/functions/src/registry.rs:264-270 (DataFusion's `coalesce`: the first argument that is not null)
//   IS_IRI / IS_BLANK / IS_LITERAL / IS_NUMERIC  scalar/terms/is_{iri,blank,literal,numeric}.rs
//   AND/OR   SQL three-valued logic on native booleans (lib/logical/src/expr_builder_context.rs:393-434)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rdfgpu.h"
#include "expr_ops.hpp"
#include "regex_prog.hpp"
#include "lex_parse.hpp"
#include "date_parts.hpp"

namespace rdfgpu {

constexpr int kMaxExpr = 40;   // nodes per program (kernarg resident: 40 * 24 B)
constexpr int kMaxStack = 8;

struct ExprProgram {
  uint32_t n;
  uint32_t pad;
  rdfgpu_expr_node nodes[kMaxExpr];
  const RegexProg* regex;        // the plan's compiled REGEX patterns (device memory), indexed by REGEX nodes' `u`
  const uint8_t* str_consts;     // bytes of the plan's string constants (RDFGPU_EX_LIT_STR): entry u = [regex[u].first, + regex[u].n_pos)
};

struct TypedTable {
  const rdfgpu_typed_value* tv;  // indexed by object id
  uint64_t n_ids;
  const int64_t* dec;            // (lo, hi) pairs of i128 decimals
  uint64_t n_dec;
  const uint64_t* str_off;       // lexical form of string id i: heap[str_off[i] .. str_off[i + 1]) (null: not installed)
  const uint8_t* heap;
  uint64_t n_str_ids;
  uint32_t* rt_error;            // the executing plan's run-time error flags (null outside a plan): bit 0 a REGEX with a Perl
                                 // class / word boundary met a non-ASCII subject, bit 1 a per-row REGEX pattern was not announced,
                                 // bit 2 a string expression met what the device does not restate (case mapping of a non-ASCII
                                 // string, a non-integer SUBSTR argument), bit 3 a numeric CAST met a simple literal (the lexical
                                 // parsers are not restated), bit 4 a computed column (RDFGPU_NODE_EXTEND) met a value of a kind its
                                 // 24-byte record cannot carry, bit 5 a SortExec key by term (RDFGPU_NODE_SORT, RDFGPU_SORT_BY_TERM) met a
                                 // kind whose rank is not defined, bit 6 a lexical cast (RDFGPU_EX_CAST_LEX) met a literal the device
                                 // cannot decide: a float / double at a rounding boundary that Eisel-Lemire declines, or a signed NaN,
                                 // bit 7 a MIN / MAX (RDFGPU_AGG_MIN / _MAX) met a bound value that is not numeric
};

// Value kinds on the evaluation stack.  VK_VALUE exists at compile only (check_program): COLUMN of an aggregate value column, whose u32 is
// an index into its AggregateExec's value array and not an object id; on the device such a column is a VK_ID like any other.
enum : uint32_t { VK_ID = 0, VK_TV = 1, VK_BOOL = 2, VK_VALUE = 3 };

struct Val {
  int64_t lo;     // ID: object id; TV: payload; BOOL: 0 false / 1 true / 2 null
  int64_t hi;     // TV decimal: high 64 bits
  uint32_t aux;   // TV: language id / datatype id
  uint8_t kind, tag, flags, pad;
};
// String VIEWS (RDFGPU_EX_STR / LIT_STR / SUBSTR / UCASE / LCASE): tag STRING with `pad` saying where the bytes are —
//   0  a dictionary string as ENC_TV delivers it: lo = rank in `str` order, hi = object id (its lexical form is in the heap)
//   1  a window of the heap's lexical form of object id (u32)hi:   lo = (first byte << 32) | bytes
//   2  a window of the plan's string constant (u32)hi:             lo = (first byte << 32) | bytes
// and flags bits 4 / 5 an ASCII upper / lower case mapping applied when a byte is read.  Nothing is materialised.
constexpr uint8_t kStrUpper = 0x10, kStrLower = 0x20;
constexpr uint32_t kRtStringUnsupported = 4u;
constexpr uint32_t kRtCastFromString = 8u;
constexpr uint32_t kRtExtendKind = 16u;
constexpr uint32_t kRtSortTerm = 32u;
constexpr uint32_t kRtLexParse = 64u;
constexpr uint32_t kRtMinMaxKind = 128u;

typedef __int128 i128_t;
typedef unsigned __int128 u128_t;

__device__ __forceinline__ Val val_tv_null() { Val v; v.lo = 0; v.hi = 0; v.aux = 0; v.kind = VK_TV; v.tag = RDFGPU_TV_NULL; v.flags = 0; v.pad = 0; return v; }
__device__ __forceinline__ Val val_tv_bool(bool b) { Val v = val_tv_null(); v.tag = RDFGPU_TV_BOOLEAN; v.lo = b ? 1 : 0; return v; }
__device__ __forceinline__ Val val_bool(uint32_t b) { Val v = val_tv_null(); v.kind = VK_BOOL; v.lo = b; return v; }
__device__ __forceinline__ Val val_id(uint32_t id) { Val v = val_tv_null(); v.kind = VK_ID; v.lo = id; return v; }

__device__ __forceinline__ i128_t val_dec(const Val& v) { return (i128_t)(((u128_t)(uint64_t)v.hi << 64) | (u128_t)(uint64_t)v.lo); }
__device__ __forceinline__ void set_dec(Val& v, i128_t d) { v.lo = (int64_t)(uint64_t)(u128_t)d; v.hi = (int64_t)(uint64_t)((u128_t)d >> 64); }

// dateTime / time / date: a Timestamp = timeOnTimeline seconds * 10^18 (i128 side table) + "has a timezone" (aux bit 0),
// lib/model/src/xsd/date_time.rs:1599-1603
__device__ __forceinline__ bool tv_is_timestamp(uint8_t tag) { return tag == RDFGPU_TV_DATE_TIME || tag == RDFGPU_TV_TIME || tag == RDFGPU_TV_DATE; }

// ENC_TV: one 16-byte gather (global_load_dwordx4) per row.
// TZ: a timestamp also takes its timezone offset (rdfgpu_typed_value.tz_minutes, bits 16..31 of the row's fourth dword) into bits 16..31
// of `aux`, where a timestamp LITERAL carries it (rdfgpu_expr_node.u).  Nothing but the date parts (tv_date_part) reads those bits: the
// comparisons look at bit 0 only.  Only the VM instantiations that compile the date parts in ask for it (eval_program<true>).
template <bool TZ = false>
__device__ __forceinline__ Val enc_tv(const TypedTable& t, uint32_t id) {
  Val v = val_tv_null();
  if (id == 0 || id >= t.n_ids) return v;
  const int4 raw = *reinterpret_cast<const int4*>(t.tv + id);
  v.lo = (int64_t)(((uint64_t)(uint32_t)raw.y << 32) | (uint32_t)raw.x);
  v.aux = (uint32_t)raw.z;
  v.tag = (uint8_t)((uint32_t)raw.w & 0xff);
  v.flags = (uint8_t)(((uint32_t)raw.w >> 8) & 0xff);
  if (v.tag == RDFGPU_TV_STRING) v.hi = id;   // string builtins find the lexical form through the id
  if (v.tag == RDFGPU_TV_DECIMAL || tv_is_timestamp(v.tag)) {   // the i128 lives in the side table
    if ((uint64_t)v.lo >= t.n_dec) return val_tv_null();
    const int64_t* d = t.dec + 2 * v.lo;
    v.lo = d[0]; v.hi = d[1];
    if constexpr (TZ) { if (v.tag != RDFGPU_TV_DECIMAL) v.aux |= (uint32_t)raw.w & 0xFFFF0000u; }
  }
  return v;
}

// kExAggValue: the value a value column's entry stands for.  `idx` is 1-based (row g of the AggregateExec carries g + 1); 0, the error
// aggregate, and anything beyond the array are the null typed value.  An rdfgpu_agg_value is what enc_tv leaves after its side-table read:
// integer lo; decimal (lo, hi) = the i128; float / double their bits in lo.
__device__ __forceinline__ Val agg_value_load(const rdfgpu_expr_node& e, uint32_t idx) {
  Val v = val_tv_null();
  if (idx == 0 || (uint64_t)idx > (uint64_t)e.hi) return v;
  const long long* p = reinterpret_cast<const long long*>(e.lo) + 3ull * (idx - 1u);
  v.lo = p[0]; v.hi = p[1]; v.tag = (uint8_t)((uint64_t)p[2] & 0xff);
  return v;
}

// ---- decimal (i128 * 10^-18) -> f64, From<Decimal> for Double lib/model/src/xsd/decimal.rs:445-462 ----
// No 128-bit division / int->fp libcalls exist on the device, so both are spelled out.
__device__ __forceinline__ uint32_t u128_divmod10(u128_t& v) {  // v /= 10, returns v % 10
  uint32_t limb[4] = {(uint32_t)(v >> 96), (uint32_t)(v >> 64), (uint32_t)(v >> 32), (uint32_t)v};
  uint64_t rem = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) { uint64_t cur = (rem << 32) | limb[i]; limb[i] = (uint32_t)(cur / 10u); rem = cur % 10u; }
  v = ((u128_t)limb[0] << 96) | ((u128_t)limb[1] << 64) | ((u128_t)limb[2] << 32) | (u128_t)limb[3];
  return (uint32_t)rem;
}
__device__ __forceinline__ double u128_to_f64(u128_t v) {  // round-to-nearest-even, like Rust `as f64`
  uint64_t hi = (uint64_t)(v >> 64), lo = (uint64_t)v;
  if (hi == 0) return (double)lo;
  int lz = __clzll((long long)hi);
  u128_t n = v << lz;
  uint64_t m = (uint64_t)(n >> 64);
  if ((uint64_t)n != 0) m |= 1;  // sticky bit (11 guard bits below the 53-bit mantissa)
  return ldexp((double)m, 64 - lz);
}
__device__ __forceinline__ double dec_to_f64(i128_t value) {
  bool neg = value < 0;
  u128_t mag = neg ? (u128_t)(-(value + 1)) + 1 : (u128_t)value;
  uint64_t shift = 1000000000000000000ull;
  if (mag != 0) {
    while (shift != 1) {
      u128_t q = mag;
      uint32_t r = u128_divmod10(q);
      if (r != 0) break;
      mag = q; shift /= 10;
    }
  }
  double d = u128_to_f64(mag) / (double)shift;
  return neg ? -d : d;
}

enum { NK_INT, NK_INTEGER, NK_FLOAT, NK_DOUBLE, NK_DECIMAL, NK_NONE };
__device__ __forceinline__ int num_kind(uint8_t tag) {
  switch (tag) {
    case RDFGPU_TV_INT: return NK_INT;
    case RDFGPU_TV_INTEGER: return NK_INTEGER;
    case RDFGPU_TV_FLOAT: return NK_FLOAT;
    case RDFGPU_TV_DOUBLE: return NK_DOUBLE;
    case RDFGPU_TV_DECIMAL: return NK_DECIMAL;
    default: return NK_NONE;
  }
}
// NumericPair::with_casts_from numeric.rs:127-201
__device__ __forceinline__ int pair_kind(int a, int b) {
  if (a == NK_DOUBLE || b == NK_DOUBLE) return NK_DOUBLE;
  if (a == NK_FLOAT || b == NK_FLOAT) return NK_FLOAT;
  if (a == NK_DECIMAL || b == NK_DECIMAL) return NK_DECIMAL;
  if (a == NK_INTEGER || b == NK_INTEGER) return NK_INTEGER;
  return NK_INT;
}
__device__ __forceinline__ double to_f64(const Val& v, int k) {
  switch (k) {
    case NK_INT: case NK_INTEGER: return (double)v.lo;             // i64 as f64, double.rs:196-201
    case NK_FLOAT: return (double)__uint_as_float((uint32_t)v.lo);
    case NK_DOUBLE: return __longlong_as_double(v.lo);
    default: return dec_to_f64(val_dec(v));
  }
}
__device__ __forceinline__ float to_f32(const Val& v, int k) {
  switch (k) {
    case NK_INT: return (float)(int32_t)v.lo;                      // float.rs:156-161
    case NK_INTEGER: return (float)v.lo;                           // float.rs:164-169
    case NK_FLOAT: return __uint_as_float((uint32_t)v.lo);
    case NK_DECIMAL: return (float)dec_to_f64(val_dec(v));         // decimal.rs:437-443
    default: return (float)__longlong_as_double(v.lo);
  }
}
__device__ __forceinline__ i128_t to_dec(const Val& v, int k) {
  return k == NK_DECIMAL ? val_dec(v) : (i128_t)v.lo * (i128_t)1000000000000000000ll;  // decimal.rs:363-375
}

constexpr int ORD_NONE = 2;
// PartialOrd for TypedValueRef, typed_value.rs:162-261 : -1 / 0 / 1 or ORD_NONE (incomparable => error)
__device__ __forceinline__ int tv_partial_cmp(const Val& a, const Val& b) {
  if (a.tag == RDFGPU_TV_NULL || b.tag == RDFGPU_TV_NULL) return ORD_NONE;
  if (a.tag == RDFGPU_TV_BLANK_NODE) return b.tag == RDFGPU_TV_BLANK_NODE ? (a.lo < b.lo ? -1 : a.lo > b.lo) : -1;
  if (a.tag == RDFGPU_TV_NAMED_NODE) {
    if (b.tag == RDFGPU_TV_BLANK_NODE) return 1;
    if (b.tag == RDFGPU_TV_NAMED_NODE) return a.lo < b.lo ? -1 : a.lo > b.lo;
    return -1;
  }
  if (b.tag == RDFGPU_TV_NAMED_NODE || b.tag == RDFGPU_TV_BLANK_NODE) return 1;
  if (a.tag == RDFGPU_TV_STRING) {
    if (b.tag != RDFGPU_TV_STRING || a.aux != b.aux) return ORD_NONE;  // simple vs lang / other language
    return a.lo < b.lo ? -1 : a.lo > b.lo;
  }
  if (a.tag == RDFGPU_TV_BOOLEAN) return b.tag == RDFGPU_TV_BOOLEAN ? (int)(a.lo != 0) - (int)(b.lo != 0) : ORD_NONE;
  const int ka = num_kind(a.tag), kb = num_kind(b.tag);
  if (ka != NK_NONE) {
    if (kb == NK_NONE) return ORD_NONE;
    switch (pair_kind(ka, kb)) {
      case NK_INT: case NK_INTEGER: return a.lo < b.lo ? -1 : a.lo > b.lo;
      case NK_FLOAT: { float x = to_f32(a, ka), y = to_f32(b, kb); return x < y ? -1 : x > y ? 1 : x == y ? 0 : ORD_NONE; }
      case NK_DOUBLE: { double x = to_f64(a, ka), y = to_f64(b, kb); return x < y ? -1 : x > y ? 1 : x == y ? 0 : ORD_NONE; }
      default: { i128_t x = to_dec(a, ka), y = to_dec(b, kb); return x < y ? -1 : x > y; }
    }
  }
  if (a.tag == RDFGPU_TV_OTHER) return (b.tag == RDFGPU_TV_OTHER && a.aux == b.aux && a.lo == b.lo) ? 0 : ORD_NONE;
  if (tv_is_timestamp(a.tag)) {
    // PartialOrd for Timestamp, date_time.rs:1617-1654: both or neither with a timezone => the values; otherwise the
    // value without one may lie 14 h either way, and the order must hold for both (an overflowing shift => None)
    if (b.tag != a.tag) return ORD_NONE;
    const i128_t x = val_dec(a), y = val_dec(b);
    const bool ta = a.aux & 1u, tb = b.aux & 1u;
    if (ta == tb) return x < y ? -1 : x > y;
    const i128_t shift = (i128_t)50400 * (i128_t)1000000000000000000ll;   // Decimal 14 * 3600
    i128_t hi, lo;
    if (__builtin_add_overflow(ta ? y : x, shift, &hi) || __builtin_sub_overflow(ta ? y : x, shift, &lo)) return ORD_NONE;
    const int plus = ta ? (x < hi ? -1 : x > hi) : (hi < y ? -1 : hi > y);
    const int minus = ta ? (x < lo ? -1 : x > lo) : (lo < y ? -1 : lo > y);
    return plus == minus ? plus : ORD_NONE;
  }
  return ORD_NONE;  // durations are opaque on device (their order is calendar arithmetic, duration.rs:271-310)
}

// ADD / SUB, add.rs:40-86
__device__ __forceinline__ Val tv_arith(const Val& a, const Val& b, bool sub) {
  const int ka = num_kind(a.tag), kb = num_kind(b.tag);
  Val r = val_tv_null();
  if (ka == NK_NONE || kb == NK_NONE) return r;
  switch (pair_kind(ka, kb)) {
    case NK_INT: {
      int32_t x = (int32_t)a.lo, y = (int32_t)b.lo, z;
      if (sub ? __builtin_sub_overflow(x, y, &z) : __builtin_add_overflow(x, y, &z)) return r;
      r.tag = RDFGPU_TV_INT; r.lo = z; return r; }
    case NK_INTEGER: {
      long long z;
      if (sub ? __builtin_sub_overflow((long long)a.lo, (long long)b.lo, &z) : __builtin_add_overflow((long long)a.lo, (long long)b.lo, &z)) return r;
      r.tag = RDFGPU_TV_INTEGER; r.lo = z; return r; }
    case NK_FLOAT: {
      float x = to_f32(a, ka), y = to_f32(b, kb);
      float z = sub ? __fsub_rn(x, y) : __fadd_rn(x, y);
      r.tag = RDFGPU_TV_FLOAT; r.lo = (int64_t)(uint64_t)__float_as_uint(z); return r; }
    case NK_DOUBLE: {
      double x = to_f64(a, ka), y = to_f64(b, kb);
      double z = sub ? __dsub_rn(x, y) : __dadd_rn(x, y);
      r.tag = RDFGPU_TV_DOUBLE; r.lo = __double_as_longlong(z); return r; }
    default: {
      i128_t x = to_dec(a, ka), y = to_dec(b, kb), z;
      if (sub ? __builtin_sub_overflow(x, y, &z) : __builtin_add_overflow(x, y, &z)) return r;
      r.tag = RDFGPU_TV_DECIMAL; set_dec(r, z); return r; }
  }
}

// ---- decimals (i128 x 10^-18): multiply, divide, round — lib/model/src/xsd/decimal.rs:93-163, 211-254 ----
// There is no 128-bit multiply-overflow or division libcall on the device: magnitudes over 64-bit limbs, the sign kept apart.
// Out of line: every kernel that hosts the VM would otherwise carry the 128-step divisions in its own body.
constexpr uint64_t kDecOne = 1000000000000000000ull;   // DECIMAL_PART_POW
__device__ __forceinline__ u128_t i128_mag(i128_t v) { return v < 0 ? (u128_t)0 - (u128_t)v : (u128_t)v; }
__device__ __forceinline__ bool i128_from_mag(bool neg, u128_t m, i128_t& out) {   // false: outside [-2^127, 2^127 - 1]
  const u128_t top = (u128_t)1 << 127;
  if (neg ? m > top : m >= top) return false;
  out = (i128_t)(neg ? (u128_t)0 - m : m);
  return true;
}
__device__ __forceinline__ bool u128_mul_checked(u128_t a, u128_t b, u128_t& out) {   // false: the product needs more than 128 bits
  const uint64_t a0 = (uint64_t)a, a1 = (uint64_t)(a >> 64), b0 = (uint64_t)b, b1 = (uint64_t)(b >> 64);
  if (a1 && b1) return false;
  const u128_t cross = (u128_t)a1 * b0 + (u128_t)a0 * b1;   // (one of the two products is 0)
  if (cross >> 64) return false;
  const u128_t lo = (u128_t)a0 * b0;
  out = lo + (cross << 64);
  return out >= lo;
}
__device__ __forceinline__ u128_t u128_div(u128_t n, u128_t d) {   // shift-subtract, d != 0
  u128_t q = 0, r = 0;
  for (int i = 127; i >= 0; i--) {
    r = (r << 1) | ((n >> i) & 1);
    if (r >= d) { r -= d; q |= (u128_t)1 << i; }
  }
  return q;
}
__device__ __forceinline__ uint32_t u128_strip_zeros(u128_t& m) {   // `while v % 10 == 0 { v /= 10 }`, m != 0
  uint32_t z = 0;
  for (;;) { u128_t q = m; if (u128_divmod10(q) != 0) return z; m = q; z++; }
}
__device__ __forceinline__ u128_t u128_pow10(uint32_t e) { u128_t p = 1; for (uint32_t i = 0; i < e; i++) p *= 10u; return p; }   // e <= 38
// i128::checked_mul
__device__ __forceinline__ bool i128_mul_checked(i128_t x, i128_t y, i128_t& out) {
  u128_t m;
  return u128_mul_checked(i128_mag(x), i128_mag(y), m) && i128_from_mag((x < 0) != (y < 0), m, out);
}
// Decimal::checked_mul, decimal.rs:93-125: both values lose their trailing decimal zeros, the zeros must make up the 18 fraction digits
// (a product that would need more precision is an error, and so is 0 x anything with fewer than 18 zeros: as written there)
__device__ __noinline__ bool dec_checked_mul(i128_t left, i128_t right, i128_t& out) {
  const bool neg = (left < 0) != (right < 0);
  u128_t ml = i128_mag(left), mr = i128_mag(right);
  const uint32_t zeros = (ml ? u128_strip_zeros(ml) : 0u) + (mr ? u128_strip_zeros(mr) : 0u);
  if (zeros < 18u || zeros - 18u > 38u) return false;   // checked_sub; 10_i128.checked_pow
  u128_t m; i128_t p;   // p: only its range check counts — `left.checked_mul(right)` must fit i128 before the scale is applied
  if (!u128_mul_checked(ml, mr, m) || !i128_from_mag(neg, m, p)) return false;
  return u128_mul_checked(m, u128_pow10(zeros - 18u), m) && i128_from_mag(neg, m, out);
}
// Decimal::checked_div, decimal.rs:131-163: the dividend is scaled by 10 while it stays inside i128, the divisor loses its trailing zeros,
// two truncating divisions (toward zero: on the magnitudes); a zero divisor, MIN / -1 and a scale beyond 10^38 are errors
__device__ __noinline__ bool dec_checked_div(i128_t left, i128_t right, i128_t& out) {
  if (right == 0) return false;
  const bool neg = (left < 0) != (right < 0);
  u128_t ml = i128_mag(left), mr = i128_mag(right);
  uint32_t shift_left = 0;
  if (ml != 0) {   // `while let Some(r) = left.checked_mul(10)`: |left| * 10 stays inside i128 (for both signs) iff |left| <= (2^127 - 1) / 10
    const u128_t lim = ((u128_t)0x0CCCCCCCCCCCCCCCull << 64) | (u128_t)0xCCCCCCCCCCCCCCCCull;
    while (ml <= lim) { ml *= 10u; shift_left++; }
  }
  const uint32_t total = shift_left + u128_strip_zeros(mr);
  if (total < 18u || total - 18u > 38u) return false;
  const u128_t q = u128_div(ml, mr);
  if (!neg && (q >> 127)) return false;   // MIN / -1
  return i128_from_mag(neg, u128_div(q, u128_pow10(total - 18u)), out);
}
// Decimal::checked_round / checked_ceil / checked_floor, decimal.rs:211-254 (how: 0 round, 1 ceil, 2 floor).  Round's negative branch
// is `-value % 10 > 5`: -2.5 rounds to -2, as written there.
__device__ __noinline__ bool dec_checked_round(i128_t v, int how, i128_t& out) {
  const bool neg = v < 0;
  const u128_t m = i128_mag(v);
  u128_t q;
  if (how == 0) {
    q = u128_div(m, kDecOne / 10u);                       // value / DECIMAL_PART_POW_MINUS_ONE
    const uint32_t digit = u128_divmod10(q);
    q += neg ? digit > 5u : digit >= 5u;
  } else {
    q = u128_div(m, kDecOne);
    const bool frac = q * kDecOne != m;
    if (frac && (how == 1) != neg) q += 1;                // ceil of a positive, floor of a negative: one step away from zero
  }
  i128_t whole;
  return i128_from_mag(neg, q, whole) && i128_mul_checked(whole, (i128_t)kDecOne, out);
}
// TryFrom<Double> for Decimal, decimal.rs:420-435: in range (NaN fails both comparisons), then `as i128`: truncating and SATURATING
__device__ __forceinline__ bool f64_to_dec(double v, i128_t& out) {
  const double shifted = __dmul_rn(v, 1e18), top = 170141183460469231731687303715884105728.0;   // 2^127
  if (!(-top <= shifted && shifted <= top)) return false;
  const uint64_t bits = (uint64_t)__double_as_longlong(shifted);
  const int e = (int)((bits >> 52) & 0x7FFu) - 1075;
  const uint64_t man = (bits & 0xFFFFFFFFFFFFFull) | ((bits >> 52) & 0x7FFu ? 1ull << 52 : 0ull);
  const u128_t mag = e >= 0 ? (u128_t)man << e : (e > -64 ? (u128_t)(man >> -e) : (u128_t)0);   // e <= 75 here
  const bool neg = bits >> 63;
  if (!neg && (mag >> 127)) { out = (i128_t)(((u128_t)1 << 127) - 1); return true; }
  out = (i128_t)(neg ? (u128_t)0 - mag : mag);
  return true;
}

// MUL / DIV, mul.rs:50-76, div.rs:51-80: kinds promote as for ADD; int and integer pairs DIVIDE as decimals
__device__ __noinline__ Val tv_muldiv(Val a, Val b, bool div) {
  const int ka = num_kind(a.tag), kb = num_kind(b.tag);
  Val r = val_tv_null();
  if (ka == NK_NONE || kb == NK_NONE) return r;
  int k = pair_kind(ka, kb);
  if (div && (k == NK_INT || k == NK_INTEGER)) k = NK_DECIMAL;
  switch (k) {
    case NK_INT: {
      int32_t z;
      if (__builtin_mul_overflow((int32_t)a.lo, (int32_t)b.lo, &z)) return r;
      r.tag = RDFGPU_TV_INT; r.lo = z; return r; }
    case NK_INTEGER: {
      long long z;
      if (__builtin_mul_overflow((long long)a.lo, (long long)b.lo, &z)) return r;
      r.tag = RDFGPU_TV_INTEGER; r.lo = z; return r; }
    case NK_FLOAT: {   // the quotient is formed in f64 and rounded once: exact for f32 operands, subnormal results included
      const float x = to_f32(a, ka), y = to_f32(b, kb);
      const float z = div ? (float)__ddiv_rn((double)x, (double)y) : __fmul_rn(x, y);
      r.tag = RDFGPU_TV_FLOAT; r.lo = (int64_t)(uint64_t)__float_as_uint(z); return r; }
    case NK_DOUBLE: {
      const double x = to_f64(a, ka), y = to_f64(b, kb);
      const double z = div ? __ddiv_rn(x, y) : __dmul_rn(x, y);
      r.tag = RDFGPU_TV_DOUBLE; r.lo = __double_as_longlong(z); return r; }
    default: {
      i128_t z;
      if (!(div ? dec_checked_div(to_dec(a, ka), to_dec(b, kb), z) : dec_checked_mul(to_dec(a, ka), to_dec(b, kb), z))) return r;
      r.tag = RDFGPU_TV_DECIMAL; set_dec(r, z); return r; }
  }
}
// f32 / f64 round: half away from zero, the sign of a zero result kept (Rust's `round`)
__device__ __forceinline__ double f64_round(double x) {
  const double t = trunc(x);
  const double r = fabs(__dsub_rn(x, t)) >= 0.5 ? __dadd_rn(t, copysign(1.0, x)) : t;   // x - trunc(x) is exact
  return copysign(r, x);
}
// NEG / PLUS / ABS / ROUND / CEIL / FLOOR: numeric.rs:20-38, round.rs:48-60, ceil.rs:48-60, floor.rs
__device__ __noinline__ Val tv_unary_numeric(Val a, uint32_t op) {
  const int k = num_kind(a.tag);
  Val r = val_tv_null();
  if (k == NK_NONE) return r;
  if (op == RDFGPU_EX_PLUS) return a;
  const bool neg_op = op == RDFGPU_EX_NEG, abs_op = op == RDFGPU_EX_ABS;
  switch (k) {
    case NK_INT: case NK_INTEGER: {
      if (!neg_op && !abs_op) return a;                                            // ROUND / CEIL / FLOOR of an integer
      if (a.lo >= 0 && abs_op) return a;
      if (a.lo == (k == NK_INT ? (int64_t)INT32_MIN : INT64_MIN)) return r;        // checked_neg / checked_abs
      a.lo = -a.lo; return a; }
    case NK_FLOAT: {
      uint32_t bits = (uint32_t)a.lo;
      if (neg_op) bits ^= 0x80000000u;
      else if (abs_op) bits &= 0x7FFFFFFFu;
      else {
        const double x = (double)__uint_as_float(bits);   // exact in f64, and so is the rounded value
        bits = __float_as_uint((float)(op == RDFGPU_EX_ROUND ? f64_round(x) : op == RDFGPU_EX_CEIL ? ceil(x) : floor(x)));
      }
      a.lo = (int64_t)(uint64_t)bits; return a; }
    case NK_DOUBLE: {
      uint64_t bits = (uint64_t)a.lo;
      if (neg_op) bits ^= 1ull << 63;
      else if (abs_op) bits &= ~(1ull << 63);
      else {
        const double x = __longlong_as_double((long long)bits);
        bits = (uint64_t)__double_as_longlong(op == RDFGPU_EX_ROUND ? f64_round(x) : op == RDFGPU_EX_CEIL ? ceil(x) : floor(x));
      }
      a.lo = (int64_t)bits; return a; }
    default: {
      const i128_t v = val_dec(a);
      i128_t z;
      if (neg_op || abs_op) {
        if (abs_op && v >= 0) return a;
        if (!i128_from_mag(false, i128_mag(v), z)) return r;                       // -MIN
        if (neg_op && v > 0) z = -v;
      } else if (!dec_checked_round(v, op == RDFGPU_EX_ROUND ? 0 : op == RDFGPU_EX_CEIL ? 1 : 2, z)) return r;
      set_dec(a, z); return a; }
  }
}
// CAST to boolean / int / integer / decimal / float / double, scalar/conversion/cast_*.rs:48-62.  Booleans cast as 0 / 1; floats reach
// the integer kinds through Decimal::try_from (decimal.rs:420-435) and a truncating division (decimal.rs:464-494); a simple literal
// would have to be parsed: the plan's run-time error, never answered differently.
__device__ __noinline__ Val tv_cast(Val a, uint32_t target, uint32_t* rt_error) {
  Val r = val_tv_null();
  int k = num_kind(a.tag);
  if (a.tag == RDFGPU_TV_BOOLEAN) { a.lo = a.lo != 0; k = NK_INTEGER; }
  else if (a.tag == RDFGPU_TV_STRING && a.aux == 0) { if (rt_error) atomicOr(rt_error, kRtCastFromString); return r; }
  else if (k == NK_NONE) return r;
  r.tag = (uint8_t)target;
  switch (target) {
    case RDFGPU_TV_BOOLEAN:   // boolean.rs:51-84
      r.lo = k == NK_FLOAT ? (__uint_as_float((uint32_t)a.lo) != 0.0f && !isnan(__uint_as_float((uint32_t)a.lo)))
           : k == NK_DOUBLE ? (__longlong_as_double(a.lo) != 0.0 && !isnan(__longlong_as_double(a.lo)))
           : k == NK_DECIMAL ? (a.lo | a.hi) != 0 : a.lo != 0;
      return r;
    case RDFGPU_TV_FLOAT: r.lo = (int64_t)(uint64_t)__float_as_uint(to_f32(a, k)); return r;
    case RDFGPU_TV_DOUBLE: r.lo = __double_as_longlong(to_f64(a, k)); return r;
    default: break;
  }
  i128_t d;
  if (k == NK_FLOAT || k == NK_DOUBLE) { if (!f64_to_dec(to_f64(a, k), d)) return val_tv_null(); }
  else d = to_dec(a, k);
  if (target == RDFGPU_TV_DECIMAL) { set_dec(r, d); return r; }
  const u128_t q = u128_div(i128_mag(d), kDecOne);   // below 2^68
  const bool neg = d < 0;
  const u128_t lim = target == RDFGPU_TV_INT ? (u128_t)1 << 31 : (u128_t)1 << 63;
  if (neg ? q > lim : q >= lim) return val_tv_null();
  r.lo = neg ? (int64_t)(0ull - (uint64_t)q) : (int64_t)(uint64_t)q;
  return r;
}

// YEAR / MONTH / DAY / HOURS / MINUTES / SECONDS, scalar/dates_and_times/*.rs: a dateTime gives an xsd:integer (SECONDS: an xsd:decimal), every
// other kind — date, time, null, a numeric — the error value (`ThinError::expected()`).  The offset rides in aux bits 16..31 beside bit 0 =
// "has a timezone" (enc_tv<true>, or the literal's `u`); without a timezone it is 0 (`unwrap_or(TimezoneOffset::UTC)`).
__device__ __noinline__ Val tv_date_part(Val a, uint32_t op) {
  Val r = val_tv_null();
  if (a.tag != RDFGPU_TV_DATE_TIME) return r;
  if (op == RDFGPU_EX_SECONDS) { r.tag = RDFGPU_TV_DECIMAL; date_seconds(a.lo, a.hi, r.lo, r.hi); return r; }
  const int tz = (a.aux & 1u) ? (int)(int16_t)(uint16_t)(a.aux >> 16) : 0;
  r.tag = RDFGPU_TV_INTEGER; r.lo = date_part(a.lo, a.hi, tz, (int)(op - RDFGPU_EX_YEAR));
  return r;
}

// EBV, effective_boolean_value.rs:99-119 : 0 / 1 / 2 (error => null)
__device__ __forceinline__ uint32_t tv_ebv(const Val& v) {
  switch (v.tag) {
    case RDFGPU_TV_BOOLEAN: case RDFGPU_TV_INT: case RDFGPU_TV_INTEGER: return v.lo != 0;
    case RDFGPU_TV_FLOAT: return __uint_as_float((uint32_t)v.lo) != 0.0f;   // NaN != 0 is true (IEEE), as in the reference
    case RDFGPU_TV_DOUBLE: return __longlong_as_double(v.lo) != 0.0;
    case RDFGPU_TV_DECIMAL: return (v.lo | v.hi) != 0;
    case RDFGPU_TV_STRING: return v.aux != 0 ? 2u : ((v.flags & RDFGPU_TVF_EMPTY_STRING) ? 0u : 1u);
    default: return 2u;
  }
}

// REGEX, scalar/strings/regex.rs:47-141: unanchored search (`Regex::is_match`) by simulating the pattern's position
// automaton with ONE u64 of state per row: next = (U follow[s] for s in cur  |  first if a match may start here)
// & byte_mask[byte].  Simple and language-tagged strings match; every other kind is the error value.
// `rhs_lang` >= 0: CONTAINS / STRSTARTS / STRENDS argument compatibility (string_literal.rs:80-95) — the constant has no
// language (0) or the value's; REGEX passes -1 (no such rule).
// The error value with aux = kRegexNeedsUnicode: "a Perl class / word boundary met a non-ASCII subject" — a per-term
// verdict pass (no plan to fail) records it as verdict 3; a row that actually reads such a verdict raises the run-time error.
constexpr uint32_t kRegexNeedsUnicode = 0xFFFFFFFFu;
// The bytes of a string value: false when it has none on the device (not a string; an id without a lexical form in the heap).
struct StrBytes { const uint8_t* p; uint64_t len; uint32_t xf; };   // xf: 0 as stored, 1 ASCII upper, 2 ASCII lower
__device__ __forceinline__ bool str_bytes_of(const uint8_t* str_consts, const RegexProg* regex, const uint64_t* str_off, const uint8_t* heap, uint64_t n_str_ids, const Val& v, StrBytes& s) {
  if (v.tag != RDFGPU_TV_STRING) return false;
  s.xf = (v.flags & kStrUpper) ? 1u : (v.flags & kStrLower) ? 2u : 0u;
  if (v.pad == 2) {
    if (str_consts == nullptr) return false;
    s.p = str_consts + regex[(uint32_t)v.hi].first + ((uint64_t)v.lo >> 32); s.len = (uint32_t)v.lo;
    return true;
  }
  const uint64_t id = (uint64_t)(uint32_t)v.hi;
  if (str_off == nullptr || id == 0 || id >= n_str_ids) return false;   // (a string literal of the plan given by rank only has no bytes here)
  const uint64_t b0 = str_off[id];
  if (v.pad == 0) { s.p = heap + b0; s.len = str_off[id + 1] - b0; }
  else { s.p = heap + b0 + ((uint64_t)v.lo >> 32); s.len = (uint32_t)v.lo; }
  return true;
}
__device__ __forceinline__ bool str_bytes(const ExprProgram* prog, const TypedTable& t, const Val& v, StrBytes& s) {
  if (prog == nullptr) return v.pad == 2 ? false : str_bytes_of(nullptr, nullptr, t.str_off, t.heap, t.n_str_ids, v, s);
  return str_bytes_of(prog->str_consts, prog->regex, t.str_off, t.heap, t.n_str_ids, v, s);
}
__device__ __forceinline__ uint8_t str_at(const StrBytes& s, uint64_t i) {
  uint8_t b = s.p[i];
  if (s.xf == 1u && b >= 'a' && b <= 'z') b -= 32;
  if (s.xf == 2u && b >= 'A' && b <= 'Z') b += 32;
  return b;
}
__device__ __forceinline__ Val tv_regex(const RegexProg& p, const TypedTable& t, const Val& v, int64_t rhs_lang = -1, const ExprProgram* prog = nullptr) {
  if (v.tag != RDFGPU_TV_STRING || p.always_error || t.str_off == nullptr) return val_tv_null();
  if (rhs_lang > 0 && (int64_t)v.aux != rhs_lang) return val_tv_null();
  StrBytes sb;
  if (!str_bytes(prog, t, v, sb)) return val_tv_null();   // a string literal of the plan has no lexical form on the device
  const uint64_t len = sb.len;
  auto at = [&](uint64_t i) -> uint8_t { return sb.xf ? str_at(sb, i) : sb.p[i]; };
  if (p.ascii_only) {   // `\d \w \s \b` are compiled with their ASCII members: exact on ASCII subjects only
    bool non_ascii = false;
    for (uint64_t i = 0; i < len; i++) non_ascii = non_ascii || sb.p[i] >= 0x80;
    if (non_ascii) {
      if (t.rt_error) atomicOr(t.rt_error, 1u);
      Val e = val_tv_null(); e.aux = kRegexNeedsUnicode; return e;
    }
  }
  auto start_ok = [&](uint64_t i) { return !p.anchor_start || i == 0 || (p.ml_start && at(i - 1) == '\n'); };
  auto end_ok = [&](uint64_t i) { return !p.anchor_end || i == len || (p.ml_end && at(i) == '\n'); };
  if (!p.has_assert) {
    if (p.nullable) {
      if (!p.anchor_start && !p.anchor_end) return val_tv_bool(true);
      for (uint64_t i = 0; i <= len; i++) if (start_ok(i) && end_ok(i)) return val_tv_bool(true);
    }
    uint64_t cur = 0;
    for (uint64_t i = 0; i < len; i++) {
      uint64_t nxt = start_ok(i) ? p.first : 0;
      for (uint64_t c = cur; c; c &= c - 1) nxt |= p.follow[__builtin_ctzll(c)];
      cur = nxt & p.byte_mask[at(i)];
      if ((cur & p.last) && end_ok(i + 1)) return val_tv_bool(true);
    }
    return val_tv_bool(false);
  }
  // with `\b` / `\B`: every crossing also looks at the word-boundary flag of the point it crosses (ASCII word characters)
  auto isw = [](uint8_t c) { return (c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_'; };
  auto bnd = [&](uint64_t i) { const bool a = i > 0 && isw(at(i - 1)), b = i < len && isw(at(i)); return a != b; };
  for (uint64_t i = 0; i <= len; i++)
    if (start_ok(i) && end_ok(i) && (p.nullable || (bnd(i) ? p.nullable_b : p.nullable_nb))) return val_tv_bool(true);
  uint64_t cur = 0;
  for (uint64_t i = 0; i < len; i++) {
    const bool bi = bnd(i);
    uint64_t nxt = start_ok(i) ? (p.first | (bi ? p.first_b : p.first_nb)) : 0;
    for (uint64_t c = cur; c; c &= c - 1) { const int k = __builtin_ctzll(c); nxt |= p.follow[k] | (bi ? p.follow_b[k] : p.follow_nb[k]); }
    cur = nxt & p.byte_mask[at(i)];
    if ((cur & (p.last | (bnd(i + 1) ? p.last_b : p.last_nb))) && end_ok(i + 1)) return val_tv_bool(true);
  }
  return val_tv_bool(false);
}
// ---- string-valued expressions over views ----------------------------------------------------------------------------
__device__ __forceinline__ Val val_str_view(uint8_t where, uint32_t src, uint64_t first, uint64_t bytes, uint32_t lang, uint8_t case_bits) {
  Val v = val_tv_null();
  v.tag = RDFGPU_TV_STRING; v.pad = where; v.hi = (int64_t)(uint64_t)src; v.lo = (int64_t)((first << 32) | (bytes & 0xFFFFFFFFull));
  v.aux = lang; v.flags = (uint8_t)((bytes == 0 ? RDFGPU_TVF_EMPTY_STRING : 0u) | case_bits);
  return v;
}
// STR(term) over an object id: the lexical form as written (str.rs:42 in the plain-term encoding)
__device__ __forceinline__ Val tv_str_of_id(const TypedTable& t, uint32_t id) {
  if (t.str_off == nullptr || id == 0 || (uint64_t)id >= t.n_str_ids) return val_tv_null();
  return val_str_view(1, id, 0, t.str_off[id + 1] - t.str_off[id], 0u, 0);
}
// STRLEN, strlen.rs: `chars().count()` = bytes that do not continue a UTF-8 sequence
__device__ __forceinline__ Val tv_strlen(const ExprProgram* prog, const TypedTable& t, const Val& v) {
  StrBytes s;
  if (!str_bytes(prog, t, v, s)) return val_tv_null();
  int64_t n = 0;
  for (uint64_t i = 0; i < s.len; i++) n += (s.p[i] & 0xC0u) != 0x80u;
  Val r = val_tv_null(); r.tag = RDFGPU_TV_INTEGER; r.lo = n; return r;
}
// SUBSTR(source, start[, length]), sub_str.rs:83-121: 1-based characters; usize::try_from of a negative argument, and start 0, are errors
__device__ __forceinline__ Val tv_substr(const ExprProgram* prog, const TypedTable& t, const Val& v, const Val& start, const Val* length) {
  StrBytes s;
  if (!str_bytes(prog, t, v, s)) return val_tv_null();
  auto as_int = [&](const Val& x, int64_t& out) {
    if (x.tag == RDFGPU_TV_INT || x.tag == RDFGPU_TV_INTEGER) { out = x.lo; return true; }
    if (num_kind(x.tag) != NK_NONE && t.rt_error) atomicOr(t.rt_error, kRtStringUnsupported);   // float / double / decimal -> Integer::try_from is not restated
    return false;
  };
  int64_t st = 0, ln = 0;
  if (!as_int(start, st) || st < 1) return val_tv_null();
  if (length && (!as_int(*length, ln) || ln < 0)) return val_tv_null();
  uint64_t chars = 0, b0 = s.len, b1 = s.len;                  // byte offsets of character (st - 1) and of character (st - 1 + ln)
  const uint64_t c0 = (uint64_t)st - 1, c1 = length ? c0 + (uint64_t)ln : ~0ull;
  for (uint64_t i = 0; i < s.len; i++) {
    if ((s.p[i] & 0xC0u) == 0x80u) continue;
    if (chars == c0) b0 = i;
    if (chars == c1) { b1 = i; break; }
    chars++;
  }
  if (b0 > b1) b0 = b1;
  const uint64_t base = v.pad == 0 ? 0ull : ((uint64_t)v.lo >> 32);
  return val_str_view(v.pad == 0 ? 1 : v.pad, (uint32_t)v.hi, base + b0, b1 - b0, v.aux, (uint8_t)(v.flags & (kStrUpper | kStrLower)));
}
// UCASE / LCASE: ASCII letters on the device; any non-ASCII byte raises the plan's run-time error (Unicode case tables are not restated)
__device__ __forceinline__ Val tv_case(const ExprProgram* prog, const TypedTable& t, const Val& v, bool upper) {
  StrBytes s;
  if (!str_bytes(prog, t, v, s)) return val_tv_null();
  bool non_ascii = false;
  for (uint64_t i = 0; i < s.len; i++) non_ascii = non_ascii || s.p[i] >= 0x80;
  if (non_ascii) { if (t.rt_error) atomicOr(t.rt_error, kRtStringUnsupported); return val_tv_null(); }
  const uint64_t base = v.pad == 0 ? 0ull : ((uint64_t)v.lo >> 32);
  return val_str_view(v.pad == 0 ? 1 : v.pad, (uint32_t)v.hi, base, s.len, v.aux, upper ? kStrUpper : kStrLower);
}
// STRBEFORE / STRAFTER(a, b), str_before.rs / str_after.rs: both string literals, b without a language or with a's (string_literal.rs:80-95);
// the part of a before / behind the first occurrence of b, with a's language — a window of a's bytes, nothing is copied (UTF-8 is
// self-synchronising: a byte-wise match of valid UTF-8 starts on a character boundary); no occurrence => the simple literal "".
__device__ __forceinline__ Val tv_strpart(const ExprProgram* prog, const TypedTable& t, const Val& a, const Val& b, bool after) {
  if (a.tag != RDFGPU_TV_STRING || b.tag != RDFGPU_TV_STRING) return val_tv_null();
  if (b.aux != 0 && b.aux != a.aux) return val_tv_null();                     // incompatible arguments: error
  StrBytes x, y;
  if (!str_bytes(prog, t, a, x) || !str_bytes(prog, t, b, y)) return val_tv_null();
  const uint64_t base = a.pad == 0 ? 0ull : ((uint64_t)a.lo >> 32);
  const uint8_t kind = a.pad == 0 ? 1 : a.pad, cs = (uint8_t)(a.flags & (kStrUpper | kStrLower));
  uint64_t pos = ~0ull;
  if (y.len <= x.len) {
    for (uint64_t i = 0; i + y.len <= x.len && pos == ~0ull; i++) {
      bool eq = true;
      for (uint64_t j = 0; j < y.len && eq; j++) eq = str_at(x, i + j) == str_at(y, j);
      if (eq) pos = i;
    }
  }
  if (pos == ~0ull) return val_str_view(kind, (uint32_t)a.hi, base, 0, 0u, 0);  // "" without a language
  return after ? val_str_view(kind, (uint32_t)a.hi, base + pos + y.len, x.len - pos - y.len, a.aux, cs)
               : val_str_view(kind, (uint32_t)a.hi, base, pos, a.aux, cs);
}
// CAST_STRING, cast_string.rs:51-76, over an object id (enc_tv keeps the id for strings only): a named node, a simple literal, a
// language-tagged string and an other literal give their lexical form as a simple literal — a view of the heap; a blank node and null are
// the error value; booleans, numbers, dateTime / date / time and durations are FORMATTED there (format_value / to_string), bytes a view
// cannot express: the plan's run-time error.
__device__ __forceinline__ Val tv_cast_string(const TypedTable& t, uint32_t id) {
  if (id == 0 || (uint64_t)id >= t.n_ids) return val_tv_null();
  const uint8_t tag = (uint8_t)(reinterpret_cast<const uint32_t*>(t.tv + id)[3] & 0xffu);
  if (tag == RDFGPU_TV_NULL || tag == RDFGPU_TV_BLANK_NODE) return val_tv_null();
  if (tag != RDFGPU_TV_NAMED_NODE && tag != RDFGPU_TV_STRING && tag != RDFGPU_TV_OTHER) {
    if (t.rt_error) atomicOr(t.rt_error, kRtStringUnsupported);
    return val_tv_null();
  }
  return tv_str_of_id(t, id);
}
struct LexAt {
  const uint8_t* p;
  __device__ __forceinline__ uint8_t operator()(uint32_t i) const { return p[i]; }
};
// The cast of a simple literal's bytes is two out-of-line leaves, and the calling kernel carries only the resolution of the bytes
// (str_bytes) and the calls: what a hosting kernel pays is the registers a leaf writes and whatever is inlined around the call, so the
// leaves are kept under what tv_unary_numeric writes and even the run-time flags are raised inside them.  They take the resolved bytes,
// not the program or the typed table (an address of those handed to a call would pin the kernel's copy in scratch).
// lex_words_bytes: the literals that are words — the case-sensitive boolean (of the bytes as a UCASE / LCASE view maps them) and inf /
// infinity / nan of a float / double; p == nullptr: the operand has no lexical form on the device.  pad = LEX_NOT_SPECIAL: a number.
// lex_number_bytes: int / integer / decimal and the numbers of float / double, from the bytes as stored: an ASCII case mapping cannot
// change what those grammars answer (digits, signs, '.', 'e' / 'E').
static __device__ __noinline__ Val lex_words_bytes(const uint8_t* p, uint32_t len, uint32_t xf, uint32_t target, uint32_t* rt_error) {
  Val r = val_tv_null();
  if (p == nullptr) { if (rt_error) atomicOr(rt_error, kRtStringUnsupported); return r; }   // refused loudly (check_program refuses a rank-only literal at compile)
  if (len >= kLexMaxLen) { if (rt_error) atomicOr(rt_error, kRtLexParse); return r; }        // the parsers count in 32 bits: declined
  int st = LEX_NOT_SPECIAL;
  uint64_t bits = 0;
  if (target == RDFGPU_TV_BOOLEAN) {
    StrBytes s; s.p = p; s.len = len; s.xf = xf;
    bool b = false;
    st = lex_parse_boolean([&](uint32_t i) { return str_at(s, i); }, len, b);
    bits = b;
  } else if (target == RDFGPU_TV_FLOAT) st = lex_parse_float_special<true>(LexAt{p}, len, bits);
  else if (target == RDFGPU_TV_DOUBLE) st = lex_parse_float_special<false>(LexAt{p}, len, bits);
  if (st == LEX_DECLINED && rt_error) atomicOr(rt_error, kRtLexParse);
  if (st == LEX_OK) { r.tag = (uint8_t)target; r.lo = (int64_t)bits; }
  else if (st == LEX_NOT_SPECIAL) r.pad = LEX_NOT_SPECIAL;
  return r;
}
static __device__ __noinline__ Val lex_number_bytes(const uint8_t* p, uint32_t len, uint32_t target, uint32_t* rt_error) {
  const LexAt at{p};
  Val r = val_tv_null();
  int st = LEX_ERROR;
  switch (target) {
    case RDFGPU_TV_INT: { long long v = 0; st = lex_parse_i64(at, len, (long long)INT32_MIN, (long long)INT32_MAX, v); r.lo = v; break; }
    case RDFGPU_TV_INTEGER: { long long v = 0; st = lex_parse_i64(at, len, INT64_MIN, INT64_MAX, v); r.lo = v; break; }
    case RDFGPU_TV_DECIMAL: { uint64_t lo = 0, hi = 0; st = lex_parse_decimal(at, len, lo, hi); r.lo = (int64_t)lo; r.hi = (int64_t)hi; break; }
    case RDFGPU_TV_FLOAT: { uint64_t bits = 0; st = lex_parse_float_number<true>(at, len, bits); r.lo = (int64_t)bits; break; }
    case RDFGPU_TV_DOUBLE: { uint64_t bits = 0; st = lex_parse_float_number<false>(at, len, bits); r.lo = (int64_t)bits; break; }
    default: break;
  }
  if (st == LEX_DECLINED && rt_error) atomicOr(rt_error, kRtLexParse);
  if (st != LEX_OK) return val_tv_null();
  r.tag = (uint8_t)target;
  return r;
}
// CAST_LEX: RDFGPU_EX_CAST on every operand but a simple literal (a dictionary string, a window, a case-mapped view or a constant with
// bytes, no language), whose bytes are parsed as the reference's FromStr impls do.  (eval_program sends every other operand to tv_cast.)
__device__ __forceinline__ Val tv_cast_lex(const Val& a, uint32_t target, const ExprProgram* prog, const TypedTable& t) {
  StrBytes s;
  if (!str_bytes(prog, t, a, s)) { s.p = nullptr; s.len = 0; s.xf = 0; }
  const uint32_t len = s.len < kLexMaxLen ? (uint32_t)s.len : kLexMaxLen;   // (kLexMaxLen: 256 MB or more, which the words leaf declines)
  Val r = lex_words_bytes(s.p, len, s.xf, target, t.rt_error);
  if (r.pad == LEX_NOT_SPECIAL) r = lex_number_bytes(s.p, len, target, t.rt_error);
  return r;
}
// two strings of which at least one is a view: `str` order of their bytes (typed_value.rs:184-196 compares the values), same language only
__device__ __forceinline__ bool str_is_view(const Val& v) { return v.tag == RDFGPU_TV_STRING && (v.pad != 0 || (v.flags & (kStrUpper | kStrLower))); }
__device__ __forceinline__ int tv_cmp_string_views(const ExprProgram* prog, const TypedTable& t, const Val& a, const Val& b) {
  if (a.aux != b.aux) return ORD_NONE;
  StrBytes x, y;
  if (!str_bytes(prog, t, a, x) || !str_bytes(prog, t, b, y)) {   // one side has no bytes on the device: refused loudly, not answered as an error value
    if (t.rt_error) atomicOr(t.rt_error, kRtStringUnsupported);
    return ORD_NONE;
  }
  const uint64_t n = x.len < y.len ? x.len : y.len;
  for (uint64_t i = 0; i < n; i++) { const uint8_t p = str_at(x, i), q = str_at(y, i); if (p != q) return p < q ? -1 : 1; }
  return x.len < y.len ? -1 : x.len > y.len;
}
// REGEX(value, ?pattern): the pattern is a per-row simple literal (regex.rs:59-76, compiled per row there); here every
// DISTINCT pattern the host announced was compiled at plan time and the row picks its program by the pattern's object id.
// A pattern that was not announced raises the plan's run-time error (never answered as if it did not match).
__device__ __forceinline__ Val tv_regex_var(const RegexProg* progs, uint32_t first, uint32_t count, const TypedTable& t, const Val& v, const Val& pat, const ExprProgram* prog = nullptr) {
  if (pat.tag != RDFGPU_TV_STRING || pat.aux != 0 || pat.pad != 0) return val_tv_null();   // the pattern must be a simple literal of the dictionary
  const uint32_t pid = (uint32_t)pat.hi;
  for (uint32_t k = 0; k < count; k++) if (progs[first + k].pattern_id == pid) return tv_regex(progs[first + k], t, v, -1, prog);
  if (t.rt_error) atomicOr(t.rt_error, 2u);
  return val_tv_null();
}

// IS_IRI / IS_BLANK / IS_LITERAL / IS_NUMERIC, scalar/terms/is_*.rs: the null value is the error value (`ThinError::expected`); a string
// view is a literal like the string it is a window of (its tag is STRING).
__device__ __forceinline__ Val tv_term_test(const Val& a, uint32_t op) {
  if (a.tag == RDFGPU_TV_NULL) return val_tv_null();
  const bool node = a.tag == RDFGPU_TV_NAMED_NODE || a.tag == RDFGPU_TV_BLANK_NODE;
  return val_tv_bool(op == RDFGPU_EX_IS_IRI ? a.tag == RDFGPU_TV_NAMED_NODE : op == RDFGPU_EX_IS_BLANK ? a.tag == RDFGPU_TV_BLANK_NODE
                   : op == RDFGPU_EX_IS_LITERAL ? !node : num_kind(a.tag) != NK_NONE);
}

// LEX: whether the extended cases (the ops with kOpExtended, expr_ops.hpp) are compiled in.  The first of them was `case
// RDFGPU_EX_CAST_LEX`: the byte resolution and the calls around the leaves cost a hosting kernel one or two registers, which moved kernels
// that sit on an occupancy step; so every host exists twice, and the instantiation without the cases is, register for register, the kernel
// it was before the op existed.  Plans pick by program_has_lex / NodeInfo::lex.
// The date parts (YEAR .. SECONDS) live in the same instantiations, for the same reason: their case, and the timezone offset that ENC_TV
// then has to carry (enc_tv<true>), exist only where LEX is true.  So do IF, COALESCE and the term tests.  Their operands are all
// evaluated before the op is reached (the program is postfix): eager, as in the reference, and a run-time refusal an operand raised stays
// raised whichever operand the op then picks.
template <bool LEX = false, class ColFn>
__device__ __forceinline__ Val eval_program(const ExprProgram& prog, const TypedTable& tt, ColFn col) {
  Val st[kMaxStack];
  int sp = 0;
  for (uint32_t pc = 0; pc < prog.n; pc++) {
    const rdfgpu_expr_node& e = prog.nodes[pc];
    Val v;
    switch (e.op) {
      case RDFGPU_EX_COLUMN: v = val_id(col(e.u)); break;
      case RDFGPU_EX_LIT_ID: v = val_id(e.u); break;
      case RDFGPU_EX_LIT_TV: v = val_tv_null(); v.tag = e.tag; v.flags = e.flags; v.aux = e.u; v.lo = e.lo; v.hi = e.hi; break;
      case RDFGPU_EX_LIT_BOOL: v = val_bool(e.u > 2 ? 2 : e.u); break;
      case RDFGPU_EX_ENC_TV: v = enc_tv<LEX>(tt, (uint32_t)st[--sp].lo); break;
      case kExAggValue: v = agg_value_load(e, (uint32_t)st[--sp].lo); break;
      case RDFGPU_EX_GT: case RDFGPU_EX_LT: case RDFGPU_EX_GEQ: case RDFGPU_EX_LEQ: case RDFGPU_EX_EQ: case RDFGPU_EX_NEQ: {
        const Val b = st[--sp]; const Val a = st[--sp];
        const int o = (a.tag == RDFGPU_TV_STRING && b.tag == RDFGPU_TV_STRING && (str_is_view(a) || str_is_view(b))) ? tv_cmp_string_views(&prog, tt, a, b) : tv_partial_cmp(a, b);
        if (o == ORD_NONE) { v = val_tv_null(); break; }
        const bool r = e.op == RDFGPU_EX_GT ? o > 0 : e.op == RDFGPU_EX_LT ? o < 0 : e.op == RDFGPU_EX_GEQ ? o >= 0
                     : e.op == RDFGPU_EX_LEQ ? o <= 0 : e.op == RDFGPU_EX_EQ ? o == 0 : o != 0;
        v = val_tv_bool(r); break; }
      case RDFGPU_EX_ADD: case RDFGPU_EX_SUB: { const Val b = st[--sp]; const Val a = st[--sp]; v = tv_arith(a, b, e.op == RDFGPU_EX_SUB); break; }
      case RDFGPU_EX_MUL: case RDFGPU_EX_DIV: { const Val b = st[--sp]; const Val a = st[--sp]; v = tv_muldiv(a, b, e.op == RDFGPU_EX_DIV); break; }
      case RDFGPU_EX_NEG: case RDFGPU_EX_PLUS: case RDFGPU_EX_ABS: case RDFGPU_EX_ROUND: case RDFGPU_EX_CEIL: case RDFGPU_EX_FLOOR:
        v = tv_unary_numeric(st[--sp], e.op); break;
      case RDFGPU_EX_CAST: v = tv_cast(st[--sp], e.u, tt.rt_error); break;
      case RDFGPU_EX_CAST_LEX:   // (a simple literal is parsed; every other operand is a CAST)
        if constexpr (LEX) { const Val a = st[--sp]; v = a.tag == RDFGPU_TV_STRING && a.aux == 0 ? tv_cast_lex(a, e.u, &prog, tt) : tv_cast(a, e.u, tt.rt_error); }
        else v = val_bool(2);     // (not reached: a program with the op runs in a LEX instantiation)
        break;
      case RDFGPU_EX_CAST_STRING: v = tv_cast_string(tt, (uint32_t)st[--sp].lo); break;
      case RDFGPU_EX_YEAR: case RDFGPU_EX_MONTH: case RDFGPU_EX_DAY: case RDFGPU_EX_HOURS: case RDFGPU_EX_MINUTES: case RDFGPU_EX_SECONDS:
        if constexpr (LEX) v = tv_date_part(st[--sp], e.op);
        else v = val_bool(2);     // (not reached: a program with a date part runs in a LEX instantiation)
        break;
      case RDFGPU_EX_IF:   // (test, then, else): Boolean::try_from of the test — a boolean typed value, or the error value
        if constexpr (LEX) { const Val no = st[--sp]; const Val yes = st[--sp]; const Val test = st[--sp];
          v = test.tag != RDFGPU_TV_BOOLEAN ? val_tv_null() : test.lo != 0 ? yes : no; }
        else v = val_bool(2);     // (not reached: a program with a functional form or a term test runs in a LEX instantiation)
        break;
      case RDFGPU_EX_COALESCE:   // the first of the `u` operands that is not the error value (TV) / not 0 (ID), else the last: the error value / 0
        if constexpr (LEX) {
          const int k = e.u < 1u ? 1 : e.u > (uint32_t)sp ? sp : (int)e.u;   // (check_program: 1 <= u <= the stack's depth)
          sp -= k;
          v = st[sp];
          for (int q = 1; q < k; q++) { const bool unset = v.kind == VK_ID ? v.lo == 0 : v.tag == RDFGPU_TV_NULL; if (unset) v = st[sp + q]; }
        } else v = val_bool(2);
        break;
      case RDFGPU_EX_IS_IRI: case RDFGPU_EX_IS_BLANK: case RDFGPU_EX_IS_LITERAL: case RDFGPU_EX_IS_NUMERIC:
        if constexpr (LEX) v = tv_term_test(st[--sp], e.op);
        else v = val_bool(2);
        break;
      case RDFGPU_EX_EBV: v = val_bool(tv_ebv(st[--sp])); break;
      case RDFGPU_EX_REGEX: v = tv_regex(prog.regex[e.u], tt, st[--sp], -1, &prog); break;
      case RDFGPU_EX_REGEX_VAR: { const Val pat = st[--sp]; const Val val = st[--sp]; v = tv_regex_var(prog.regex, e.u, (uint32_t)e.lo, tt, val, pat, &prog); break; }
      case RDFGPU_EX_CONTAINS: case RDFGPU_EX_STRSTARTS: case RDFGPU_EX_STRENDS: v = tv_regex(prog.regex[e.u], tt, st[--sp], e.lo < 0 ? 0 : e.lo, &prog); break;
      case RDFGPU_EX_STR: v = tv_str_of_id(tt, (uint32_t)st[--sp].lo); break;
      case RDFGPU_EX_LIT_STR: v = val_str_view(2, e.u, 0, prog.regex[e.u].n_pos, (uint32_t)(e.lo < 0 ? 0 : e.lo), 0); break;
      case RDFGPU_EX_STRLEN: v = tv_strlen(&prog, tt, st[--sp]); break;
      case RDFGPU_EX_STRBEFORE: case RDFGPU_EX_STRAFTER: { const Val b2 = st[--sp]; const Val a2 = st[--sp]; v = tv_strpart(&prog, tt, a2, b2, e.op == RDFGPU_EX_STRAFTER); break; }
      case RDFGPU_EX_SUBSTR: {
        if (e.u == 3) { const Val ln = st[--sp]; const Val from = st[--sp]; const Val src = st[--sp]; v = tv_substr(&prog, tt, src, from, &ln); }
        else { const Val from = st[--sp]; const Val src = st[--sp]; v = tv_substr(&prog, tt, src, from, nullptr); }
        break; }
      case RDFGPU_EX_UCASE: case RDFGPU_EX_LCASE: v = tv_case(&prog, tt, st[--sp], e.op == RDFGPU_EX_UCASE); break;
      case RDFGPU_EX_LANG_IN: {   // LANGMATCHES(LANG(v), range): one verdict bit per language id (bit 0 = no language)
        const Val a = st[--sp];
        const RegexProg& p = prog.regex[e.u];
        v = val_tv_null();
        if (a.tag == RDFGPU_TV_NULL || a.tag == RDFGPU_TV_NAMED_NODE || a.tag == RDFGPU_TV_BLANK_NODE) break;
        const uint32_t lang = a.tag == RDFGPU_TV_STRING ? a.aux : 0u;
        if (lang < p.n_pos) v = val_tv_bool((p.byte_mask[lang >> 6] >> (lang & 63u)) & 1ull);
        break; }
      case RDFGPU_EX_ID_EQ: case RDFGPU_EX_ID_NEQ: {
        const uint32_t b = (uint32_t)st[--sp].lo, a = (uint32_t)st[--sp].lo;
        v = val_bool((a == 0 || b == 0) ? 2u : (uint32_t)((a == b) == (e.op == RDFGPU_EX_ID_EQ))); break; }
      case RDFGPU_EX_AND: { const uint32_t b = (uint32_t)st[--sp].lo, a = (uint32_t)st[--sp].lo;
        v = val_bool((a == 0 || b == 0) ? 0u : (a == 2 || b == 2) ? 2u : 1u); break; }
      case RDFGPU_EX_OR: { const uint32_t b = (uint32_t)st[--sp].lo, a = (uint32_t)st[--sp].lo;
        v = val_bool((a == 1 || b == 1) ? 1u : (a == 2 || b == 2) ? 2u : 0u); break; }
      case RDFGPU_EX_NOT: { const uint32_t a = (uint32_t)st[--sp].lo; v = val_bool(a == 2 ? 2u : 1u - a); break; }
      case RDFGPU_EX_IS_COMPATIBLE: { const uint32_t b = (uint32_t)st[--sp].lo, a = (uint32_t)st[--sp].lo; v = val_bool(a == 0 || b == 0 || a == b); break; }
      case RDFGPU_EX_BOUND: v = val_bool(st[--sp].lo != 0); break;
      case RDFGPU_EX_BOOL_AS_TV: { const uint32_t a = (uint32_t)st[--sp].lo; v = a == 2 ? val_tv_null() : val_tv_bool(a != 0); break; }
      default: v = val_bool(2); break;
    }
    st[sp++] = v;
  }
  return st[0];
}

}  // namespace rdfgpu
