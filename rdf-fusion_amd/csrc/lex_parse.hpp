// lex_parse.hpp — the lexical forms of xsd:boolean / int / integer / decimal / float / double, parsed per row (RDFGPU_EX_CAST_LEX).
//
// Restates, on bytes reached through an accessor (a string view maps ASCII case while it is read, expr_device.hpp: str_at):
//   boolean   lib/model/src/xsd/boolean.rs:108-115            exactly true / 1 / false / 0
//   int       i32::from_str, integer: i64::from_str            an optional sign, at least one digit, nothing else, checked range
//   decimal   Decimal::from_str  lib/model/src/xsd/decimal.rs:496-568   (\+|-)?([0-9]+(\.[0-9]*)?|\.[0-9]+), value * 10^18 in a checked i128
//   float     f32::from_str (float.rs:182-189), double: f64::from_str   Rust std's grammar, correctly rounded, ONE rounding to the target
//
// Decimal to binary: Clinger's exact case (mantissa and power of ten both exact in the target: one IEEE operation), else Eisel-Lemire
// (D. Lemire, "Number parsing at a gigabyte per second", 2021) over the 128-bit powers of five of lex_pow5_table.hpp.  A mantissa is
// cut to its first 19 significant digits; when digits were dropped, w and w + 1 are both converted and must agree.  Where Eisel-Lemire
// cannot decide (the half-way neighbourhood in which Rust falls back to its big-decimal path), or w and w + 1 disagree, the answer is
// LEX_DECLINED: the caller refuses loudly, nothing is ever answered differently.  Per-row state is a handful of 64-bit registers.
//
// Plain C++: with HIP, LEX_HD is __host__ __device__ and the table lives in device memory (one copy per code object that converts);
// without, both are empty and the same text runs in a stand-alone host program (tests/host/lex_parse_checks.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LEX_HD __host__ __device__ __forceinline__
#if defined(__HIP_DEVICE_COMPILE__)
#define LEX_TABLE_QUAL __device__ const
#else
#define LEX_TABLE_QUAL const
#endif
#else
#define LEX_HD inline
#define LEX_TABLE_QUAL const
#endif

#if defined(__clang__)
#define LEX_NOUNROLL _Pragma("nounroll")   // a byte at a time: an unrolled scan keeps a register per byte in flight, in every kernel that calls
#else
#define LEX_NOUNROLL
#endif

#include "lex_pow5_table.hpp"

namespace rdfgpu {

enum { LEX_OK = 0, LEX_ERROR = 1, LEX_DECLINED = 2 };   // parsed / not in the grammar or out of range (the error value) / cannot decide

typedef unsigned __int128 lex_u128;

// boolean.rs:108-115
template <class At> LEX_HD int lex_parse_boolean(At at, uint32_t n, bool& out) {
  if (n == 1 && (at(0) == '1' || at(0) == '0')) { out = at(0) == '1'; return LEX_OK; }
  if (n == 4 && at(0) == 't' && at(1) == 'r' && at(2) == 'u' && at(3) == 'e') { out = true; return LEX_OK; }
  if (n == 5 && at(0) == 'f' && at(1) == 'a' && at(2) == 'l' && at(3) == 's' && at(4) == 'e') { out = false; return LEX_OK; }
  return LEX_ERROR;
}

// i64::from_str, and i32::from_str through the bounds
template <class At> LEX_HD int lex_parse_i64(At at, uint32_t n, long long lo_bound, long long hi_bound, long long& out) {
  uint32_t i = 0; bool neg = false;
  if (n && (at(0) == '+' || at(0) == '-')) { neg = at(0) == '-'; i = 1; }
  if (i >= n) return LEX_ERROR;
  long long v = 0;
  LEX_NOUNROLL for (; i < n; i++) {
    const uint8_t c = at(i);
    if (c < '0' || c > '9') return LEX_ERROR;
    const long long d = c - '0';
    if (__builtin_mul_overflow(v, 10ll, &v)) return LEX_ERROR;
    if (neg ? __builtin_sub_overflow(v, d, &v) : __builtin_add_overflow(v, d, &v)) return LEX_ERROR;
  }
  if (v < lo_bound || v > hi_bound) return LEX_ERROR;
  out = v; return LEX_OK;
}

// Decimal::from_str, decimal.rs:496-568.  The reference accumulates a SIGNED i128 with checked steps and multiplies by the remaining power
// of ten at the end; magnitudes grow monotonically, so checking every step's magnitude against the sign's bound is the same test.
// out_lo / out_hi: the two's-complement i128.
template <class At> LEX_HD int lex_parse_decimal(At at, uint32_t n, uint64_t& out_lo, uint64_t& out_hi) {
  if (n == 0) return LEX_ERROR;
  uint32_t i = 0; bool neg = false;
  if (at(0) == '+') i = 1; else if (at(0) == '-') { neg = true; i = 1; }
  const lex_u128 top = (lex_u128)1 << 127;
  const lex_u128 lim = (((lex_u128)0x0CCCCCCCCCCCCCCCull) << 64) | (lex_u128)0xCCCCCCCCCCCCCCCCull;   // 2^127 / 10, rounded down
  lex_u128 v = 0;
  auto push = [&](uint8_t c) {   // v = v * 10 + digit inside the sign's range
    if (v > lim) return false;
    v = v * 10u + (lex_u128)(c - '0');
    return neg ? v <= top : v < top;
  };
  auto digit = [&](uint32_t k) { const uint8_t c = at(k); return c >= '0' && c <= '9'; };
  const bool before = i < n && digit(i);
  LEX_NOUNROLL for (; i < n && digit(i); i++) if (!push(at(i))) return LEX_ERROR;
  uint64_t exp = 1000000000000000000ull;
  if (i < n) {
    if (at(i) != '.') return LEX_ERROR;
    i++;
    if (i >= n && !before) return LEX_ERROR;                   // only a dot
    uint32_t end = n;
    LEX_NOUNROLL while (end > i && at(end - 1) == '0') end--;               // trailing zeros carry nothing
    LEX_NOUNROLL for (; i < end; i++) {
      if (!digit(i)) return LEX_ERROR;
      exp /= 10;
      if (!push(at(i))) return LEX_ERROR;
    }
    if (exp == 0) return LEX_ERROR;                            // more than 18 fraction digits
  } else if (!before) return LEX_ERROR;
  // v * exp over 64-bit limbs (exp < 2^64)
  const lex_u128 p0 = (lex_u128)(uint64_t)v * exp;
  const lex_u128 p1 = (lex_u128)(uint64_t)(v >> 64) * exp + (p0 >> 64);
  if (p1 >> 64) return LEX_ERROR;
  const lex_u128 m = (p1 << 64) | (lex_u128)(uint64_t)p0;
  if (neg ? m > top : m >= top) return LEX_ERROR;
  const lex_u128 r = neg ? (lex_u128)0 - m : m;
  out_lo = (uint64_t)r; out_hi = (uint64_t)(r >> 64);
  return LEX_OK;
}

// ---- float / double ------------------------------------------------------------------------------------------------------------
struct LexFloatFormat { int mant_bits, min_exp, inf_power, q_min, q_max, even_min, even_max, fast_q; uint64_t fast_mant; };
// mantissa bits stored, minimum exponent, the all-ones exponent, decimal exponents below / above which the value is 0 / inf, the
// exponents between which a product can be an exact half-way case, Clinger's exponent and mantissa limits
LEX_HD LexFloatFormat lex_format(bool single) {
  return single ? LexFloatFormat{23, -127, 0xFF, -65, 38, -17, 10, 10, 1ull << 24}
                : LexFloatFormat{52, -1023, 0x7FF, -342, 308, -4, 23, 22, 1ull << 53};
}

// w * 10^q (w != 0) -> the IEEE bits without the sign, or declined.  Eisel-Lemire as in the paper's appendix B.
// (The bits never have the sign bit set, so all ones says "declined": the answer travels in registers.)
constexpr uint64_t kLexDeclined = ~0ull;
template <bool single> LEX_HD uint64_t lex_eisel_lemire(uint64_t w, int32_t q) {
  const LexFloatFormat f = lex_format(single);
  if (q < f.q_min) return 0;
  if (q > f.q_max) return (uint64_t)f.inf_power << f.mant_bits;
  const int lz = __builtin_clzll(w);
  w <<= lz;
  // the 128 most significant bits of w * 5^q: one 64 x 64 product, a second one when the first cannot settle the bits that are kept
  const uint64_t* five = kLexPow5[q - kLexPow5Min];
  const uint64_t mask = ~0ull >> (f.mant_bits + 3);
  lex_u128 first = (lex_u128)w * five[0];
  uint64_t hi = (uint64_t)(first >> 64), lo = (uint64_t)first;
  if ((hi & mask) == mask) {
    const uint64_t second_hi = (uint64_t)(((lex_u128)w * five[1]) >> 64);
    lo += second_hi;
    if (second_hi > lo) hi++;
  }
  if (lo == ~0ull && !(q >= -27 && q <= 55)) return kLexDeclined;   // the truncated table cannot tell which side of a boundary this is
  const int upper = (int)(hi >> 63);
  const int shift = upper + 64 - f.mant_bits - 3;
  uint64_t m = hi >> shift;
  int p2 = (int)(((q * (152170 + 65536)) >> 16) + 63) + upper - lz - f.min_exp;   // floor(log2(10^q)) + the product's own exponent
  if (p2 <= 0) {                                   // subnormal: shift down, round to nearest (a half-way case cannot arise here)
    if (-p2 + 1 >= 64) return 0;
    m >>= -p2 + 1;
    m += m & 1;
    m >>= 1;
    return m;                                      // (a carry into 2^mant_bits is the smallest normal: the bits say so by themselves)
  }
  // exactly half-way between two values: round to even instead of up
  if (lo <= 1 && q >= f.even_min && q <= f.even_max && (m & 3) == 1 && (m << shift) == hi) m &= ~1ull;
  m += m & 1;
  m >>= 1;
  if (m >= (2ull << f.mant_bits)) { m = 1ull << f.mant_bits; p2++; }
  m &= ~(1ull << f.mant_bits);
  if (p2 >= f.inf_power) return (uint64_t)f.inf_power << f.mant_bits;
  return ((uint64_t)p2 << f.mant_bits) | m;
}

// the powers of ten that are exact in f64 (in f32 up to 10^10)
static LEX_TABLE_QUAL double kLexPow10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
LEX_HD double lex_f64_div(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ddiv_rn(a, b);
#else
  return a / b;
#endif
}
LEX_HD double lex_f64_mul(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dmul_rn(a, b);
#else
  return a * b;
#endif
}
LEX_HD uint64_t lex_f64_bits(double d) { union { double d; uint64_t u; } x; x.d = d; return x.u; }
LEX_HD uint32_t lex_f32_bits(float d) { union { float d; uint32_t u; } x; x.d = d; return x.u; }

// Lengths are 32-bit and below kLexMaxLen: the decimal exponent — the digits' positions plus the written exponent, which saturates at
// kLexExpCap, beyond every position — then fits 32 bits.  (The caller refuses a longer literal.)
constexpr uint32_t kLexMaxLen = 1u << 28;
constexpr int32_t kLexExpCap = 1 << 29;
// f32::from_str / f64::from_str on bytes: the bits of the target (f32 in the low 32 bits), sign included.
//   sign? ( "inf" | "infinity" | "nan" in any letter case  |  (Digit+ | Digit+ '.' Digit* | Digit* '.' Digit+) (('e'|'E') sign? Digit+)? )
// A signed NaN is declined.
// The words: sign? ("inf" | "infinity" | "nan") in any letter case.  LEX_NOT_SPECIAL: the literal does not start like one — a number or nothing.
// (A part of its own: on the device it runs in the calling kernel, and the out-of-line number parser does without its registers.)
constexpr int LEX_NOT_SPECIAL = 4;
template <bool single, class At> LEX_HD int lex_parse_float_special(At at, uint32_t n, uint64_t& out) {
  const int sign_shift = single ? 31 : 63, mant_bits = single ? 23 : 52;
  const uint64_t inf_bits = (single ? 0xFFull : 0x7FFull) << mant_bits;
  uint32_t i = 0; bool neg = false, sign = false;
  if (n) { const uint8_t c = at(0); if (c == '+' || c == '-') { neg = c == '-'; sign = true; i = 1; } }
  if (i >= n) return LEX_ERROR;
  const uint8_t first = at(i) | 0x20;   // (ASCII letters in lower case)
  if (first != 'i' && first != 'n') return LEX_NOT_SPECIAL;
  const uint32_t left = n - i;
  if (left != 3 && left != 8) return LEX_ERROR;   // (the length itself: a NUL byte is a character like any other)
  const uint64_t word = first == 'n' ? 0x6E616Eull : 0x7974696E69666E69ull;   // "nan" / "infinity" ("inf" is its start), first byte lowest
  if (first == 'n' && left != 3) return LEX_ERROR;
  LEX_NOUNROLL for (uint32_t k = 0; k < left; k++) {
    const uint8_t c = at(i + k);
    if ((uint8_t)(c >= 'A' && c <= 'Z' ? c + 32 : c) != (uint8_t)(word >> (8 * k))) return LEX_ERROR;
  }
  if (first == 'i') { out = inf_bits | ((uint64_t)neg << sign_shift); return LEX_OK; }
  if (sign) return LEX_DECLINED;          // a signed NaN: by decision not answered (see rdfgpu.h)
  out = inf_bits | (1ull << (mant_bits - 1));   // the quiet NaN of f32::NAN / f64::NAN
  return LEX_OK;
}
// The numbers: sign? (Digit+ | Digit+ '.' Digit* | Digit* '.' Digit+) (('e'|'E') sign? Digit+)?
template <bool single, class At> LEX_HD int lex_parse_float_number(At at, uint32_t n, uint64_t& out) {
  const int sign_shift = single ? 31 : 63;
  uint32_t i = 0; bool neg = false;
  if (n) { const uint8_t c = at(0); if (c == '+' || c == '-') { neg = c == '-'; i = 1; } }
  if (i >= n) return LEX_ERROR;
  // one pass, one byte read per step.  state: 0 integer digits, 1 fraction digits, 2 behind 'e', 3 behind the exponent's sign or in its digits
  uint64_t w = 0; int state = 0; int32_t q = 0, ex = 0; bool any = false, eany = false, eneg = false, dropped = false;
  LEX_NOUNROLL for (; i < n; i++) {
    const uint8_t c = at(i);
    const bool digit = c >= '0' && c <= '9';
    if (state <= 1) {
      if (digit) {                                  // the first 19 significant digits are kept
        any = true;
        if (w == 0 && c == '0') q -= state;
        else if (w < 1000000000000000000ull) { w = w * 10u + (uint64_t)(c - '0'); q -= state; }   // (below 10^18: fewer than 19 digits so far)
        else { dropped = dropped || c != '0'; q += 1 - state; }   // (cut zeros leave the value exactly w)
      } else if (c == '.' && state == 0) state = 1;
      else if ((c == 'e' || c == 'E') && any) state = 2;
      else return LEX_ERROR;
    } else if (digit) {
      eany = true; state = 3;
      ex = ex < kLexExpCap / 10 ? ex * 10 + (c - '0') : kLexExpCap;   // saturates (before the multiply) far beyond any representable exponent; the digits are still checked
    } else if ((c == '+' || c == '-') && state == 2) { eneg = c == '-'; state = 3; }
    else return LEX_ERROR;
  }
  if (!any || (state >= 2 && !eany)) return LEX_ERROR;
  q += eneg ? -ex : ex;
  const uint64_t sign_bit = (uint64_t)neg << sign_shift;
  if (w == 0) { out = sign_bit; return LEX_OK; }          // (every digit a zero: nothing was dropped)
  const int32_t fast_q = single ? 10 : 22;
  if (!dropped && w <= (single ? 1ull << 24 : 1ull << 53) && q >= -fast_q && q <= fast_q) {   // Clinger: both operands exact, one correctly rounded operation
    const double p10 = kLexPow10[q < 0 ? -q : q];
    if (single) {
      const float mf = (float)w, pf = (float)p10;
#if defined(__HIP_DEVICE_COMPILE__)
      const float r = q < 0 ? __fdiv_rn(mf, pf) : __fmul_rn(mf, pf);
#else
      const float r = q < 0 ? mf / pf : mf * pf;
#endif
      out = (uint64_t)lex_f32_bits(r) | sign_bit;
    } else {
      const double md = (double)w;
      out = lex_f64_bits(q < 0 ? lex_f64_div(md, p10) : lex_f64_mul(md, p10)) | sign_bit;
    }
    return LEX_OK;
  }
  // with non-zero dropped digits the true mantissa lies in (w, w + 1): both ends must round alike.  (A loop, so that the conversion exists once.)
  uint64_t bits = 0;
  LEX_NOUNROLL for (int pass = 0; pass < (dropped ? 2 : 1); pass++) {
    const uint64_t b = lex_eisel_lemire<single>(w + (uint64_t)pass, q);
    if (b == kLexDeclined || (pass && b != bits)) return LEX_DECLINED;
    bits = b;
  }
  out = bits | sign_bit;
  return LEX_OK;
}

template <bool single, class At> LEX_HD int lex_parse_float_as(At at, uint32_t n, uint64_t& out) {
  const int st = lex_parse_float_special<single>(at, n, out);
  return st == LEX_NOT_SPECIAL ? lex_parse_float_number<single>(at, n, out) : st;
}
template <class At> LEX_HD int lex_parse_float(At at, uint32_t n, bool single, uint64_t& out) {
  return single ? lex_parse_float_as<true>(at, n, out) : lex_parse_float_as<false>(at, n, out);
}

}  // namespace rdfgpu
