// date_parts.hpp — YEAR / MONTH / DAY / HOURS / MINUTES / SECONDS of an xsd:dateTime, per row (RDFGPU_EX_YEAR .. RDFGPU_EX_SECONDS).
//
// Restates Timestamp::{year_month_day, hour, minute, second} (lib/model/src/xsd/date_time.rs:1731-1839) statement by statement over a
// Timestamp as the device holds it: `value` = seconds on the XSD time line * 10^18 in an i128 (already shifted to UTC when a timezone is
// present) and the timezone offset in minutes (0 when there is none: `timezone_offset.unwrap_or(TimezoneOffset::UTC)`).
//   t       = value / 10^18 truncated toward zero (Decimal::as_i128, decimal.rs:277-279), then + offset * 60
//   days    = t.div_euclid(86400) + 366, then the 400 / 100 / 4 / 1-year descent and the month loop as written there, the shift that
//             makes a negative day count positive included (days_in_month: date_time.rs:2004-2020)
//   hour    = t.rem_euclid(86400) / 3600;  minute = t.rem_euclid(3600) / 60 (3600 divides 86400: one division serves both)
//   second  = value.rem_euclid(60 * 10^18) on the scaled i128 (its checked_abs changes nothing: the remainder is never negative); no
//             offset is applied, offsets are whole minutes
// |t| stays below 2^68 and the day count below 2^52, so everything after the first division is 64-bit arithmetic.  There is no 128-bit
// division on the device: the i128 is divided limb by limb by divisors below 2^32 (10^9 twice for 10^18; 86400; 60).
//
// Plain C++: with HIP, DP_HD is __host__ __device__; without, the same text runs in a stand-alone host program
// (tests/host/date_parts_checks.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DP_HD __host__ __device__ __forceinline__
#else
#define DP_HD inline
#endif

namespace rdfgpu {

typedef __int128 dp_i128;
typedef unsigned __int128 dp_u128;

enum { DP_YEAR = 0, DP_MONTH = 1, DP_DAY = 2, DP_HOURS = 3, DP_MINUTES = 4 };

// v /= d, returns v % d; d < 2^32
DP_HD uint32_t dp_divmod_small(dp_u128& v, uint32_t d) {
  uint32_t limb[4] = {(uint32_t)(v >> 96), (uint32_t)(v >> 64), (uint32_t)(v >> 32), (uint32_t)v};
  uint64_t rem = 0;
  for (int i = 0; i < 4; i++) { const uint64_t cur = (rem << 32) | limb[i]; limb[i] = (uint32_t)(cur / d); rem = cur % d; }
  v = ((dp_u128)limb[0] << 96) | ((dp_u128)limb[1] << 64) | ((dp_u128)limb[2] << 32) | (dp_u128)limb[3];
  return (uint32_t)rem;
}
DP_HD dp_i128 dp_value(int64_t lo, int64_t hi) { return (dp_i128)(((dp_u128)(uint64_t)hi << 64) | (dp_u128)(uint64_t)lo); }
DP_HD dp_u128 dp_mag(dp_i128 v) { return v < 0 ? (dp_u128)0 - (dp_u128)v : (dp_u128)v; }

// days_in_month(Some(y), m), date_time.rs:2004-2020 (Rust's `%` takes the dividend's sign, as C++'s does)
DP_HD int dp_days_in_month(long long y, int m) {
  if (m == 2) return (y % 4 != 0 || (y % 100 == 0 && y % 400 != 0)) ? 28 : 29;
  return (m == 4 || m == 6 || m == 9 || m == 11) ? 30 : 31;
}

// One of year / month / day / hour / minute (`part` = DP_*) of the timestamp (lo, hi) with `tz_minutes` of offset.
DP_HD long long date_part(int64_t lo, int64_t hi, int tz_minutes, int part) {
  const dp_i128 value = dp_value(lo, hi);
  dp_u128 m = dp_mag(value);
  dp_divmod_small(m, 1000000000u); dp_divmod_small(m, 1000000000u);          // as_i128: value / 10^18 toward zero (|.| < 2^68)
  const dp_i128 t = (value < 0 ? -(dp_i128)m : (dp_i128)m) + (dp_i128)((long long)tz_minutes * 60);
  dp_u128 q = dp_mag(t);
  uint32_t rem = dp_divmod_small(q, 86400u);
  long long days = (long long)(uint64_t)q;                                    // div_euclid / rem_euclid from the truncating pair
  if (t < 0) { days = -days; if (rem != 0) { days -= 1; rem = 86400u - rem; } }
  if (part == DP_HOURS) return (long long)(rem / 3600u);
  if (part == DP_MINUTES) return (long long)((rem % 3600u) / 60u);
  days += 366;
  long long shift = 0;
  if (days < 0) {                                                             // "Make days positive"
    shift = days / 146097 - 1;
    days -= shift * 146097;
    shift *= 400;
  }
  const long long year_mul_400 = days / 146097;
  days -= year_mul_400 * 146097;
  days -= 1;
  const long long year_mul_100 = days / 36524;
  days -= year_mul_100 * 36524;
  days += 1;
  const long long year_mul_4 = days / 1461;
  days -= year_mul_4 * 1461;
  days -= 1;
  const long long year_mod_4 = days / 365;
  days -= year_mod_4 * 365;
  const long long year = 400 * year_mul_400 + 100 * year_mul_100 + 4 * year_mul_4 + year_mod_4 + shift;
  if (part == DP_YEAR) return year;
  const bool is_leap_year = (year_mul_100 == 0 || year_mul_4 != 0) && year_mod_4 == 0;
  days += is_leap_year ? 1 : 0;
  int month = 0;
  for (int month_i = 1; month_i <= 12; month_i++) {
    const long long dim = dp_days_in_month(year, month_i);
    if (dim > days) { month = month_i; break; }
    days -= dim;
  }
  if (part == DP_MONTH) return month;
  return (long long)(uint8_t)days + 1;                                        // `days as u8 + 1`
}

// second(): value.rem_euclid(60 * 10^18), the scaled decimal in (lo, hi)
DP_HD void date_seconds(int64_t lo, int64_t hi, int64_t& out_lo, int64_t& out_hi) {
  const dp_i128 value = dp_value(lo, hi);
  dp_u128 a = dp_mag(value);
  const uint64_t f0 = dp_divmod_small(a, 1000000000u), f1 = dp_divmod_small(a, 1000000000u);   // a = whole seconds, f = the fraction
  const uint64_t frac = f1 * 1000000000ull + f0;
  const uint32_t s = dp_divmod_small(a, 60u);
  const dp_u128 minute = (dp_u128)60u * (dp_u128)1000000000000000000ull;
  dp_u128 r = (dp_u128)s * (dp_u128)1000000000000000000ull + (dp_u128)frac;
  if (value < 0 && r != 0) r = minute - r;
  out_lo = (int64_t)(uint64_t)r; out_hi = (int64_t)(uint64_t)(r >> 64);
}

}  // namespace rdfgpu
