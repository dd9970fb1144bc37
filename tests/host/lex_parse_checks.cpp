// lex_parse_checks.cpp — the lexical parsers of RDFGPU_EX_CAST_LEX (rdf-fusion_amd/csrc/lex_parse.hpp) as a stand-alone host program: the
// header is plain C++ when it is compiled without HIP, so the text the device runs is checked here, under AddressSanitizer /
// UndefinedBehaviorSanitizer too:
//
//   make -C rdf-fusion_amd/csrc lex-parse-checks [SANITIZE=1]      (builds build/lex_parse_checks[_san])
//
//   lex_parse_checks cases FILE      every row of the case tables (tests/lex_cases.py writes the file) against the Python reference:
//                                    `target hex-bytes status bits-lo bits-hi may-decline`, status ok / error / any (a signed NaN)
//   lex_parse_checks fuzz N SEED     N generated grammar-valid strings (1-25 digits, exponents over the whole range, a share next to
//                                    f32 / f64 half-way points) against glibc's correctly rounded strtof / strtod: every row matches bit
//                                    for bit or is declined; over the strings of at most 19 digits the declined share must be 0 for
//                                    f32 and below 0.1 % for f64
#include "../../rdf-fusion_amd/csrc/lex_parse.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <sstream>
#include <string>

using namespace rdfgpu;

namespace {
struct Bytes {
  const unsigned char* p;
  uint8_t operator()(uint32_t i) const { return p[i]; }
};
// the bytes in an exactly sized heap block: a read past either end is AddressSanitizer's to report
struct Exact {
  unsigned char* p; uint32_t n;
  explicit Exact(const std::string& s) : p((unsigned char*)std::malloc(s.size() ? s.size() : 1)), n((uint32_t)s.size()) { std::memcpy(p, s.data(), s.size()); }
  ~Exact() { std::free(p); }
};

int run_cases(const char* path) {
  std::ifstream in(path);
  if (!in) { std::printf("cannot read %s\n", path); return 2; }
  std::string line; int rows = 0, failures = 0, declined = 0;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string target, hex, status; unsigned long long lo = 0, hi = 0; int may = 0;
    if (!(ls >> target >> hex >> status >> lo >> hi >> may)) continue;
    std::string s;
    for (size_t i = 1; i + 1 < hex.size(); i += 2) s.push_back((char)std::stoi(hex.substr(i, 2), nullptr, 16));   // ("x" + hex digits: never empty)
    Exact e(s); Bytes at{e.p};
    int st = LEX_ERROR; uint64_t glo = 0, ghi = 0;
    if (target == "boolean") { bool b = false; st = lex_parse_boolean(at, e.n, b); glo = b; }
    else if (target == "int") { long long v = 0; st = lex_parse_i64(at, e.n, INT32_MIN, INT32_MAX, v); glo = (uint64_t)v; }
    else if (target == "integer") { long long v = 0; st = lex_parse_i64(at, e.n, INT64_MIN, INT64_MAX, v); glo = (uint64_t)v; }
    else if (target == "decimal") st = lex_parse_decimal(at, e.n, glo, ghi);
    else st = lex_parse_float(at, e.n, target == "float", glo);
    bool ok;
    if (st == LEX_DECLINED) { ok = may == 1; declined++; }
    else if (status == "any") ok = false;                        // a signed NaN must be declined
    else if (status == "error") ok = st == LEX_ERROR;
    else ok = st == LEX_OK && glo == lo && ghi == hi;
    rows++;
    if (!ok) { failures++; std::printf("FAIL %s \"%s\": status %d bits %llx %llx, want %s %llx %llx (may decline %d)\n", target.c_str(), s.c_str(), st, (unsigned long long)glo, (unsigned long long)ghi, status.c_str(), lo, hi, may); }
  }
  std::printf("cases: %d rows, %d declined, %d failure(s)\n", rows, declined, failures);
  return failures || rows == 0 ? 1 : 0;
}

// a decimal string of `digits` significant digits around the value v (exact digits of v from printf, then cut; the cut may be bumped)
std::string near_value(long double v, int digits, std::mt19937_64& rng) {
  char buf[128];
  std::snprintf(buf, sizeof buf, "%.*Le", digits - 1, v);
  std::string s(buf);
  if (digits > 1 && rng() % 3 == 0) {          // nudge the last mantissa digit: just below / above
    const size_t e = s.find('e');
    char& c = s[e - 1];
    if (c >= '1' && c <= '8') c = (char)(c + (rng() % 2 ? 1 : -1));
  }
  return s;
}

std::string generate(std::mt19937_64& rng, int& digits) {
  const unsigned kind = (unsigned)(rng() % 10);
  digits = 1 + (int)(rng() % 25);
  if (kind < 2) {                              // next to an f32 half-way point: the mid-point of two neighbours is exact in f64
    uint32_t b = (uint32_t)rng() & 0x7F7FFFFFu; float f; std::memcpy(&f, &b, 4);
    const long double mid = ((long double)f + (long double)std::nextafterf(f, INFINITY)) / 2;
    if (std::isfinite((double)mid)) return near_value(mid, digits, rng);
  }
  if (kind < 4) {                              // next to an f64 half-way point: exact in the 64-bit mantissa of long double
    uint64_t b = rng() & 0x7FEFFFFFFFFFFFFFull; double d; std::memcpy(&d, &b, 8);
    const long double mid = ((long double)d + (long double)std::nextafter(d, (double)INFINITY)) / 2;
    return near_value(mid, digits, rng);
  }
  std::string s;
  if (rng() % 4 == 0) s.push_back(rng() % 2 ? '-' : '+');
  std::string m;
  for (int i = 0; i < digits; i++) m.push_back((char)('0' + (i == 0 ? 1 + rng() % 9 : rng() % 10)));
  const unsigned form = (unsigned)(rng() % 4);
  const size_t dot = (size_t)(rng() % (m.size() + 1));
  if (form == 0) s += m;
  else if (form == 1) s += m + ".";
  else if (form == 2) s += "." + m;
  else s += m.substr(0, dot) + "." + m.substr(dot);
  const unsigned ek = (unsigned)(rng() % 8);
  if (ek) {
    int e;
    if (ek < 4) e = (int)(rng() % 61) - 30;                    // the everyday range
    else if (ek < 7) e = (int)(rng() % 701) - 350;             // over every finite exponent, the subnormals and both overflows
    else e = (int)(rng() % 2001) - 1000;
    s += (rng() % 2 ? "e" : "E");
    if (e >= 0 && rng() % 2) s += "+";
    s += std::to_string(e);
  }
  return s;
}

int run_fuzz(long n, unsigned long long seed) {
  std::mt19937_64 rng(seed);
  long short_rows = 0, declined32 = 0, declined64 = 0, long_declined = 0, mismatches = 0, long_rows = 0;
  for (long r = 0; r < n; r++) {
    int digits = 0;
    const std::string s = generate(rng, digits);
    Exact e(s); Bytes at{e.p};
    const float f = std::strtof(s.c_str(), nullptr); const double d = std::strtod(s.c_str(), nullptr);
    uint32_t fb; uint64_t db; std::memcpy(&fb, &f, 4); std::memcpy(&db, &d, 8);
    uint64_t g32 = 0, g64 = 0;
    const int s32 = lex_parse_float(at, e.n, true, g32), s64 = lex_parse_float(at, e.n, false, g64);
    const bool is_short = digits <= 19;
    (is_short ? short_rows : long_rows)++;
    if (s32 == LEX_DECLINED) (is_short ? declined32 : long_declined)++;
    else if (s32 != LEX_OK || g32 != fb) { mismatches++; std::printf("MISMATCH f32 \"%s\": status %d %llx, strtof %x\n", s.c_str(), s32, (unsigned long long)g32, fb); }
    if (s64 == LEX_DECLINED) (is_short ? declined64 : long_declined)++;
    else if (s64 != LEX_OK || g64 != db) { mismatches++; std::printf("MISMATCH f64 \"%s\": status %d %llx, strtod %llx\n", s.c_str(), s64, (unsigned long long)g64, (unsigned long long)db); }
  }
  const double share64 = short_rows ? 100.0 * (double)declined64 / (double)short_rows : 0.0;
  std::printf("fuzz: %ld strings (%ld of at most 19 digits), mismatches %ld, declined: f32 %ld, f64 %ld (%.5f %%) of the short ones, %ld conversions of the long ones\n",
              n, short_rows, mismatches, declined32, declined64, share64, long_declined);
  return mismatches == 0 && declined32 == 0 && share64 < 0.1 && short_rows > n / 2 ? 0 : 1;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "cases")) return run_cases(argv[2]);
  if (argc == 4 && !std::strcmp(argv[1], "fuzz")) return run_fuzz(std::atol(argv[2]), std::strtoull(argv[3], nullptr, 10));
  std::printf("usage: lex_parse_checks cases FILE | fuzz N SEED\n");
  return 2;
}
