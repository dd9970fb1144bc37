// date_parts_checks.cpp — csrc/date_parts.hpp (the arithmetic of RDFGPU_EX_YEAR .. RDFGPU_EX_SECONDS) compiled as plain C++, as a
// stand-alone host program:
//
//   make -C rdf-fusion_amd/csrc date-parts-checks [SANITIZE=1]
//
// date_parts_checks FILE: every line of FILE is a timestamp `lo hi tz_minutes` (the two signed 64-bit halves of the scaled i128 value and
// the offset in minutes, 0 when there is no timezone); the answer is one line `year month day hours minutes seconds_lo seconds_hi`.
// tests/test_dateparts_cpu.py compares the answers with its Python reference (tests/datepart_cases.py).
#include "../../rdf-fusion_amd/csrc/date_parts.hpp"

#include <cinttypes>
#include <cstdio>

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s FILE\n", argv[0]); return 2; }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) { std::perror(argv[1]); return 2; }
  long long lo, hi; int tz;
  unsigned long lines = 0;
  while (std::fscanf(f, "%lld %lld %d", &lo, &hi, &tz) == 3) {
    int64_t s_lo = 0, s_hi = 0;
    rdfgpu::date_seconds((int64_t)lo, (int64_t)hi, s_lo, s_hi);
    std::printf("%lld %lld %lld %lld %lld %" PRId64 " %" PRId64 "\n",
                rdfgpu::date_part(lo, hi, tz, rdfgpu::DP_YEAR), rdfgpu::date_part(lo, hi, tz, rdfgpu::DP_MONTH), rdfgpu::date_part(lo, hi, tz, rdfgpu::DP_DAY),
                rdfgpu::date_part(lo, hi, tz, rdfgpu::DP_HOURS), rdfgpu::date_part(lo, hi, tz, rdfgpu::DP_MINUTES), s_lo, s_hi);
    lines++;
  }
  std::fclose(f);
  std::fprintf(stderr, "%lu timestamps\n", lines);
  return 0;
}
