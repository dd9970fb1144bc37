// extend.hip — ProjectionExec with expressions (include/rdfgpu.h, RDFGPU_NODE_EXTEND; SPARQL Extend: BIND, `SELECT (expr AS ?x)`, the
// `DIV(xsd:float(monthCount@1), monthBeforeCount@2) as ratio` of ..Business Intelligence - Q3 (Execution Plan).snap).
//
// One pass, one lane per input row, kExtendBlock rows per workgroup: every computed column's program runs in the generic VM
// (eval_program, expr_device.hpp) over the row's columns; per column the lane leaves
//   the 24-byte rdfgpu_agg_value of the row (what a value load reads back: lo, (lo, hi) for a decimal, the tag), and
//   the 4-byte entry of the value column: row + 1, or 0 where the value is the error value (an unbound binding).
// A value of a kind the record cannot carry (its `aux` has no room: strings, IRIs, blank nodes, dateTime / date / time, durations) raises
// the plan's run-time flag kRtExtendKind and is written as the error value; the execute then fails.
//
// The store.  A wave's 64 records are 1536 contiguous bytes, but a lane's own record is 24 bytes at a 24-byte stride: written per lane it
// is three 8-byte stores (global_store_dwordx2 x 3), each wave instruction touching 64 x 8 bytes spread over 1536.  Instead the wave
// lays its records down in LDS (three ds_write_b64 per lane) and takes them back as 96 16-byte chunks in address order: lanes 0 .. 63 the
// first 1024 bytes, lanes 0 .. 31 the other 512 — two global_store_dwordx4, every one of them a run of full consecutive lines.  The last
// wave of the input stores its live bytes only (a multiple of 8: its last chunk may be a half).  No atomics on the data path, no
// dependence on the order in which workgroups run: the output is a function of the input.  (Measured afterwards, DESIGN §6: over 2^24 rows
// both forms take the same time — the VM bounds the pass, not its stores — so the per-lane form would do as well.)
#include "join_device.hpp"

namespace rdfgpu {

static_assert(sizeof(rdfgpu_agg_value) == 24, "a record is three 8-byte words");
constexpr u32 kRecordWords = 3;                                  // 8-byte words of a record
constexpr u32 kWaveWords = 64 * kRecordWords;                    // .. of a wave's 64 records

// Column `c` of the input, for a program: a chain of value selects over the kernarg pointers stays in SGPRs (aggregate.hip, agg_col).
__device__ __forceinline__ const u32* extend_col(const ExtendArgs& a, u32 c) {
  const u32* p = a.col[0];
#pragma unroll
  for (u32 q = 1; q < (u32)kMaxCols; q++) p = c == q ? a.col[q] : p;
  return p;
}

template <bool LEX>
__device__ __forceinline__ void extend_rows(const ExtendArgs& a) {
  __shared__ __attribute__((aligned(16))) unsigned long long rec[(kExtendBlock / 64) * kWaveWords];   // 1536 B per wave
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u64 n = live_rows(a.n_dev, a.cap);
  const u64 base = (u64)blockIdx.x * kExtendBlock;
  if (base >= n) return;                                         // (uniform over the workgroup)
  const u64 row = base + tid;
  const bool valid = row < n;
  const u64 wave_row = base + (u64)wave * 64;                    // first row of this wave
  const u64 wave_live = wave_row < n ? (n - wave_row < 64 ? n - wave_row : 64) : 0;   // its live rows
  unsigned long long* const mine = rec + wave * kWaveWords;
  for (u32 q = 0; q < a.n_exprs; q++) {
    Val v = eval_program<LEX>(*a.prog[q], a.tt, [&](u32 c) { return valid ? extend_col(a, c)[row] : 0u; });
    const u8 t = v.tag;
    const bool carried = t == RDFGPU_TV_INT || t == RDFGPU_TV_INTEGER || t == RDFGPU_TV_DECIMAL || t == RDFGPU_TV_FLOAT ||
                         t == RDFGPU_TV_DOUBLE || t == RDFGPU_TV_BOOLEAN;
    if (valid && !carried && t != RDFGPU_TV_NULL && a.tt.rt_error) atomicOr(a.tt.rt_error, kRtExtendKind);   // (rare: the execute fails)
    const bool bound = valid && carried;
    mine[lane * kRecordWords + 0] = bound ? (unsigned long long)v.lo : 0ull;
    mine[lane * kRecordWords + 1] = bound && t == RDFGPU_TV_DECIMAL ? (unsigned long long)v.hi : 0ull;
    mine[lane * kRecordWords + 2] = bound ? (unsigned long long)t : 0ull;    // (tag, reserved bytes = 0)
    if (valid) a.out_val[q][row] = bound ? (u32)row + 1u : 0u;
    __syncthreads();
    // the wave's records leave in address order, 16 bytes per lane and instruction
    unsigned long long* const out = reinterpret_cast<unsigned long long*>(a.out[q] + wave_row);
    const u32 live_words = (u32)wave_live * kRecordWords;
#pragma unroll
    for (u32 w = 2 * lane; w < kWaveWords; w += 128) {
      if (w + 1 < live_words) *reinterpret_cast<ulonglong2*>(out + w) = *reinterpret_cast<const ulonglong2*>(mine + w);
      else if (w < live_words) out[w] = mine[w];
    }
    __syncthreads();                                             // the next column's records reuse `rec`
  }
}
__global__ __launch_bounds__(kExtendBlock) void extend_kernel(const ExtendArgs a) { extend_rows<false>(a); }
__global__ __launch_bounds__(kExtendBlock) void extend_lex_kernel(const ExtendArgs a) { extend_rows<true>(a); }   // the extended cases (kOpExtended, expr_ops.hpp) compiled into the VM

void launch_extend(const ExtendArgs& a, bool lex, hipStream_t s) {
  const u64 g = (a.cap + kExtendBlock - 1) / kExtendBlock;       // (cap < 2^32 - 1: Plan::exec_extend)
  if (lex) hipLaunchKernelGGL(extend_lex_kernel, dim3((unsigned)(g ? g : 1)), dim3(kExtendBlock), 0, s, a);   // (a program holds an op with kOpExtended)
  else hipLaunchKernelGGL(extend_kernel, dim3((unsigned)(g ? g : 1)), dim3(kExtendBlock), 0, s, a);
  RDFGPU_HIP(hipGetLastError());
}

// (kernels.hpp, preload_code_objects: the runtime loads a translation unit's code object at the first use of one of its kernels)
void preload_tu_extend() { hipFuncAttributes at; RDFGPU_HIP(hipFuncGetAttributes(&at, reinterpret_cast<const void*>(extend_kernel))); }

}  // namespace rdfgpu
