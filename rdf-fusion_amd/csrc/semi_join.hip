// semi_join.hip — HashJoinExec / NestedLoopJoinExec with JoinType::LeftSemi and JoinType::LeftAnti: FILTER EXISTS, FILTER NOT
// EXISTS (correlated subqueries, lib/logical/src/expr_builder_context.rs:197-300, decorrelated by DataFusion into semi / anti joins)
// and MINUS (lib/logical/src/minus/rewrite.rs:58-130, a LeftAnti join).
//
// A left row needs one bit: does ANY right row equal it on every key and pass the join filter with exactly `true`?  So nothing is
// queued and nothing per match is reserved, unlike lds_join_kernel: a lane takes one left row at a time, walks the table with an
// early exit at the first passing candidate and settles the row's bit; the survivors of a tile are compacted with ballot + mbcnt
// and leave through ONE output reservation per workgroup and tile (same-address atomics retire at ~88 per microsecond, so per wave
// would cost a 32 M-row probe side 6 ms), their projected left columns stored at consecutive positions.
//
// Tables (the right input is always the table, the left rows are always the probe):
//   kSemiLds     every workgroup builds a {key0, row + 1} open-addressing set of the right rows in its LDS, then probes it
//   kSemiHbm     the same set once in HBM (semi_build_kernel), probed by every workgroup
//   kSemiNested  no keys (NestedLoopJoinExec): the right rows are staged through LDS in tiles of kNljTile rows; a lane stops at its
//                first passing right row and the workgroup stops once every lane of it is decided
// Without a join filter one entry per distinct right key is enough (existence only): equal keys are not inserted twice, which keeps
// a right side of many equal keys from turning the linear-probing build quadratic.  With a filter every right row is an entry.
#include "join_device.hpp"

namespace rdfgpu {

constexpr int kSemiBlock = 256;
constexpr int kSemiItems = 4;                       // left rows per lane and tile: one reservation per 1024 rows
constexpr u32 kSemiTile = (u32)kSemiBlock * kSemiItems;
constexpr u32 kNljTile = 256;                       // right rows staged per step of the nested-loop form

__device__ __forceinline__ unsigned long long semi_entry(u32 key0, u64 row) { return (unsigned long long)key0 | ((unsigned long long)(row + 1) << 32); }

// Whether right row r carries key tuple `k` (key 0 already compared through the slot).
template <bool ONE>
__device__ __forceinline__ bool right_keys_equal(const SemiJoinArgs& a, const Keys& k, u64 r) {
  if constexpr (ONE) return true;
  bool eq = true;
#pragma unroll
  for (u32 q = 1; q < RDFGPU_MAX_KEYS; q++) if (q < a.n_keys) eq = eq && a.right_key[q][r] == k.k[q];
  return eq;
}

// Inserts right row r (non-null keys `k`) into the set `tbl`; DEDUPE: not when an entry with the same key tuple is there already.
template <bool ONE, bool DEDUPE>
__device__ __forceinline__ void semi_insert(const SemiJoinArgs& a, unsigned long long* tbl, const Keys& k, u64 r) {
  const unsigned long long e = semi_entry(k.k[0], r);
  u32 h = hash_keys4(k, ONE ? 1u : a.n_keys) & a.tbl_mask;
  for (;;) {   // load factor <= 0.5: an empty slot exists
    const unsigned long long prev = atomicCAS(tbl + h, 0ull, e);
    if (prev == 0ull) return;
    if (DEDUPE && (u32)prev == k.k[0] && right_keys_equal<ONE>(a, k, (prev >> 32) - 1)) return;
    h = (h + 1) & a.tbl_mask;
  }
}

// The join filter on (left row j, right row r) is exactly true.  RIGHT(c) gives right column c (0-based) of row r.
template <int FK, class Right>
__device__ __forceinline__ bool semi_filter(const SemiJoinArgs& a, u64 j, Right right) {
  if constexpr (FK == kSemiNoFilter) return true;
  else if constexpr (FK == kSemiIdPair) {
    const u32 va = a.idp.a < a.n_left_cols ? a.cols[a.idp.a][j] : right(a.idp.a - a.n_left_cols);
    const u32 vb = a.idp.b < a.n_left_cols ? a.cols[a.idp.b][j] : right(a.idp.b - a.n_left_cols);
    if (va == 0 || vb == 0) return false;   // null: not a match
    return (va == vb) == (a.idp.is_eq != 0);
  } else {
    const Val v = eval_program<FK == kSemiVmLex>(*a.prog, a.tt, [&](u32 c) { return c < a.n_left_cols ? a.cols[c][j] : right(c - a.n_left_cols); });
    return v.lo == 1;
  }
}

// Whether left row j has a partner in the set `tbl`.
template <bool ONE, int FK>
__device__ __forceinline__ bool semi_probe(const SemiJoinArgs& a, const unsigned long long* tbl, u64 j) {
  Keys k;
  if (!load_keys(a.left_key, ONE ? 1u : a.n_keys, j, k)) return false;   // NullEqualsNothing
  u32 h = hash_keys4(k, ONE ? 1u : a.n_keys) & a.tbl_mask;
  for (;;) {
    const unsigned long long e = tbl[h];
    if (e == 0ull) return false;
    if ((u32)e == k.k[0]) {
      const u64 r = (e >> 32) - 1;
      if (right_keys_equal<ONE>(a, k, r) &&
          semi_filter<FK>(a, j, [&](u32 c) { return a.cols[a.n_left_cols + c][r]; })) return true;
    }
    h = (h + 1) & a.tbl_mask;
  }
}

// Compacts the kept rows of one tile of the workgroup and stores their projected left columns: one reservation per tile.
template <int IT>
__device__ __forceinline__ void semi_emit(const SemiJoinArgs& a, const u64 (&row)[IT], const bool (&keep)[IT], u32* wave_tot, u64* wg_base) {
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long mask[IT]; u32 off[IT]; u32 wtot = 0;
#pragma unroll
  for (int k = 0; k < IT; k++) { mask[k] = __ballot(keep[k]); off[k] = wtot; wtot += (u32)__popcll(mask[k]); }
  if (lane == 0) wave_tot[wave] = wtot;
  __syncthreads();
  if (tid == 0) {
    u32 total = 0;
    for (int w = 0; w < kSemiBlock / 64; w++) { const u32 t = wave_tot[w]; wave_tot[w] = total; total += t; }
    *wg_base = total ? atomicAdd((unsigned long long*)a.n_out_dev, (unsigned long long)total) : 0ull;
  }
  __syncthreads();
  const u64 base = *wg_base + wave_tot[wave];
#pragma unroll
  for (int k = 0; k < IT; k++) {
    if (!keep[k]) continue;
    const u64 pos = base + off[k] + lane_prefix(mask[k]);
    for (u32 c = 0; c < a.n_out_cols; c++) a.out[c][pos] = a.cols[a.proj[c]][row[k]];
  }
  __syncthreads();   // wave_tot / wg_base are reused by the next tile
}

// HBM set: one entry per right row (per distinct key tuple when DEDUPE).
template <bool ONE, bool DEDUPE>
__global__ __launch_bounds__(kSemiBlock) void semi_build_kernel(const SemiJoinArgs a) {
  const u64 nr = live_rows(a.n_right_dev, a.n_right_cap);
  for (u64 r = (u64)blockIdx.x * kSemiBlock + threadIdx.x; r < nr; r += (u64)gridDim.x * kSemiBlock) {
    Keys k;
    if (load_keys(a.right_key, ONE ? 1u : a.n_keys, r, k)) semi_insert<ONE, DEDUPE>(a, a.gslots, k, r);
  }
}

// Hash forms.  FORM = kSemiLds: the set lives in dynamic LDS, built by every workgroup; kSemiHbm: a.gslots.
template <int FORM, bool ANTI, int FK, bool ONE>
__global__ __launch_bounds__(kSemiBlock) void semi_join_kernel(const SemiJoinArgs a) {
  extern __shared__ unsigned long long lds_tbl[];
  __shared__ u32 wave_tot[kSemiBlock / 64];
  __shared__ u64 wg_base;
  const u32 tid = threadIdx.x;
  const u64 nl = live_rows(a.n_left_dev, a.n_left_cap);
  const unsigned long long* tbl = a.gslots;
  if constexpr (FORM == kSemiLds) {
    const u64 nr = live_rows(a.n_right_dev, a.n_right_cap);
    for (u32 s = tid; s <= a.tbl_mask; s += kSemiBlock) lds_tbl[s] = 0ull;
    __syncthreads();
    for (u64 r = tid; r < nr; r += kSemiBlock) {
      Keys k;
      if (load_keys(a.right_key, ONE ? 1u : a.n_keys, r, k)) semi_insert<ONE, FK == kSemiNoFilter>(a, lds_tbl, k, r);
    }
    __syncthreads();
    tbl = lds_tbl;
  }
  const u64 n_tiles = (nl + kSemiTile - 1) / kSemiTile;
  for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    u64 row[kSemiItems]; bool keep[kSemiItems];
#pragma unroll
    for (int k = 0; k < kSemiItems; k++) {
      row[k] = tile * kSemiTile + (u64)k * kSemiBlock + tid;
      keep[k] = row[k] < nl && (semi_probe<ONE, FK>(a, tbl, row[k]) != ANTI);
    }
    semi_emit<kSemiItems>(a, row, keep, wave_tot, &wg_base);
  }
}

// NestedLoopJoinExec.  Without a filter the verdict is the same for every row: does the right input have a row?
template <bool ANTI, int FK>
__global__ __launch_bounds__(kSemiBlock) void semi_nested_kernel(const SemiJoinArgs a) {
  __shared__ u32 rt[kMaxCols * kNljTile];   // right rows r0 .. r0 + kNljTile, column-major
  __shared__ u32 wave_tot[kSemiBlock / 64];
  __shared__ u64 wg_base;
  const u32 tid = threadIdx.x;
  const u64 nl = live_rows(a.n_left_dev, a.n_left_cap), nr = live_rows(a.n_right_dev, a.n_right_cap);
  const u64 n_tiles = (nl + kSemiBlock - 1) / kSemiBlock;
  for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    u64 row[1] = {tile * kSemiBlock + tid};
    const bool valid = row[0] < nl;
    bool matched = false;
    if constexpr (FK == kSemiNoFilter) {
      matched = nr > 0;
    } else {
      bool decided = !valid;
      for (u64 r0 = 0; r0 < nr; r0 += kNljTile) {
        const u32 cnt = (u32)(nr - r0 < kNljTile ? nr - r0 : kNljTile);
        for (u32 i = tid; i < a.n_right_cols * kNljTile; i += kSemiBlock) {
          const u32 c = i / kNljTile, t = i % kNljTile;
          if (t < cnt) rt[i] = a.cols[a.n_left_cols + c][r0 + t];
        }
        __syncthreads();
        for (u32 t = 0; t < cnt; t++) {
          if (__ballot(!decided) == 0ull) break;   // every lane of the wave knows its answer
          if (!decided && semi_filter<FK>(a, row[0], [&](u32 c) { return rt[c * kNljTile + t]; })) decided = matched = true;
        }
        if (!__syncthreads_or(!decided)) break;   // (also the barrier before the tile is overwritten)
      }
    }
    bool keep[1] = {valid && (matched != ANTI)};
    semi_emit<1>(a, row, keep, wave_tot, &wg_base);
  }
}

// ---- JoinType::LeftMark (RDFGPU_JOIN_LEFT_MARK): EXISTS as an operand ----
// Every left row comes out once, at its own index, with one further column: the mark, 1 + "the row has a partner" (an index into the
// node's two-record value array: 1 = false, 2 = true).  Same tables, same probe, same filter as the semi join — but nothing is compacted
// and nothing reserved: a lane settles its row's bit and stores the row.  SemiJoinArgs::proj indexes [left cols, mark]: entry
// n_left_cols is the mark.
__device__ __forceinline__ void mark_store(const SemiJoinArgs& a, u64 j, bool bit) {
  for (u32 c = 0; c < a.n_out_cols; c++) a.out[c][j] = a.proj[c] == a.n_left_cols ? 1u + (u32)bit : a.cols[a.proj[c]][j];
}

// Hash forms (FORM as for semi_join_kernel).
template <int FORM, int FK, bool ONE>
__global__ __launch_bounds__(kSemiBlock) void mark_join_kernel(const SemiJoinArgs a) {
  extern __shared__ unsigned long long lds_tbl[];
  const u32 tid = threadIdx.x;
  const u64 nl = live_rows(a.n_left_dev, a.n_left_cap);
  const unsigned long long* tbl = a.gslots;
  if constexpr (FORM == kSemiLds) {
    const u64 nr = live_rows(a.n_right_dev, a.n_right_cap);
    for (u32 s = tid; s <= a.tbl_mask; s += kSemiBlock) lds_tbl[s] = 0ull;
    __syncthreads();
    for (u64 r = tid; r < nr; r += kSemiBlock) {
      Keys k;
      if (load_keys(a.right_key, ONE ? 1u : a.n_keys, r, k)) semi_insert<ONE, FK == kSemiNoFilter>(a, lds_tbl, k, r);
    }
    __syncthreads();
    tbl = lds_tbl;
  }
  for (u64 j = (u64)blockIdx.x * kSemiBlock + tid; j < nl; j += (u64)gridDim.x * kSemiBlock) mark_store(a, j, semi_probe<ONE, FK>(a, tbl, j));
}

// NestedLoopJoinExec.  Without a filter the mark is the same for every row: does the right input have a row?
template <int FK>
__global__ __launch_bounds__(kSemiBlock) void mark_nested_kernel(const SemiJoinArgs a) {
  __shared__ u32 rt[kMaxCols * kNljTile];   // right rows r0 .. r0 + kNljTile, column-major
  const u32 tid = threadIdx.x;
  const u64 nl = live_rows(a.n_left_dev, a.n_left_cap), nr = live_rows(a.n_right_dev, a.n_right_cap);
  const u64 n_tiles = (nl + kSemiBlock - 1) / kSemiBlock;
  for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const u64 row = tile * kSemiBlock + tid;
    const bool valid = row < nl;
    bool matched = false;
    if constexpr (FK == kSemiNoFilter) {
      matched = nr > 0;
    } else {
      bool decided = !valid;
      for (u64 r0 = 0; r0 < nr; r0 += kNljTile) {
        const u32 cnt = (u32)(nr - r0 < kNljTile ? nr - r0 : kNljTile);
        for (u32 i = tid; i < a.n_right_cols * kNljTile; i += kSemiBlock) {
          const u32 c = i / kNljTile, t = i % kNljTile;
          if (t < cnt) rt[i] = a.cols[a.n_left_cols + c][r0 + t];
        }
        __syncthreads();
        for (u32 t = 0; t < cnt; t++) {
          if (__ballot(!decided) == 0ull) break;   // every lane of the wave knows its answer
          if (!decided && semi_filter<FK>(a, row, [&](u32 c) { return rt[c * kNljTile + t]; })) decided = matched = true;
        }
        if (!__syncthreads_or(!decided)) break;   // (also the barrier before the tile is overwritten)
      }
    }
    if (valid) mark_store(a, row, matched);
  }
}

size_t semi_join_lds_bytes(const SemiJoinArgs& a, int form) {
  return form == kSemiLds ? (size_t)(a.tbl_mask + 1) * sizeof(unsigned long long) : 0;
}

void launch_semi_build(const SemiJoinArgs& a, bool dedupe, hipStream_t s) {
  u64 g = (a.n_right_cap + kSemiBlock - 1) / kSemiBlock;
  if (g > 8192) g = 8192;
  const dim3 grid((unsigned)(g ? g : 1));
  const bool one = a.n_keys == 1;
  if (one && dedupe) hipLaunchKernelGGL((semi_build_kernel<true, true>), grid, dim3(kSemiBlock), 0, s, a);
  else if (one) hipLaunchKernelGGL((semi_build_kernel<true, false>), grid, dim3(kSemiBlock), 0, s, a);
  else if (dedupe) hipLaunchKernelGGL((semi_build_kernel<false, true>), grid, dim3(kSemiBlock), 0, s, a);
  else hipLaunchKernelGGL((semi_build_kernel<false, false>), grid, dim3(kSemiBlock), 0, s, a);
  RDFGPU_HIP(hipGetLastError());
}

template <int FORM, bool ANTI, int FK, bool ONE>
static void launch_hash_form(const SemiJoinArgs& a, hipStream_t s) {
  const size_t lds = semi_join_lds_bytes(a, FORM);
  if constexpr (FORM == kSemiLds) {   // more than 64 KiB of dynamic LDS has to be allowed per kernel
    static std::once_flag attr_once;
    std::call_once(attr_once, [] {
      RDFGPU_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(semi_join_kernel<FORM, ANTI, FK, ONE>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)(2 * kSemiLdsMaxBuild * sizeof(unsigned long long) + 1024)));
    });
  }
  u64 g = (a.n_left_cap + kSemiTile - 1) / kSemiTile;
  // every workgroup of the LDS form builds the whole set: enough of them to fill the part, not one per tile
  const u64 max_g = FORM == kSemiLds ? 1024 : 16384;
  if (g > max_g) g = max_g;
  hipLaunchKernelGGL((semi_join_kernel<FORM, ANTI, FK, ONE>), dim3((unsigned)(g ? g : 1)), dim3(kSemiBlock), lds, s, a);
}

template <int FORM, bool ANTI, int FK>
static void launch_hash_fk(const SemiJoinArgs& a, hipStream_t s) {
  if (a.n_keys == 1) launch_hash_form<FORM, ANTI, FK, true>(a, s); else launch_hash_form<FORM, ANTI, FK, false>(a, s);
}

template <bool ANTI, int FK>
static void launch_form(const SemiJoinArgs& a, int form, hipStream_t s) {
  if (form == kSemiLds) launch_hash_fk<kSemiLds, ANTI, FK>(a, s);
  else if (form == kSemiHbm) launch_hash_fk<kSemiHbm, ANTI, FK>(a, s);
  else {
    u64 g = (a.n_left_cap + kSemiBlock - 1) / kSemiBlock;
    if (g > 16384) g = 16384;
    hipLaunchKernelGGL((semi_nested_kernel<ANTI, FK>), dim3((unsigned)(g ? g : 1)), dim3(kSemiBlock), 0, s, a);
  }
}

template <bool ANTI>
static void launch_anti(const SemiJoinArgs& a, int form, int filter, hipStream_t s) {
  if (filter == kSemiNoFilter) launch_form<ANTI, kSemiNoFilter>(a, form, s);
  else if (filter == kSemiIdPair) launch_form<ANTI, kSemiIdPair>(a, form, s);
  else if (filter == kSemiVmLex) launch_form<ANTI, kSemiVmLex>(a, form, s);
  else launch_form<ANTI, kSemiVm>(a, form, s);
}

void launch_semi_join(const SemiJoinArgs& a, int form, bool anti, int filter, hipStream_t s) {
  if (form < kSemiLds || form > kSemiNested) fail(RDFGPU_ERR_INVALID, "semi join: table form %d", form);
  if (form == kSemiLds && a.tbl_mask + 1 > 2 * kSemiLdsMaxBuild) fail(RDFGPU_ERR_INVALID, "semi join: LDS set of %u slots", a.tbl_mask + 1);
  if (anti) launch_anti<true>(a, form, filter, s); else launch_anti<false>(a, form, filter, s);
  RDFGPU_HIP(hipGetLastError());
}

template <int FORM, int FK, bool ONE>
static void launch_mark_hash_form(const SemiJoinArgs& a, hipStream_t s) {
  const size_t lds = semi_join_lds_bytes(a, FORM);
  if constexpr (FORM == kSemiLds) {   // more than 64 KiB of dynamic LDS has to be allowed per kernel
    static std::once_flag attr_once;
    std::call_once(attr_once, [] {
      RDFGPU_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mark_join_kernel<FORM, FK, ONE>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)(2 * kSemiLdsMaxBuild * sizeof(unsigned long long) + 1024)));
    });
  }
  u64 g = (a.n_left_cap + kSemiTile - 1) / kSemiTile;   // kSemiItems rows per lane, as in the semi join; the LDS form builds the set per workgroup
  const u64 max_g = FORM == kSemiLds ? 1024 : 16384;
  if (g > max_g) g = max_g;
  hipLaunchKernelGGL((mark_join_kernel<FORM, FK, ONE>), dim3((unsigned)(g ? g : 1)), dim3(kSemiBlock), lds, s, a);
}

template <int FK>
static void launch_mark_form(const SemiJoinArgs& a, int form, hipStream_t s) {
  const bool one = a.n_keys == 1;
  if (form == kSemiLds) { if (one) launch_mark_hash_form<kSemiLds, FK, true>(a, s); else launch_mark_hash_form<kSemiLds, FK, false>(a, s); }
  else if (form == kSemiHbm) { if (one) launch_mark_hash_form<kSemiHbm, FK, true>(a, s); else launch_mark_hash_form<kSemiHbm, FK, false>(a, s); }
  else {
    u64 g = (a.n_left_cap + kSemiBlock - 1) / kSemiBlock;
    if (g > 16384) g = 16384;
    hipLaunchKernelGGL((mark_nested_kernel<FK>), dim3((unsigned)(g ? g : 1)), dim3(kSemiBlock), 0, s, a);
  }
}

// The HBM set of a mark join is built by launch_semi_build, like a semi join's.
void launch_mark_join(const SemiJoinArgs& a, int form, int filter, hipStream_t s) {
  if (form < kSemiLds || form > kSemiNested) fail(RDFGPU_ERR_INVALID, "mark join: table form %d", form);
  if (form == kSemiLds && a.tbl_mask + 1 > 2 * kSemiLdsMaxBuild) fail(RDFGPU_ERR_INVALID, "mark join: LDS set of %u slots", a.tbl_mask + 1);
  for (u32 c = 0; c < a.n_out_cols; c++) if (a.proj[c] > a.n_left_cols) fail(RDFGPU_ERR_INVALID, "mark join: output column %u of [%u left columns, mark]", a.proj[c], a.n_left_cols);
  if (filter == kSemiNoFilter) launch_mark_form<kSemiNoFilter>(a, form, s);
  else if (filter == kSemiIdPair) launch_mark_form<kSemiIdPair>(a, form, s);
  else if (filter == kSemiVmLex) launch_mark_form<kSemiVmLex>(a, form, s);
  else launch_mark_form<kSemiVm>(a, form, s);
  RDFGPU_HIP(hipGetLastError());
}

// (kernels.hpp, preload_code_objects: the runtime loads a translation unit's code object at the first use of one of its kernels)
void preload_tu_semi_join() { hipFuncAttributes at; RDFGPU_HIP(hipFuncGetAttributes(&at, reinterpret_cast<const void*>((semi_build_kernel<true, true>)))); }

}  // namespace rdfgpu
