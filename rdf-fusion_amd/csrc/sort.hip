// sort.hip — SortExec (include/rdfgpu.h, RDFGPU_NODE_SORT): ORDER BY over object-id and value columns, ASC / DESC per key, with an
// optional fetch — the `SortExec: TopK(fetch=10), expr=[ENC_SORT(DIV(..)) DESC, ENC_SORT(ENC_PT(product@0)) ASC]` that ends the BSBM
// Business Intelligence plans (..Business Intelligence - Q3 / Q1 (Execution Plan).snap:6).  No DISTINCT: every input row comes out (up to
// the fetch).  Only the u32 entries of the columns are permuted; a value column's 24-byte values stay where they are.
//
// The sort key of a value (RDFGPU_SORT_BY_VALUE) restates the reference's sortable encoding: the struct (type, numeric, bytes) of
// lib/encoding/src/sortable_term/builder.rs:24-39,113-140 with the type numbers of term_type.rs:56-70, as encoders/typed_value.rs:23-50
// fills it (an error value appends a valid struct of type Null), the bytes being the value's own big-endian bytes
// (lib/model/src/xsd/numeric.rs:52-60).  Of it a 24-byte value record can hold: type 0 (unbound / the error value), type 3 (a boolean:
// numeric 0.0 / 1.0, one byte) and type 4 (INT / INTEGER / DECIMAL / FLOAT / DOUBLE: numeric = Double::from(Numeric) — to_f64, the
// Decimal -> Double routine of decimal.rs:445 included — compared in IEEE total order, then 4 / 8 / 16 bytes compared as byte strings, a
// prefix first).
//
// A comparison sort in three steps, since the keys are multi-word tuples:
//   sort_keys_kernel    one lane per live row writes the row's RECORD: `words` 64-bit words whose unsigned lexicographic order is the
//                       required order.  An id key is one word, a value key kSortValueWords; a DESC key is stored bit-inverted; the last
//                       word is the row index, so records are distinct and rows equal on every key keep their input order.
//   sort_tile_kernel    one workgroup per tile of kSortTile rows: the records in LDS word by word (word w of record r at w * kSortTile + r:
//                       a wave's 64 records of one word are 512 consecutive bytes), a bitonic network over them, the last tile padded
//                       with all-ones records (+inf: a live record's row word is below 2^32).  Leaves a sorted run of row indices.
//   sort_merge_kernel   one launch per pass, log2(runs) passes: run 2q and run 2q + 1 of the pass merge into run q of the next, by merge
//                       path — a workgroup finds the split of its kSortMergeChunk outputs, every thread the split of its kSortMergeItems
//                       inside it (binary searches on the diagonal), then merges serially, comparing the rows' records in HBM / L2.  A
//                       run without a partner is copied by the same code (its partner is empty).
//   sort_gather_kernel  the projected columns of the first rows of the final run, and the row count.
// With a fetch k every run is cut to its first min(length, k) rows after the tile sort and after every pass: TopK(fetch=10) over 10^6
// rows merges 10-row runs.  Where a run lies and how long it is follows from the pass, the live row count and k alone, so nothing is
// kept per run.  The row count may live on the device only: launch geometry comes from the capacity, every kernel reads live_rows.
#include "join_device.hpp"

namespace rdfgpu {

static_assert(kSortMaxWords * kSortTile * sizeof(u64) <= 64u * 1024u, "a tile of the widest record fills 64 KB of LDS");
static_assert((kSortTile & (kSortTile - 1)) == 0 && kSortTile >= 2 * 64, "the bitonic network needs a power of two");
constexpr u32 kSortTileThreads = kSortTile / 2;        // one compare-exchange per thread and step
constexpr u32 kSortMergeChunk = kSortMergeThreads * kSortMergeItems;

__device__ __forceinline__ const u32* sort_col(const SortArgs& a, u32 c) {   // (a chain of selects over the kernarg pointers: aggregate.hip, agg_col)
  const u32* p = a.in[0];
#pragma unroll
  for (u32 q = 1; q < (u32)kMaxCols; q++) p = c == q ? a.in[q] : p;
  return p;
}

// a double in IEEE total order as an unsigned word: -NaN < -inf < .. < -0 < +0 < .. < +inf < NaN
__device__ __forceinline__ u64 sort_ordered_f64(double d) {
  const u64 bits = (u64)__double_as_longlong(d);
  return (bits >> 63) ? ~bits : (bits | 0x8000000000000000ull);
}

// The key word of an object id, as RDFGPU_NODE_TOPK defines it (topk.hip, topk_key): the id; (tag, rank) of a string / IRI / blank node,
// anything else raising the plan's run-time flag; or the numeric value as a double in total order, everything else first.
__device__ __forceinline__ u64 sort_id_word(const SortArgs& a, u32 how, u32 id) {
  if (how == RDFGPU_SORT_BY_ID) return id;
  if (id == 0 || id >= a.tt.n_ids) return 0;
  if (how == RDFGPU_SORT_BY_DOUBLE) {
    const Val v = enc_tv(a.tt, id);
    const int k = num_kind(v.tag);
    return k == NK_NONE ? 0ull : sort_ordered_f64(to_f64(v, k));
  }
  const int4 raw = *reinterpret_cast<const int4*>(a.tt.tv + id);
  const u32 tag = (u32)raw.w & 0xff;
  if (tag != RDFGPU_TV_STRING && tag != RDFGPU_TV_NAMED_NODE && tag != RDFGPU_TV_BLANK_NODE && tag != RDFGPU_TV_NULL && a.tt.rt_error) atomicOr(a.tt.rt_error, kRtSortTerm);
  const u64 lo = ((u64)(u32)raw.y << 32) | (u32)raw.x;
  return ((u64)tag << 56) | (lo & 0x00FFFFFFFFFFFFFFull);
}

// The kSortValueWords words of a value key: the 200 bits  type:3 | numeric:64 | bytes:128 (left-aligned, zero-padded) | length:5, from the
// top.  Zero padding then the length is the byte-string order: a differing byte inside the common length decides as it stands; a prefix
// pads to no more than the longer string, and if to the same the shorter length wins.
__device__ __forceinline__ void sort_value_words(const rdfgpu_agg_value* values, u64 n_values, u32 idx, u64* w) {
  u64 type = 0, numeric = 0, len = 0;   // unbound, the error value: type Null, and nothing else to tell two of them apart
  u128_t bytes = 0;
  if (idx != 0 && (u64)idx <= n_values) {
    const long long* p = reinterpret_cast<const long long*>(values) + 3ull * (idx - 1u);
    Val v = val_tv_null();
    v.lo = p[0]; v.hi = p[1]; v.tag = (u8)((u64)p[2] & 0xff);
    const int k = num_kind(v.tag);
    if (v.tag == RDFGPU_TV_BOOLEAN) {
      type = 3; numeric = sort_ordered_f64(v.lo ? 1.0 : 0.0); bytes = (u128_t)(v.lo ? 1u : 0u) << 120; len = 1;
    } else if (k != NK_NONE) {
      type = 4; numeric = sort_ordered_f64(to_f64(v, k));
      if (k == NK_INT || k == NK_FLOAT) { bytes = (u128_t)(u32)v.lo << 96; len = 4; }
      else if (k == NK_INTEGER || k == NK_DOUBLE) { bytes = (u128_t)(u64)v.lo << 64; len = 8; }
      else { bytes = (u128_t)val_dec(v); len = 16; }
    }
  }
  w[0] = (type << 61) | (numeric >> 3);
  w[1] = (numeric << 61) | (u64)(bytes >> 67);
  w[2] = (u64)(bytes >> 3);
  w[3] = ((u64)bytes << 61) | (len << 56);
}

__global__ __launch_bounds__(256) void sort_keys_kernel(const SortArgs a) {
  const u64 n = live_rows(a.n_in_dev, a.n_in_cap);
  const u64 row = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  u64* rec = a.rec + row * a.words;
  u32 at = 0;
  for (u32 k = 0; k < a.n_keys; k++) {
    const u32 entry = sort_col(a, a.key_col[k])[row];
    const u64 flip = a.key_desc[k] ? ~0ull : 0ull;
    if (a.key_how[k] == RDFGPU_SORT_BY_VALUE) {
      u64 w[kSortValueWords];
      sort_value_words(a.key_values[k], a.key_n_values[k], entry, w);
#pragma unroll
      for (u32 q = 0; q < kSortValueWords; q++) rec[at + q] = w[q] ^ flip;
      at += kSortValueWords;
    } else {
      rec[at++] = sort_id_word(a, a.key_how[k], entry) ^ flip;
    }
  }
  rec[at] = row;   // at == a.words - 1 (Plan::exec_sort lays the keys out the same way)
}

__global__ __launch_bounds__(kSortTileThreads) void sort_tile_kernel(const SortArgs a) {
  extern __shared__ __attribute__((aligned(16))) u64 tile[];   // a.words * kSortTile words
  const u64 n = live_rows(a.n_in_dev, a.n_in_cap);
  const u64 base = (u64)blockIdx.x * kSortTile;
  if (base >= n) return;                                         // (uniform over the workgroup)
  const u32 W = a.words, tid = threadIdx.x;
  const u32 live = n - base < kSortTile ? (u32)(n - base) : kSortTile;
  const u64* src = a.rec + base * W;                             // the tile's records are consecutive: read in address order
  for (u32 f = tid; f < kSortTile * W; f += kSortTileThreads) {
    const u32 r = f / W, w = f - r * W;
    tile[w * kSortTile + r] = r < live ? src[f] : ~0ull;
  }
  for (u32 k = 2; k <= kSortTile; k <<= 1) {
    for (u32 j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      const u32 i = ((tid & ~(j - 1)) << 1) | (tid & (j - 1)), p = i | j;   // the pair (i, i + j) of this step
      const bool ascending = (i & k) == 0;
      u32 w = 0;
      u64 x = 0, y = 0;
      for (; w < W; w++) { x = tile[w * kSortTile + i]; y = tile[w * kSortTile + p]; if (x != y) break; }
      if (w < W && (x > y) == ascending) {                       // out of order: the words before w are equal, the rest change places
        for (; w < W; w++) {
          x = tile[w * kSortTile + i]; y = tile[w * kSortTile + p];
          tile[w * kSortTile + i] = y; tile[w * kSortTile + p] = x;
        }
      }
    }
  }
  __syncthreads();
  const u64 keep = a.fetch && a.fetch < live ? a.fetch : live;   // the run, cut to the fetch
  for (u32 r = tid; r < keep; r += kSortTileThreads) a.run[0][base + r] = (u32)tile[(W - 1) * kSortTile + r];
}

// whether row x sorts before row y: their records' key words, then the row index (the records' last word)
__device__ __forceinline__ bool sort_row_less(const u64* rec, u32 key_words, u32 W, u32 x, u32 y) {
  const u64* rx = rec + (u64)x * W;
  const u64* ry = rec + (u64)y * W;
  for (u32 w = 0; w < key_words; w++) { const u64 p = rx[w], q = ry[w]; if (p != q) return p < q; }
  return x < y;
}
// Merge path: of the first d rows of merge(A[0, hi_a), B), how many come from A — searched in [lo, hi], which the caller has narrowed.
__device__ __forceinline__ u64 sort_merge_split(const u64* rec, u32 W, const u32* A, const u32* B, u64 d, u64 lo, u64 hi) {
  while (lo < hi) {
    const u64 mid = (lo + hi) >> 1;
    if (sort_row_less(rec, W - 1, W, A[mid], B[d - 1 - mid])) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kSortMergeThreads) void sort_merge_kernel(const SortArgs a, const u32 pass, const u32 blocks_per_pair) {
  __shared__ u64 split[2];
  const u64 n = live_rows(a.n_in_dev, a.n_in_cap);
  const u64 S = (u64)kSortTile << pass;                          // rows a run of this pass stands for
  const u64 pair = blockIdx.x / blocks_per_pair, chunk = blockIdx.x % blocks_per_pair;
  const u64 a0 = pair * 2 * S, b0 = a0 + S;
  if (a0 >= n) return;                                           // (uniform over the workgroup)
  const u64 kk = a.fetch ? a.fetch : ~0ull;
  const u64 rows_a = n - a0 < S ? n - a0 : S, rows_b = b0 < n ? (n - b0 < S ? n - b0 : S) : 0;
  const u64 la = rows_a < kk ? rows_a : kk, lb = rows_b < kk ? rows_b : kk;   // the runs, as the step before cut them
  const u64 total = la + lb < kk ? la + lb : kk;                              // .. and this pair's, cut again
  const u64 d0 = chunk * kSortMergeChunk;
  if (d0 >= total) return;
  const u64 d1 = d0 + kSortMergeChunk < total ? d0 + kSortMergeChunk : total;
  const u32* A = a.run[pass & 1] + a0;
  const u32* B = a.run[pass & 1] + b0;                           // (never read when lb == 0)
  u32* out = a.run[(pass + 1) & 1] + a0;
  const u32 W = a.words;
  if (threadIdx.x < 2) {                                         // the workgroup's own splits: where its chunk begins and ends in A
    const u64 d = threadIdx.x ? d1 : d0;
    split[threadIdx.x] = sort_merge_split(a.rec, W, A, B, d, d > lb ? d - lb : 0, d < la ? d : la);
  }
  __syncthreads();
  const u64 ia0 = split[0], ia1 = split[1], jb0 = d0 - ia0, jb1 = d1 - ia1;
  const u64 d = d0 + (u64)threadIdx.x * kSortMergeItems;
  if (d >= d1) return;
  // this thread's split lies between the workgroup's: ia0 <= i <= ia1 and jb0 <= d - i <= jb1
  u64 i = sort_merge_split(a.rec, W, A, B, d, d > jb1 && d - jb1 > ia0 ? d - jb1 : ia0, d - jb0 < ia1 ? d - jb0 : ia1);
  u64 j = d - i;
  const u64 end = d + kSortMergeItems < d1 ? d + kSortMergeItems : d1;
  for (u64 o = d; o < end; o++) {                                // (o < total <= la + lb: one of the two runs has a row left)
    const bool from_a = j >= lb || (i < la && sort_row_less(a.rec, W - 1, W, A[i], B[j]));
    out[o] = from_a ? A[i++] : B[j++];
  }
}

__global__ __launch_bounds__(256) void sort_gather_kernel(const SortArgs a, const u32 final_run) {
  const u64 n = live_rows(a.n_in_dev, a.n_in_cap);
  const u64 n_out = a.fetch && a.fetch < n ? a.fetch : n;
  const u64 pos = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (pos == 0 && a.n_out_dev) *a.n_out_dev = n_out;
  if (pos >= n_out) return;
  const u32 row = a.run[final_run][pos];
  for (u32 c = 0; c < a.n_out_cols; c++) a.out[c][pos] = sort_col(a, a.proj[c])[row];
}

static inline dim3 sort_grid(u64 n, u64 per_block) { const u64 g = (n + per_block - 1) / per_block; return dim3((unsigned)(g ? g : 1)); }
u32 sort_merge_passes(u64 cap) {
  const u64 runs = (cap + kSortTile - 1) / kSortTile;
  u32 passes = 0;
  while ((1ull << passes) < runs) passes++;
  return passes;
}
void launch_sort_keys(const SortArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(sort_keys_kernel, sort_grid(a.n_in_cap, 256), dim3(256), 0, s, a);
  RDFGPU_HIP(hipGetLastError());
}
void launch_sort_tile(const SortArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(sort_tile_kernel, sort_grid(a.n_in_cap, kSortTile), dim3(kSortTileThreads), (size_t)a.words * kSortTile * sizeof(u64), s, a);
  RDFGPU_HIP(hipGetLastError());
}
void launch_sort_merge(const SortArgs& a, u32 pass, hipStream_t s) {
  const u64 S = (u64)kSortTile << pass;
  const u64 runs = (a.n_in_cap + S - 1) / S, pairs = (runs + 1) / 2;
  u64 rows = 2 * S < a.n_in_cap ? 2 * S : a.n_in_cap;            // the most rows one pair writes
  if (a.fetch && a.fetch < rows) rows = a.fetch;
  const u64 blocks_per_pair = (rows + kSortMergeChunk - 1) / kSortMergeChunk;
  hipLaunchKernelGGL(sort_merge_kernel, dim3((unsigned)(pairs * blocks_per_pair)), dim3(kSortMergeThreads), 0, s, a, pass, (u32)blocks_per_pair);
  RDFGPU_HIP(hipGetLastError());
}
void launch_sort_gather(const SortArgs& a, u32 final_run, u64 out_cap, hipStream_t s) {
  hipLaunchKernelGGL(sort_gather_kernel, sort_grid(out_cap, 256), dim3(256), 0, s, a, final_run);
  RDFGPU_HIP(hipGetLastError());
}

// (kernels.hpp, preload_code_objects: the runtime loads a translation unit's code object at the first use of one of its kernels)
void preload_tu_sort() { hipFuncAttributes at; RDFGPU_HIP(hipFuncGetAttributes(&at, reinterpret_cast<const void*>(sort_keys_kernel))); }

}  // namespace rdfgpu
