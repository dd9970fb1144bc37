// aggregate.hip — AggregateExec(mode=Single) over object-id group columns: COUNT(*), COUNT, COUNT(DISTINCT), SUM, AVG, MIN, MAX
// (include/rdfgpu.h, RDFGPU_NODE_AGGREGATE; lib/functions/src/aggregates/sum.rs:34-73, avg.rs:43-134, min.rs / max.rs).
//
// Three passes over the input, the group count read back once in between (it sizes the accumulators):
//   agg_groups_kernel  every row finds its key tuple in one open-addressing table in HBM (slot = row + 1 of the row that claimed it; a
//                      row whose tuple is there already only reads).  A claiming row takes the next dense group index: the claims of a
//                      1024-row tile are compacted with ballot + mbcnt behind ONE counter reservation per workgroup and tile.
//   agg_accum_kernel   every row adds into its group's accumulator words.  Rows of a wave are consecutive rows, so runs of equal
//                      neighbouring groups (clustered join output, one hot group) are summed within the wave first and only the run's
//                      head lane issues the atomic (Guideline 12).  When every group's words fit in 64 KiB, each workgroup keeps
//                      partials in LDS and merges them into HBM once; otherwise (or with NO_AGG_LDS) the atomics go to HBM directly.
//   agg_final_kernel   one lane per group: the key ids from the group's first row, every aggregate's rdfgpu_agg_value.
// A node with a value column among its group columns, or more than 4 of them (RDFGPU_PLAN_VALUE_KEYS), runs agg_groups_wide_kernel as its
// group pass (same contract: row_slot, slot_gid, rep_row, the count) and agg_wide_keys_kernel for the key columns 4..; the rest is shared.
// When aggregate values are columns (RDFGPU_PLAN_AGG_COLUMNS) a fourth, agg_value_cols_kernel, writes each aggregate's value column.
// A node with a MIN / MAX (RDFGPU_PLAN_AGG_COLUMNS only) runs the MINMAX instantiation of the accumulate pass (agg_accum_minmax_kernel),
// then agg_minmax_refine_kernel (the low word of decimal candidates) and, beside agg_final_kernel, agg_minmax_final_kernel.
//
// Accumulator words of one group (u64, word w of group g at acc[w * groups + g]): word 0 counts the group's rows; COUNT / COUNT DISTINCT have one
// (rows with a bound id / first insertions of (group, id) into the aggregate's set); SUM / AVG and MIN / MAX index theirs by the names of kernels.hpp.
// A limb sum of up to 2^32 rows fits a u64, and two's complement makes the exact total sum(limb_i * 2^(32 i)) - negatives * 2^64 (2^128):
// integer and decimal results are exact and do not depend on row order.  Float and double results are the f64 sums, in the device's
// order (the header states the bound).
#include <algorithm>

#include "join_device.hpp"

namespace rdfgpu {

constexpr int kAggBlock = 256;
constexpr int kAggItems = 4;                        // rows per lane and tile of the group pass: one reservation per 1024 rows
constexpr u32 kAggTile = (u32)kAggBlock * kAggItems;
constexpr u32 kGroupNone = 0xFFFFFFFFu;
// Workgroups of a launch, at most.  In the LDS form every workgroup zeroes and merges all partials: enough to fill the part, not one per tile.
constexpr u64 kAggGroupGrid = 16384, kAggAccumLdsGrid = 512, kAggAccumHbmGrid = 16384;
enum : u32 { kKindInt = 1, kKindDec = 2, kKindFloat = 4, kKindDouble = 8, kKindOther = 16 };

// ---- pass 1 ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ Keys agg_keys(const AggArgs& a, u64 row) {
  Keys k;
#pragma unroll
  for (u32 q = 0; q < RDFGPU_MAX_KEYS; q++) k.k[q] = q < a.n_keys ? a.key[q][row] : 0u;   // id 0 is a key value like any other
  return k;
}
__device__ __forceinline__ bool agg_keys_equal(const AggArgs& a, u64 row, const Keys& k) {
  bool eq = true;
#pragma unroll
  for (u32 q = 0; q < RDFGPU_MAX_KEYS; q++) if (q < a.n_keys) eq = eq && a.key[q][row] == k.k[q];
  return eq;
}

__global__ __launch_bounds__(kAggBlock) void agg_groups_kernel(const AggArgs a) {
  __shared__ u32 wave_tot[kAggBlock / 64];
  __shared__ u64 wg_base;
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u64 n = live_rows(a.n_dev, a.cap);
  const u64 n_tiles = (n + kAggTile - 1) / kAggTile;
  for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    u64 row[kAggItems]; u32 slot[kAggItems]; bool won[kAggItems];
#pragma unroll
    for (int it = 0; it < kAggItems; it++) {
      row[it] = tile * kAggTile + (u64)it * kAggBlock + tid;
      won[it] = false; slot[it] = 0;
      if (row[it] >= n) continue;
      const Keys k = agg_keys(a, row[it]);
      u32 h = hash_keys4(k, a.n_keys) & a.slot_mask;
      for (;;) {   // load factor <= 0.5: an empty slot exists
        u32 cur = a.slots[h];   // slots are written once: a stale read can only be a 0, which the CAS settles
        if (cur == 0) {
          cur = atomicCAS(a.slots + h, 0u, (u32)row[it] + 1u);
          if (cur == 0) { won[it] = true; break; }
        }
        if (agg_keys_equal(a, cur - 1, k)) break;
        h = (h + 1) & a.slot_mask;
      }
      slot[it] = h;
      a.row_slot[row[it]] = h;
    }
    unsigned long long mask[kAggItems]; u32 off[kAggItems]; u32 wtot = 0;
#pragma unroll
    for (int it = 0; it < kAggItems; it++) { mask[it] = __ballot(won[it]); off[it] = wtot; wtot += (u32)__popcll(mask[it]); }
    if (lane == 0) wave_tot[wave] = wtot;
    __syncthreads();
    if (tid == 0) {
      u32 total = 0;
      for (int w = 0; w < kAggBlock / 64; w++) { const u32 t = wave_tot[w]; wave_tot[w] = total; total += t; }
      wg_base = total ? atomicAdd((unsigned long long*)a.n_groups_dev, (unsigned long long)total) : 0ull;
    }
    __syncthreads();
    const u64 base = wg_base + wave_tot[wave];
#pragma unroll
    for (int it = 0; it < kAggItems; it++) {
      if (!won[it]) continue;
      const u32 gid = (u32)(base + off[it] + lane_prefix(mask[it]));
      a.slot_gid[slot[it]] = gid;
      a.rep_row[gid] = (u32)row[it];
    }
    __syncthreads();   // wave_tot / wg_base are reused by the next tile
  }
}

// ---- pass 1, the wide form (RDFGPU_PLAN_VALUE_KEYS): value columns among the group columns, or more than RDFGPU_MAX_KEYS of them ----------
// The same table, claim and compaction as agg_groups_kernel; only what a key IS differs.  An id key is its u32.  A value key is the plain
// term its value stands for (the reference groups by ENC_PT of the column), in the canonical form of include/rdfgpu.h: the tag, `lo`, and
// `hi` for a decimal only; every NaN of a tag is one term; +0.0 and -0.0, and INTEGER / INT / DECIMAL of one value, are different terms;
// entry 0, an entry behind the array and a record with tag RDFGPU_TV_NULL are all "unbound", one key value.  The canonical words are
// hashed, never the entry: equal values have different entries.  A row's own record is a stream (a computed column's entry is row + 1),
// the claimant's a gather; two equal entries are the same record and need no read.
struct WideKey { u32 tag; u64 lo, hi; };
__device__ __forceinline__ WideKey wide_value_key(const rdfgpu_agg_value* val, u64 val_n, u32 e) {
  WideKey k{RDFGPU_TV_NULL, 0ull, 0ull};
  if (e == 0 || (u64)e > val_n) return k;
  const unsigned long long* p = reinterpret_cast<const unsigned long long*>(val) + 3ull * (e - 1u);
  const u32 tag = (u32)(p[2] & 0xffull);
  if (tag == RDFGPU_TV_NULL) return k;
  k.tag = tag; k.lo = p[0];
  if (tag == RDFGPU_TV_DECIMAL) k.hi = p[1];
  else if (tag == RDFGPU_TV_FLOAT && ((u32)k.lo & 0x7FFFFFFFu) > 0x7F800000u) k.lo = 0x7FC00000ull;
  else if (tag == RDFGPU_TV_DOUBLE && (k.lo & ~(1ull << 63)) > 0x7FF0000000000000ull) k.lo = 0x7FF8000000000000ull;
  return k;
}
__device__ __forceinline__ u32 wide_mix(u32 h, u32 v) { h ^= v; h *= 0x9E3779B1u; h ^= h >> 15; return h; }
__device__ __forceinline__ u32 wide_hash(const AggWideArgs& w, u64 row) {
  u32 h = 0x811C9DC5u;
#pragma unroll
  for (u32 q = 0; q < RDFGPU_MAX_GROUP_KEYS; q++) {
    if (q >= w.n_keys) continue;
    const u32 e = w.key[q][row];
    if (!(w.value_mask >> q & 1u)) { h = wide_mix(h, e); continue; }
    const WideKey k = wide_value_key(w.val[q], w.val_n[q], e);
    h = wide_mix(h, k.tag); h = wide_mix(h, (u32)k.lo); h = wide_mix(h, (u32)(k.lo >> 32)); h = wide_mix(h, (u32)k.hi); h = wide_mix(h, (u32)(k.hi >> 32));
  }
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return h;
}
__device__ __forceinline__ bool wide_rows_equal(const AggWideArgs& w, u64 ra, u64 rb) {
  bool eq = true;
#pragma unroll
  for (u32 q = 0; q < RDFGPU_MAX_GROUP_KEYS; q++) {
    if (q >= w.n_keys || !eq) continue;
    const u32 ea = w.key[q][ra], eb = w.key[q][rb];
    if (ea == eb) continue;
    if (!(w.value_mask >> q & 1u)) { eq = false; continue; }
    const WideKey x = wide_value_key(w.val[q], w.val_n[q], ea), y = wide_value_key(w.val[q], w.val_n[q], eb);
    eq = x.tag == y.tag && x.lo == y.lo && x.hi == y.hi;
  }
  return eq;
}

__global__ __launch_bounds__(kAggBlock) void agg_groups_wide_kernel(const AggWideArgs w) {
  __shared__ u32 wave_tot[kAggBlock / 64];
  __shared__ u64 wg_base;
  const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u64 n = live_rows(w.n_dev, w.cap);
  const u64 n_tiles = (n + kAggTile - 1) / kAggTile;
  for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    u64 row[kAggItems]; u32 slot[kAggItems]; bool won[kAggItems];
#pragma unroll
    for (int it = 0; it < kAggItems; it++) {
      row[it] = tile * kAggTile + (u64)it * kAggBlock + tid;
      won[it] = false; slot[it] = 0;
      if (row[it] >= n) continue;
      u32 h = wide_hash(w, row[it]) & w.slot_mask;
      for (;;) {   // load factor <= 0.5: an empty slot exists
        u32 cur = w.slots[h];   // slots are written once: a stale read can only be a 0, which the CAS settles
        if (cur == 0) {
          cur = atomicCAS(w.slots + h, 0u, (u32)row[it] + 1u);
          if (cur == 0) { won[it] = true; break; }
        }
        if (wide_rows_equal(w, cur - 1, row[it])) break;
        h = (h + 1) & w.slot_mask;
      }
      slot[it] = h;
      w.row_slot[row[it]] = h;
    }
    unsigned long long mask[kAggItems]; u32 off[kAggItems]; u32 wtot = 0;
#pragma unroll
    for (int it = 0; it < kAggItems; it++) { mask[it] = __ballot(won[it]); off[it] = wtot; wtot += (u32)__popcll(mask[it]); }
    if (lane == 0) wave_tot[wave] = wtot;
    __syncthreads();
    if (tid == 0) {
      u32 total = 0;
      for (int q = 0; q < kAggBlock / 64; q++) { const u32 t = wave_tot[q]; wave_tot[q] = total; total += t; }
      wg_base = total ? atomicAdd((unsigned long long*)w.n_groups_dev, (unsigned long long)total) : 0ull;
    }
    __syncthreads();
    const u64 base = wg_base + wave_tot[wave];
#pragma unroll
    for (int it = 0; it < kAggItems; it++) {
      if (!won[it]) continue;
      const u32 gid = (u32)(base + off[it] + lane_prefix(mask[it]));
      w.slot_gid[slot[it]] = gid;
      w.rep_row[gid] = (u32)row[it];
    }
    __syncthreads();   // wave_tot / wg_base are reused by the next tile
  }
}

// The key columns RDFGPU_MAX_KEYS .. of the wide form, one lane per group: the representative row's entries (agg_final_kernel copies the
// first four as it always did; a value key's entry indexes the same value array as the input's).
__global__ __launch_bounds__(kAggBlock) void agg_wide_keys_kernel(const AggWideArgs w) {
  const u32 g = blockIdx.x * kAggBlock + threadIdx.x;
  if (g >= w.n_groups) return;
  const u32 rep = w.rep_row[g];
#pragma unroll
  for (u32 q = RDFGPU_MAX_KEYS; q < RDFGPU_MAX_GROUP_KEYS; q++) if (q < w.n_keys) w.out_key[q][g] = w.key[q][rep];
}

// ---- pass 2 ---------------------------------------------------------------------------------------------------------------------
// A lane's run: the lanes [lane, end) of its wave hold rows of the same group; the head lane (first of the run) issues the atomic.
struct AggRun { u32 lane, end; bool head; bool merge; };
// Where the accumulate pass adds: the workgroup's partials in LDS (the LDS form, same layout) or the accumulators in HBM.
template <bool LDS> __device__ __forceinline__ unsigned long long* agg_acc(const AggArgs& a) {
  extern __shared__ unsigned long long lacc[];
  if constexpr (LDS) return lacc; else return a.acc;
}
// The group of a row (kGroupNone behind the live rows), and the run of its lane among the wave's groups.
__device__ __forceinline__ u32 agg_group(const AggArgs& a, u64 row, bool valid) { return !valid ? kGroupNone : a.n_keys ? a.slot_gid[a.row_slot[row]] : 0u; }
__device__ __forceinline__ AggRun agg_run(u32 g, bool valid, u32 lane) {
  const u32 prev = __shfl_up(g, 1);
  const bool head = lane == 0 || prev != g;
  const unsigned long long heads = __ballot(head);
  const unsigned long long after = heads & ~((2ull << lane) - 1ull);   // heads of later lanes (lane 63: 2 << 63 wraps to 0, none)
  return AggRun{lane, after ? (u32)__ffsll((long long)after) - 1u : 64u, head && valid, heads != ~0ull};
}
// Where the first word of aggregate `i` lies for group `g`; word `word` (an AggSumWord / AggMinMaxWord) of the aggregate whose first is at `w`.
__device__ __forceinline__ u64 agg_word0(const AggArgs& a, u32 i, u32 g) { return (u64)a.word0[i] * a.n_groups + g; }
__device__ __forceinline__ u64 agg_word(const AggArgs& a, u64 w, u32 word) { return w + (u64)word * a.n_groups; }

template <class T, class Op>
__device__ __forceinline__ T run_reduce(T v, const AggRun& r, Op op) {
  if (!r.merge) return v;   // (uniform: no run of the wave is longer than one lane)
#pragma unroll
  for (u32 off = 1; off < 64; off <<= 1) {
    const T o = __shfl_down(v, off);
    if (r.lane + off < r.end) v = op(v, o);
  }
  return v;
}
__device__ __forceinline__ void acc_add(unsigned long long* acc, u64 at, unsigned long long v, const AggRun& r) {
  v = run_reduce(v, r, [](unsigned long long x, unsigned long long y) { return x + y; });
  if (r.head && v) atomicAdd(acc + at, v);
}
__device__ __forceinline__ void acc_or(unsigned long long* acc, u64 at, unsigned long long v, const AggRun& r) {
  v = run_reduce(v, r, [](unsigned long long x, unsigned long long y) { return x | y; });
  if (r.head && v) atomicOr(acc + at, v);
}
__device__ __forceinline__ void acc_add_f64(unsigned long long* acc, u64 at, double v, const AggRun& r) {
  v = run_reduce(v, r, [](double x, double y) { return __dadd_rn(x, y); });
  if (r.head && v != 0.0) unsafeAtomicAdd(reinterpret_cast<double*>(acc + at), v);
}
// MIN / MAX: the largest key of the run.  0 is the identity (zeroed memory), so a wave none of whose lanes holds a key for this word —
// every word but one, over a column of one kind — leaves before the shuffles.
__device__ __forceinline__ void acc_max(unsigned long long* acc, u64 at, unsigned long long v, const AggRun& r) {
  if (!__any(v != 0ull)) return;
  v = run_reduce(v, r, [](unsigned long long x, unsigned long long y) { return x > y ? x : y; });
  // The word only grows, so a key that is not above what is there changes nothing: read first, and most rows of a group that has met
  // its extremum issue no atomic (every row of one group on one word ran at the contended-atomic rate).  A stale read costs only the
  // atomic it would have saved.
  if (r.head && v && v > __hip_atomic_load(acc + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(acc + at, v);
}

// ---- MIN / MAX (min.rs / max.rs; the rule is in include/rdfgpu.h) ----------------------------------------------------------------
// Words of one MIN / MAX (AggMinMaxWord): the flags below (kAggOr), one key per kind, the decimal's low word.  A key is an order-preserving
// u64 of the value, complemented for MIN: the largest key is the candidate for both functions and 0 is the identity of both, so the memset
// and the merge that skips zero partials stay what they are.  A kind's `seen` bit tells a legitimate key of 0 from "no value".
enum : u32 { kMmSeen0 = 1, kMmNanFloat = 32, kMmNanDouble = 64, kMmError = 128, kMmOther = 256 };
__device__ __forceinline__ u64 mm_key_i64(long long v) { return (u64)v ^ (1ull << 63); }
__device__ __forceinline__ u64 mm_key_f32(u32 b) { return (b & 0x80000000u) ? (u32)~b : (b | 0x80000000u); }   // IEEE order, -0 below +0
__device__ __forceinline__ u64 mm_key_f64(u64 b) { return (b >> 63) ? ~b : (b | (1ull << 63)); }
__device__ __forceinline__ u32 mm_unkey_f32(u64 k) { const u32 b = (u32)k; return (b & 0x80000000u) ? (b & 0x7FFFFFFFu) : ~b; }
__device__ __forceinline__ u64 mm_unkey_f64(u64 k) { return (k >> 63) ? (k & ~(1ull << 63)) : ~k; }

// One row's contribution: which flag it sets and, for a numeric value that is not NaN, its kind (AggMinMaxKind) and key (before MIN's complement).
struct MmRow { u32 flags; u32 kind; u64 key; bool has; };
__device__ __forceinline__ MmRow mm_row(const Val& v) {
  MmRow m{0, 0, 0, false};
  switch (num_kind(v.tag)) {
    case NK_INT: m.kind = kMmInt; m.key = mm_key_i64(v.lo); m.has = true; break;
    case NK_INTEGER: m.kind = kMmInteger; m.key = mm_key_i64(v.lo); m.has = true; break;
    case NK_DECIMAL: m.kind = kMmDecKind; m.key = mm_key_i64(v.hi); m.has = true; break;
    case NK_FLOAT: { const u32 b = (u32)v.lo; if ((b & 0x7FFFFFFFu) > 0x7F800000u) m.flags = kMmNanFloat; else { m.kind = kMmFloat; m.key = mm_key_f32(b); m.has = true; } break; }
    case NK_DOUBLE: { const u64 b = (u64)v.lo; if ((b & ~(1ull << 63)) > 0x7FF0000000000000ull) m.flags = kMmNanDouble; else { m.kind = kMmDouble; m.key = mm_key_f64(b); m.has = true; } break; }
    default: m.flags = v.tag == RDFGPU_TV_NULL ? kMmError : kMmOther;
  }
  if (m.has) m.flags = kMmSeen0 << m.kind;
  return m;
}
// .. into the words of a MIN (`mn`) / MAX whose first word of the row's group is at `w`.  true: the row held a decimal (the refinement has work).
template <bool LDS> __device__ __forceinline__ bool minmax_accum(const AggArgs& a, u64 w, const Val v, bool valid, bool mn, const AggRun& r) {
  unsigned long long* acc = agg_acc<LDS>(a);
  MmRow m = mm_row(v);
  if (!valid) m = MmRow{0, 0, 0, false};
  if (mn) m.key = ~m.key;
  acc_or(acc, agg_word(a, w, kMmFlags), m.flags, r);
#pragma unroll
  for (u32 q = 0; q < kMmKinds; q++) acc_max(acc, agg_word(a, w, kMmKey0 + q), m.has && m.kind == q ? m.key : 0ull, r);
  return m.has && m.kind == kMmDecKind;
}

// One row's contribution to the words of a SUM / AVG whose first word of the row's group is at `w`.
template <bool LDS> __device__ __forceinline__ void sum_accum(const AggArgs& a, u64 w, const Val v, bool valid, const AggRun& r) {
  unsigned long long* acc = agg_acc<LDS>(a);
  const int k = num_kind(v.tag);
  u32 kind = k == NK_NONE ? kKindOther : k == NK_DECIMAL ? kKindDec : k == NK_FLOAT ? kKindFloat : k == NK_DOUBLE ? kKindDouble : kKindInt;
  if (!valid) kind = 0;
  const bool is_int = kind == kKindInt, is_dec = kind == kKindDec, num = valid && k != NK_NONE;
  const u64 ix = is_int ? (u64)v.lo : 0ull;
  const u64 d0 = is_dec ? (u64)v.lo : 0ull, d1 = is_dec ? (u64)v.hi : 0ull;
  acc_or(acc, agg_word(a, w, kSumKinds), kind, r);
  acc_add(acc, agg_word(a, w, kSumIntLo), ix & 0xFFFFFFFFull, r);
  acc_add(acc, agg_word(a, w, kSumIntHi), ix >> 32, r);
  acc_add(acc, agg_word(a, w, kSumIntNeg), is_int && v.lo < 0, r);
  acc_add(acc, agg_word(a, w, kSumDec0), d0 & 0xFFFFFFFFull, r);
  acc_add(acc, agg_word(a, w, kSumDec1), d0 >> 32, r);
  acc_add(acc, agg_word(a, w, kSumDec2), d1 & 0xFFFFFFFFull, r);
  acc_add(acc, agg_word(a, w, kSumDec3), d1 >> 32, r);
  acc_add(acc, agg_word(a, w, kSumDecNeg), is_dec && v.hi < 0, r);
  acc_add_f64(acc, agg_word(a, w, kSumF64), num ? to_f64(v, k) : 0.0, r);
  acc_add_f64(acc, agg_word(a, w, kSumF32), num ? (double)to_f32(v, k) : 0.0, r);
}

// First insertion of (g, id) into the COUNT DISTINCT set.
__device__ __forceinline__ bool dset_insert(unsigned long long* set, u32 mask, u32 g, u32 id) {
  const unsigned long long e = ((unsigned long long)g << 32) | id;
  Keys k; k.k[0] = g; k.k[1] = id; k.k[2] = 0; k.k[3] = 0;
  u32 h = hash_keys4(k, 2) & mask;
  for (;;) {
    unsigned long long cur = set[h];
    if (cur == e) return false;
    if (cur == 0ull) {
      cur = atomicCAS(set + h, 0ull, e);
      if (cur == 0ull) return true;
      if (cur == e) return false;
    }
    h = (h + 1) & mask;
  }
}

// Column `c` of the input, for an aggregate's program: `c` comes from the program (wave-uniform), and indexing the kernarg array with it
// would copy the array to scratch — a chain of value selects over the pointers stays in SGPRs ("What the generic VM costs").
__device__ __forceinline__ const u32* agg_col(const AggArgs& a, u32 c) {
  const u32* p = a.col[0];
#pragma unroll
  for (u32 q = 1; q < (u32)kMaxCols; q++) p = c == q ? a.col[q] : p;
  return p;
}
// The input of aggregate `i` at `row`: its id (0 behind the live rows, and for an expression input, which has no column) ..
template <bool EXPR> __device__ __forceinline__ u32 agg_input_id(const AggArgs& a, u32 i, u64 row, bool valid) {
  return valid && (!EXPR || a.in[i]) ? a.in[i][row] : 0u;
}
// .. and its value: ENC_TV of that id, one 16-byte gather, or the value of the aggregate's program (uniform).  COUNT / COUNT DISTINCT stop at the id.
template <bool EXPR, bool LEX> __device__ __forceinline__ Val agg_input(const AggArgs& a, u32 i, u32 id, u64 row, bool valid) {
  if constexpr (EXPR) return a.prog[i] ? eval_program<LEX>(*a.prog[i], a.tt, [&](u32 c) { return valid ? agg_col(a, c)[row] : 0u; }) : enc_tv(a.tt, id);
  else return enc_tv(a.tt, id);
}

// EXPR: some aggregate reads an expression (RDFGPU_AGG_INPUT_EXPR): its value is its program's, evaluated by the VM.  A node whose aggregates
// are all plain columns runs the instantiation without the VM in it.  MINMAX: some aggregate is a MIN / MAX; the others leave that code out.
template <bool LDS, bool EXPR, bool LEX = false, bool MINMAX = false>
__device__ __forceinline__ void agg_accum_rows(const AggArgs& a) {
  const u32 tid = threadIdx.x, lane = tid & 63;
  [[maybe_unused]] bool dec_seen = false;
  const u64 n = live_rows(a.n_dev, a.cap);
  const u32 G = a.n_groups;
  unsigned long long* const acc = agg_acc<LDS>(a);
  if constexpr (LDS) {
    for (u32 i = tid; i < a.n_words * G; i += kAggBlock) acc[i] = 0ull;
    __syncthreads();
  }
  for (u64 base = (u64)blockIdx.x * kAggBlock; base < n; base += (u64)gridDim.x * kAggBlock) {
    const u64 row = base + tid;
    const bool valid = row < n;
    const u32 g = agg_group(a, row, valid);
    const AggRun r = agg_run(g, valid, lane);
    acc_add(acc, g, 1ull, r);   // word 0: rows of the group
    for (u32 i = 0; i < a.n_aggs; i++) {
      const u32 fn = a.fn[i];
      if (fn == RDFGPU_AGG_COUNT_STAR) continue;
      const u64 w = agg_word0(a, i, valid ? g : 0u);
      const u32 id = agg_input_id<EXPR>(a, i, row, valid);
      if (fn == RDFGPU_AGG_COUNT) { acc_add(acc, w, id != 0, r); continue; }
      if (fn == RDFGPU_AGG_COUNT_DISTINCT) { acc_add(acc, w, id != 0 && dset_insert(a.dset[i], a.dset_mask, g, id), r); continue; }
      const Val v = agg_input<EXPR, LEX>(a, i, id, row, valid);
      if (MINMAX && agg_is_minmax(fn)) dec_seen = minmax_accum<LDS>(a, w, v, valid, fn == RDFGPU_AGG_MIN, r) || dec_seen;   // (uniform)
      else sum_accum<LDS>(a, w, v, valid, r);
    }
  }
  if constexpr (LDS) {   // merge this workgroup's partials once (same layout: the LDS form holds every group)
    __syncthreads();
    for (u32 i = tid; i < a.n_words * G; i += kAggBlock) {
      const unsigned long long v = acc[i];
      if (v == 0ull) continue;
      const u8 op = a.word_op[i / G];
      if (op == kAggOr) atomicOr(a.acc + i, v);
      else if (MINMAX && op == kAggMax) atomicMax(a.acc + i, v);
      else if (op == kAggAddF64) unsafeAtomicAdd(reinterpret_cast<double*>(a.acc + i), __longlong_as_double((long long)v));
      else atomicAdd(a.acc + i, v);
    }
  }
  if constexpr (MINMAX) {   // at most one atomic per wave: a decimal was met, the refinement has work
    if (__any(dec_seen) && lane == 0) atomicOr(reinterpret_cast<unsigned long long*>(a.mm_dec_seen), 1ull);
  }
}

template <bool LDS> __global__ __launch_bounds__(kAggBlock) void agg_accum_kernel(const AggArgs a) { agg_accum_rows<LDS, false>(a); }
template <bool LDS> __global__ __launch_bounds__(kAggBlock) void agg_accum_expr_kernel(const AggArgs a) { agg_accum_rows<LDS, true>(a); }
template <bool LDS> __global__ __launch_bounds__(kAggBlock) void agg_accum_lex_kernel(const AggArgs a) { agg_accum_rows<LDS, true, true>(a); }   // a.exprs == 2: a program holds an op with kOpExtended (expr_ops.hpp)

// .. and with a MIN / MAX among the aggregates (a.minmax): kernels of their own, so that a node without one launches what it always did
template <bool LDS> __global__ __launch_bounds__(kAggBlock) void agg_accum_minmax_kernel(const AggArgs a) { agg_accum_rows<LDS, false, false, true>(a); }
template <bool LDS> __global__ __launch_bounds__(kAggBlock) void agg_accum_minmax_expr_kernel(const AggArgs a) { agg_accum_rows<LDS, true, false, true>(a); }
template <bool LDS> __global__ __launch_bounds__(kAggBlock) void agg_accum_minmax_lex_kernel(const AggArgs a) { agg_accum_rows<LDS, true, true, true>(a); }

// The refinement of MIN / MAX over decimals: pass 2 settled the high word of every group's decimal candidate; among the rows whose high
// word is that one, the largest low-word key is the candidate's low word.  HBM atomics after the same run merging.  A node whose MIN /
// MAX inputs held no decimal leaves on the device word pass 2 would have set.
template <bool EXPR, bool LEX>
__global__ __launch_bounds__(kAggBlock) void agg_minmax_refine_kernel(const AggArgs a) {
  if (*a.mm_dec_seen == 0) return;
  const u32 tid = threadIdx.x, lane = tid & 63;
  const u64 n = live_rows(a.n_dev, a.cap);
  for (u64 base = (u64)blockIdx.x * kAggBlock; base < n; base += (u64)gridDim.x * kAggBlock) {
    const u64 row = base + tid;
    const bool valid = row < n;
    const u32 g = agg_group(a, row, valid);
    const AggRun r = agg_run(g, valid, lane);
    for (u32 i = 0; i < a.n_aggs; i++) {
      const u32 fn = a.fn[i];
      if (!agg_is_minmax(fn)) continue;
      const u64 w = agg_word0(a, i, valid ? g : 0u);
      const Val v = agg_input<EXPR, LEX>(a, i, agg_input_id<EXPR>(a, i, row, valid), row, valid);
      const bool mn = fn == RDFGPU_AGG_MIN;
      const bool dec = valid && v.tag == RDFGPU_TV_DECIMAL;
      const u64 hi = mn ? ~mm_key_i64(v.hi) : mm_key_i64(v.hi);
      const bool won = dec && a.acc[agg_word(a, w, kMmDecHi)] == hi;
      acc_max(a.acc, agg_word(a, w, kMmDecLo), won ? (mn ? ~(u64)v.lo : (u64)v.lo) : 0ull, r);
    }
  }
}

// ---- pass 3 ---------------------------------------------------------------------------------------------------------------------
// 256-bit two's complement, enough for sum(limb_i * 2^(32 i)) over 2^32 rows and for the integer part scaled by 10^18.
struct Wide { u64 w[4]; };
__device__ __forceinline__ void wide_add(Wide& x, const Wide& y) {
  u64 carry = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) { const u128_t s = (u128_t)x.w[i] + y.w[i] + carry; x.w[i] = (u64)s; carry = (u64)(s >> 64); }
}
__device__ __forceinline__ Wide wide_shifted(u64 v, u32 bits) {   // v << bits, bits a multiple of 32 below 192
  Wide r{{0, 0, 0, 0}};
  const u32 word = bits / 64, b = bits % 64;
  r.w[word] = v << b;
  if (b && word + 1 < 4) r.w[word + 1] = v >> (64 - b);
  return r;
}
__device__ __forceinline__ Wide wide_neg(Wide x) {
#pragma unroll
  for (int i = 0; i < 4; i++) x.w[i] = ~x.w[i];
  wide_add(x, Wide{{1, 0, 0, 0}});
  return x;
}
__device__ __forceinline__ void wide_mul(Wide& x, u64 m) {   // modulo 2^256: exact for the signed values here
  u64 carry = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) { const u128_t p = (u128_t)x.w[i] * m + carry; x.w[i] = (u64)p; carry = (u64)(p >> 64); }
}
__device__ __forceinline__ bool wide_fits(const Wide& x, int words) {   // fits a signed integer of `words` 64-bit words
  const u64 ext = (x.w[words - 1] >> 63) ? ~0ull : 0ull;
  for (int i = words; i < 4; i++) if (x.w[i] != ext) return false;
  return true;
}

__device__ __forceinline__ void put(rdfgpu_agg_value* o, u32 g, u8 tag, long long lo, long long hi) {
  long long* p = reinterpret_cast<long long*>(o + g);
  p[0] = lo; p[1] = hi; p[2] = (long long)tag;   // (tag, reserved bytes = 0)
}

// MIN / MAX of one group (rule 4 of include/rdfgpu.h): the up-to-five candidates are rebuilt from the key words; a candidate is beaten
// if another is strictly less (MIN) / greater (MAX) under tv_partial_cmp, the comparison of the FILTER VM's LT / GT; the result is the
// unbeaten candidate of the lowest kind.  NaN candidates (a kind whose values were all NaN) take part only if there is no other.
__device__ __noinline__ int mm_cmp(const Val& x, const Val& y) { return tv_partial_cmp(x, y); }
__device__ __forceinline__ void minmax_final(const AggArgs& a, u32 i, u32 g, u64 rows) {
  const bool mn = a.fn[i] == RDFGPU_AGG_MIN;
  rdfgpu_agg_value* o = a.out[i];
  const unsigned long long* w = a.acc + agg_word0(a, i, g);
  auto word = [&](u32 k) { return w[agg_word(a, 0, k)]; };
  const u32 flags = (u32)word(kMmFlags);
  if (flags & kMmOther) { if (a.tt.rt_error) atomicOr(a.tt.rt_error, kRtMinMaxKind); put(o, g, RDFGPU_TV_NULL, 0, 0); return; }   // rule 3: the execute fails
  if (rows == 0 || (flags & kMmError)) { put(o, g, RDFGPU_TV_NULL, 0, 0); return; }                                                // rules 1 and 2
  const u8 tags[kMmKinds] = {RDFGPU_TV_INT, RDFGPU_TV_INTEGER, RDFGPU_TV_DECIMAL, RDFGPU_TV_FLOAT, RDFGPU_TV_DOUBLE};
  Val c[kMmKinds];
  u32 have = flags & ((kMmSeen0 << kMmKinds) - 1u);
  for (u32 q = 0; q < kMmKinds; q++) {
    c[q] = val_tv_null();
    if (!(have >> q & 1u)) continue;
    u64 k = word(kMmKey0 + q);
    if (mn) k = ~k;
    c[q].tag = tags[q];
    if (q == kMmFloat) c[q].lo = (int64_t)(u64)mm_unkey_f32(k);
    else if (q == kMmDouble) c[q].lo = (int64_t)mm_unkey_f64(k);
    else if (q == kMmDecKind) { const u64 lo = word(kMmDecLo); c[q].hi = (int64_t)(k ^ (1ull << 63)); c[q].lo = (int64_t)(mn ? ~lo : lo); }
    else c[q].lo = (int64_t)(k ^ (1ull << 63));
  }
  if (have == 0) {   // every value a NaN: the lowest kind's
    if (flags & kMmNanFloat) put(o, g, RDFGPU_TV_FLOAT, 0x7FC00000ll, 0); else put(o, g, RDFGPU_TV_DOUBLE, 0x7FF8000000000000ll, 0);
    return;
  }
  const int beats = mn ? -1 : 1;
  for (u32 q = 0; q < kMmKinds; q++) {
    if (!(have >> q & 1u)) continue;
    bool beaten = false;
    for (u32 p = 0; p < kMmKinds; p++) if (p != q && (have >> p & 1u) && mm_cmp(c[p], c[q]) == beats) beaten = true;
    if (!beaten) { put(o, g, c[q].tag, c[q].lo, c[q].hi); return; }
  }
  put(o, g, RDFGPU_TV_NULL, 0, 0);   // (unreachable: the exact extremum's candidate is unbeaten)
}

__global__ __launch_bounds__(kAggBlock) void agg_final_kernel(const AggArgs a) {
  const u32 g = blockIdx.x * kAggBlock + threadIdx.x;
  if (g >= a.n_groups) return;
  if (a.n_keys) {
    const u32 rep = a.rep_row[g];
    for (u32 q = 0; q < a.n_keys; q++) a.out_key[q][g] = a.key[q][rep];
  }
  const u64 rows = a.acc[g];
  for (u32 i = 0; i < a.n_aggs; i++) {
    const u32 fn = a.fn[i];
    rdfgpu_agg_value* o = a.out[i];
    if (fn == RDFGPU_AGG_COUNT_STAR) { put(o, g, RDFGPU_TV_INTEGER, (long long)rows, 0); continue; }
    const unsigned long long* w = a.acc + agg_word0(a, i, g);
    auto word = [&](u32 k) { return w[agg_word(a, 0, k)]; };
    if (fn == RDFGPU_AGG_COUNT || fn == RDFGPU_AGG_COUNT_DISTINCT) { put(o, g, RDFGPU_TV_INTEGER, (long long)w[0], 0); continue; }
    if (agg_is_minmax(fn)) continue;   // agg_minmax_final_kernel's
    // SUM / AVG (sum.rs, avg.rs).  The arithmetic stays in this kernel's loop: as a function beside minmax_final it cost the kernel 5 % at 2^24 groups.
    const u32 kinds = (u32)word(kSumKinds);
    const bool avg = fn == RDFGPU_AGG_AVG;
    if (avg && rows == 0) { put(o, g, RDFGPU_TV_INTEGER, 0, 0); continue; }                   // avg.rs: count 0 => integer 0
    if (avg && (kinds & kKindOther)) { put(o, g, RDFGPU_TV_NULL, 0, 0); continue; }            // avg.rs:63-78
    const double f64 = __longlong_as_double((long long)word(kSumF64));
    const double f32s = __longlong_as_double((long long)word(kSumF32));
    if (kinds & kKindDouble) {
      const double v = avg ? __ddiv_rn(f64, (double)rows) : f64;
      put(o, g, RDFGPU_TV_DOUBLE, __double_as_longlong(v), 0); continue;
    }
    if (kinds & kKindFloat) {
      const float s = (float)f32s;
      const float v = avg ? __fdiv_rn(s, (float)rows) : s;
      put(o, g, RDFGPU_TV_FLOAT, (long long)(u64)__float_as_uint(v), 0); continue;
    }
    // exact integer part I = L0 + L1 * 2^32 - negatives * 2^64
    Wide I = wide_shifted(word(kSumIntLo), 0);
    wide_add(I, wide_shifted(word(kSumIntHi), 32));
    wide_add(I, wide_neg(wide_shifted(word(kSumIntNeg), 64)));
    if (!avg && !(kinds & kKindDec)) {   // sum.rs: starts as integer 0, integers only
      if (wide_fits(I, 1)) put(o, g, RDFGPU_TV_INTEGER, (long long)I.w[0], 0); else put(o, g, RDFGPU_TV_NULL, 0, 0);
      continue;
    }
    // decimal: D = sum(limb_i * 2^(32 i)) - negatives * 2^128, plus I * 10^18
    Wide D = wide_shifted(word(kSumDec0), 0);
    wide_add(D, wide_shifted(word(kSumDec1), 32));
    wide_add(D, wide_shifted(word(kSumDec2), 64));
    wide_add(D, wide_shifted(word(kSumDec3), 96));
    wide_add(D, wide_neg(wide_shifted(word(kSumDecNeg), 128)));
    wide_mul(I, 1000000000000000000ull);
    wide_add(D, I);
    if (!wide_fits(D, 2)) { put(o, g, RDFGPU_TV_NULL, 0, 0); continue; }
    i128_t sum = (i128_t)(((u128_t)D.w[1] << 64) | (u128_t)D.w[0]);
    // Decimal::checked_div(sum, Decimal::from(count)), expr_device.hpp (count > 0; count * 10^18 is below 2^92)
    if (avg && !dec_checked_div(sum, (i128_t)rows * (i128_t)kDecOne, sum)) { put(o, g, RDFGPU_TV_NULL, 0, 0); continue; }
    put(o, g, RDFGPU_TV_DECIMAL, (long long)(u64)(u128_t)sum, (long long)(u64)((u128_t)sum >> 64));
  }
}

// The MIN / MAX of every group, one lane per group like agg_final_kernel and launched beside it for the nodes that have one (a.minmax):
// the five candidates and their comparisons stay out of the kernel that every other node runs.
__global__ __launch_bounds__(kAggBlock) void agg_minmax_final_kernel(const AggArgs a) {
  const u32 g = blockIdx.x * kAggBlock + threadIdx.x;
  if (g >= a.n_groups) return;
  const u64 rows = a.acc[g];
  for (u32 i = 0; i < a.n_aggs; i++)
    if (agg_is_minmax(a.fn[i])) minmax_final(a, i, g, rows);
}

// ---- pass 4, aggregate values as columns (RDFGPU_PLAN_AGG_COLUMNS) only ------------------------------------------------------------
// One lane per group: row g's entry of every aggregate's value column is g + 1, or 0 where the value is the error value (an unbound
// binding).  A pass of its own, 4 bytes written per group and aggregate: agg_final_kernel stays what it is for the plans without the flag.
__global__ __launch_bounds__(kAggBlock) void agg_value_cols_kernel(const AggArgs a) {
  const u32 g = blockIdx.x * kAggBlock + threadIdx.x;
  if (g >= a.n_groups) return;
  for (u32 i = 0; i < a.n_aggs; i++) a.out_val[i][g] = a.out[i][g].tag == RDFGPU_TV_NULL ? 0u : g + 1u;
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
using AggKernel = void (*)(const AggArgs);
// The accumulate kernels by [a.minmax][a.exprs][a.lds], the refinement's by [a.exprs]  (plan.hpp, agg_accum_class: the class reported for the same fields).
static const AggKernel kAggAccumKernels[2][3][2] = {
    {{agg_accum_kernel<false>, agg_accum_kernel<true>}, {agg_accum_expr_kernel<false>, agg_accum_expr_kernel<true>}, {agg_accum_lex_kernel<false>, agg_accum_lex_kernel<true>}},
    {{agg_accum_minmax_kernel<false>, agg_accum_minmax_kernel<true>}, {agg_accum_minmax_expr_kernel<false>, agg_accum_minmax_expr_kernel<true>},
     {agg_accum_minmax_lex_kernel<false>, agg_accum_minmax_lex_kernel<true>}}};
static const AggKernel kAggRefineKernels[3] = {agg_minmax_refine_kernel<false, false>, agg_minmax_refine_kernel<true, false>, agg_minmax_refine_kernel<true, true>};

static void agg_launch(AggKernel kernel, u64 grid, size_t lds, const AggArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)(grid ? grid : 1)), dim3(kAggBlock), lds, s, a);
  RDFGPU_HIP(hipGetLastError());
}
void launch_agg_groups_wide(const AggWideArgs& w, hipStream_t s) {
  const u64 grid = std::min<u64>((w.cap + kAggTile - 1) / kAggTile, kAggGroupGrid);
  hipLaunchKernelGGL(agg_groups_wide_kernel, dim3((unsigned)(grid ? grid : 1)), dim3(kAggBlock), 0, s, w);
  RDFGPU_HIP(hipGetLastError());
}
void launch_agg_wide_keys(const AggWideArgs& w, hipStream_t s) {
  const u64 grid = ((u64)w.n_groups + kAggBlock - 1) / kAggBlock;
  hipLaunchKernelGGL(agg_wide_keys_kernel, dim3((unsigned)(grid ? grid : 1)), dim3(kAggBlock), 0, s, w);
  RDFGPU_HIP(hipGetLastError());
}
void launch_agg_groups(const AggArgs& a, hipStream_t s) { agg_launch(agg_groups_kernel, std::min<u64>((a.cap + kAggTile - 1) / kAggTile, kAggGroupGrid), 0, a, s); }
void launch_agg_accum(const AggArgs& a, hipStream_t s) {
  const size_t lds = a.lds ? (size_t)a.n_words * a.n_groups * sizeof(unsigned long long) : 0;
  if (lds > kAggLdsBytes) fail(RDFGPU_ERR_INVALID, "aggregate: %zu bytes of LDS partials", lds);
  const u64 grid = std::min<u64>((a.cap + kAggBlock - 1) / kAggBlock, a.lds ? kAggAccumLdsGrid : kAggAccumHbmGrid);
  agg_launch(kAggAccumKernels[a.minmax ? 1 : 0][std::min(a.exprs, 2u)][a.lds ? 1 : 0], grid, lds, a, s);
}
void launch_agg_minmax_refine(const AggArgs& a, hipStream_t s) { agg_launch(kAggRefineKernels[std::min(a.exprs, 2u)], std::min<u64>((a.cap + kAggBlock - 1) / kAggBlock, kAggAccumHbmGrid), 0, a, s); }
void launch_agg_final(const AggArgs& a, hipStream_t s) {
  const u64 grid = ((u64)a.n_groups + kAggBlock - 1) / kAggBlock;
  agg_launch(agg_final_kernel, grid, 0, a, s);
  if (a.minmax) agg_launch(agg_minmax_final_kernel, grid, 0, a, s);
}
void launch_agg_value_cols(const AggArgs& a, hipStream_t s) { agg_launch(agg_value_cols_kernel, ((u64)a.n_groups + kAggBlock - 1) / kAggBlock, 0, a, s); }

// (kernels.hpp, preload_code_objects: the runtime loads a translation unit's code object at the first use of one of its kernels)
void preload_tu_aggregate() { hipFuncAttributes at; RDFGPU_HIP(hipFuncGetAttributes(&at, reinterpret_cast<const void*>(agg_final_kernel))); }

}  // namespace rdfgpu
