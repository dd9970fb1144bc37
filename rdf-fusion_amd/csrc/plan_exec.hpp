// plan_exec.hpp — what the plan*.cpp units share beyond plan.hpp: the member templates of Plan and a few inline helpers.
// Private to those units (abi.cpp sees plan.hpp only).
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <shared_mutex>

#include "plan.hpp"

namespace rdfgpu {

// whether a node of this kind has a right input
inline bool is_binary(u32 kind) {
  return kind == RDFGPU_NODE_HASH_JOIN || kind == RDFGPU_NODE_CROSS_JOIN || kind == RDFGPU_NODE_NESTED_LOOP_JOIN || kind == RDFGPU_NODE_UNION;
}

// The columns a program reads, as a bit set (a program addresses at most 2 * kMaxCols = 32 columns: a join's two sides).
inline u32 columns_read(const ExprProgram& p) {
  static_assert(2 * kMaxCols <= 32, "one bit per column of a join's two sides");
  u32 cols = 0;
  for (u32 i = 0; i < p.n; i++) if (p.nodes[i].op == RDFGPU_EX_COLUMN) cols |= 1u << p.nodes[i].u;
  return cols;
}

// The output columns of `nd` selected from its input `in`, zero-copy: a ProjectionExec, or an operator that keeps every row.
inline DevTable project(const DevTable& in, const NodeInfo& nd) {
  DevTable t;
  t.n_cols = nd.n_proj; t.cap = in.cap; t.n_dev = in.n_dev;
  for (u32 c = 0; c < nd.n_proj; c++) t.cols[c] = in.cols[nd.proj[c]];
  return t;
}

// whether column `c` of a join's [left cols, right cols] schema belongs to its build side
inline bool on_build_side(const LdsJoinArgs& a, u32 c) { return (c < a.n_left_cols) == (a.build_is_left != 0); }

// The literal, arithmetic and comparison of one half of the window shape (detect_join_filter_shape 3) that starts at node `o`.
inline TvLiteral window_literal(const rdfgpu_expr_node* e, u32 o) {
  TvLiteral l{};
  l.lo = e[o + 4].lo; l.hi = e[o + 4].hi; l.aux = e[o + 4].u; l.tag = e[o + 4].tag; l.flags = e[o + 4].flags;
  l.arith_sub = e[o + 5].op == RDFGPU_EX_SUB; l.cmp_op = e[o + 6].op;
  return l;
}

// which scan an n-element scan of counts takes (kernels.hip: one workgroup up to kSmallScanElems elements, rocPRIM's device scan beyond)
inline int scan_class(u64 n) { return n <= kSmallScanElems ? KC_SMALL_SCAN : KC_DEVICE_SCAN; }

// brackets one launch with HIP events when timing is on (the durations and bytes: Plan::resolve_timing, plan.cpp)
template <class F>
void Plan::timed(int kc, u64 fixed_bytes, u64 rows_cap, const u64* rows_dev, u64 bytes_per_row,
                 const u64* out_dev, u64 out_rows, u64 bytes_per_out, F&& launch) {
  metrics.kernels_launched++;
  if (!timing || (timing_focus >= 0 && kc != timing_focus)) { launch(); return; }
  PendingLaunch p{kc, ctx->event(events_used), ctx->event(events_used + 1), fixed_bytes, rows_cap, rows_dev, bytes_per_row, out_dev, out_rows, bytes_per_out};
  events_used += 2;
  RDFGPU_HIP(hipEventRecord(p.start, stream));
  launch();
  RDFGPU_HIP(hipEventRecord(p.stop, stream));
  pending.push_back(p);
}

// device memory of the current execution, from the store's pool (handed back by Plan::release_intermediates)
// Behind a pending tail (Plan::retired is not empty) the predecessor's blocks are served first, by the pool's own rule over both sets: an exact fit among the
// retired blocks or the pool's cached ones, then the smallest retired block that is not wastefully large, then the pool (which allocates only if it has none either).
template <class T> T* Plan::scratch(u64 n) {
  const size_t bytes = (n ? n : 1) * sizeof(T);
  void* p = nullptr;
  if (!retired.empty()) {
    const size_t b = DevicePool::bucket(bytes);
    p = retired.take_exact(b);
    if (!p) p = store->pool.alloc_exact(bytes);
    if (!p) p = retired.take(b);
  }
  if (!p) p = store->pool.alloc(bytes);
  allocs.push_back(p);
  metrics.device_bytes += (n ? n : 1) * sizeof(T);
  return (T*)p;
}

// {min, max} of the i64 values `launch(slots)` folds into two counter slots, read back in one host round trip.
template <class F> void Plan::device_minmax_i64(long long (&got)[2], F&& launch) {
  long long* mm = reinterpret_cast<long long*>(new_counter()); (void)new_counter();   // {min, max}: two slots
  const long long init[2] = {INT64_MAX, INT64_MIN + 1};
  RDFGPU_HIP(hipMemcpyAsync(mm, init, sizeof init, hipMemcpyHostToDevice, stream));
  launch(mm);
  read_back(got, mm, sizeof got);
}

}  // namespace rdfgpu
