// plan_sort.cpp — SortExec (RDFGPU_NODE_SORT; kernels: sort.hip) as named steps over one SortRun: bind the keys, write the records, sort
// the tiles, merge the runs, gather the output.  Everything is enqueued on the plan's stream; the input's row count may live on the device
// only and nothing here waits for it: launch geometry comes from the capacity, scratch from the plan's arena.
#include "plan_exec.hpp"

namespace rdfgpu {

namespace {
// One SortExec while it is set up and run.
struct SortRun {
  const NodeInfo& nd; const DevTable& in;
  SortArgs a{};
  u64 out_cap = 0;            // rows of the output, at most
  u32 passes = 0;             // merge passes: the final run is run[passes & 1]
  u64 key_row_bytes = 0;      // what the record pass reads per row: 4 per key column, 16 per typed-value gather, 24 per value
  SortRun(const NodeInfo& n, const DevTable& t) : nd(n), in(t) {}
};
}  // namespace

// The keys as the kernels take them; a key by value gets the array its column's entries index, of this execution (the node that owns it
// has run: it is below).
static void sort_bind_keys(const Plan& plan, SortRun& s) {
  SortArgs& a = s.a;
  const NodeInfo& child = plan.nodes[(u32)s.nd.d.left];
  for (u32 c = 0; c < s.in.n_cols; c++) a.in[c] = s.in.cols[c];
  a.n_in_dev = s.in.n_dev; a.n_in_cap = s.in.cap;
  a.n_keys = s.nd.d.n_keys;
  a.words = s.nd.sort_words;
  a.fetch = s.nd.d.table_cols;
  for (u32 k = 0; k < a.n_keys; k++) {
    a.key_col[k] = s.nd.d.left_keys[k];
    a.key_how[k] = s.nd.d.right_keys[k] & ~RDFGPU_SORT_DESC;
    a.key_desc[k] = (s.nd.d.right_keys[k] & RDFGPU_SORT_DESC) ? 1u : 0u;
    s.key_row_bytes += 4;
    if (a.key_how[k] == RDFGPU_SORT_BY_TERM || a.key_how[k] == RDFGPU_SORT_BY_DOUBLE) s.key_row_bytes += 16;
    if (a.key_how[k] != RDFGPU_SORT_BY_VALUE) continue;
    const ValueOrigin& o = child.origin[a.key_col[k]];
    if (o.node < 0 || plan.nodes[o.node].values_run != plan.run) fail(RDFGPU_ERR_INVALID, "SortExec: the value column of key %u is read before the node that computes it ran", k);
    a.key_values[k] = plan.nodes[o.node].values[o.agg];
    a.key_n_values[k] = plan.nodes[o.node].n_values;
    s.key_row_bytes += 24;
  }
  a.n_out_cols = s.nd.n_proj;
  for (u32 c = 0; c < s.nd.n_proj; c++) a.proj[c] = s.nd.proj[c];
  s.passes = sort_merge_passes(s.in.cap);
  s.out_cap = a.fetch && a.fetch < s.in.cap ? a.fetch : s.in.cap;
}

// SortExec.  Compulsory bytes: the record pass reads a row's key entries (and what they point to) and writes 8 * words; the
// tile sort reads the records and writes 4 per kept row; a merge pass reads, per row it writes, the row index and its record's key words
// and writes 4; the gather reads 4 + 4 per output column and writes 4 per output column, per output row.
DevTable Plan::exec_sort(NodeInfo& nd) {
  const DevTable in = exec_sub_plan((u32)nd.d.left);
  flush_pending_oj();   // a held-back ordered-join write must have happened before the input is read
  DevTable t;
  t.n_cols = nd.n_proj;
  if (in.cap == 0) { t.cap = 0; return t; }
  if (in.cap >= 0xFFFFFFFFull) fail(RDFGPU_ERR_UNSUPPORTED, "SortExec over %llu rows (fewer than 2^32 - 1)", (unsigned long long)in.cap);
  SortRun s(nd, in);
  sort_bind_keys(*this, s);
  SortArgs& a = s.a;
  a.tt = typed_table();
  a.rec = scratch<u64>(in.cap * a.words);
  a.run[0] = scratch<u32>(in.cap);
  a.run[1] = s.passes ? scratch<u32>(in.cap) : nullptr;
  for (u32 c = 0; c < nd.n_proj; c++) { a.out[c] = scratch<u32>(s.out_cap); t.cols[c] = a.out[c]; }
  a.n_out_dev = in.n_dev ? new_counter() : nullptr;   // (a count known on the host stays known: min(rows, fetch))

  const u64 key_bytes = 8ull * (a.words - 1);
  timed(KC_SORT_KEYS, 0, in.cap, in.n_dev, s.key_row_bytes + 8ull * a.words, nullptr, 0, 0, [&] { launch_sort_keys(a, stream); });
  timed(KC_SORT_TILE, 0, in.cap, in.n_dev, 8ull * a.words + 4, nullptr, 0, 0, [&] { launch_sort_tile(a, stream); });
  for (u32 p = 0; p < s.passes; p++) {
    // rows this pass writes, at most: every pair's two runs, each cut to the fetch
    const u64 S = (u64)kSortTile << p, pairs = ((in.cap + S - 1) / S + 1) / 2;
    const u64 rows = a.fetch ? std::min<u64>(in.cap, pairs * std::min<u64>(2 * S, a.fetch)) : in.cap;
    timed(KC_SORT_MERGE, 0, rows, a.fetch ? nullptr : in.n_dev, 8 + key_bytes, nullptr, 0, 0, [&] { launch_sort_merge(a, p, stream); });
  }
  timed(KC_SORT_GATHER, 0, 0, nullptr, 0, a.n_out_dev, a.n_out_dev ? 0 : s.out_cap, 4 + 8ull * nd.n_proj, [&] { launch_sort_gather(a, s.passes & 1u, s.out_cap, stream); });
  t.cap = s.out_cap; t.n_dev = a.n_out_dev;
  return t;
}

}  // namespace rdfgpu
