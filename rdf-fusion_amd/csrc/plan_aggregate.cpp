// plan_aggregate.cpp — AggregateExec(mode=Single) (RDFGPU_NODE_AGGREGATE; kernels: aggregate.hip) as named steps over one AggNode
// (plan.hpp): bind the inputs, lay out the accumulator words, group pass, allocate the outputs, accumulate, finish.
#include "plan_exec.hpp"

namespace rdfgpu {

// An expression input's program goes to the device: the VM form of the accumulate pass, over every input column.
void Plan::agg_bind_inputs(AggNode& n) {
  AggArgs& a = n.a;
  const NodeInfo& nd = n.nd;
  // The wide form (RDFGPU_PLAN_VALUE_KEYS): a value column among the group columns, or more than RDFGPU_MAX_KEYS of them.  Every other node is
  // bound, and launches, exactly as before.  AggArgs then carries the first four keys only (agg_final_kernel's copy); `w` carries them all.
  const u32 nk = nd.d.n_keys;
  n.wide = value_keys && nk > RDFGPU_MAX_KEYS;
  for (u32 k = 0; k < nk && value_keys; k++) n.wide = n.wide || nd.origin[k].node >= 0;
  a.n_keys = std::min<u32>(nk, RDFGPU_MAX_KEYS);
  for (u32 k = 0; k < a.n_keys; k++) a.key[k] = n.in.cols[agg_key_col(nd.d, k)];
  if (n.wide) {
    AggWideArgs& w = n.w;
    w.n_keys = nk; w.n_dev = n.in.n_dev; w.cap = n.in.cap;
    for (u32 k = 0; k < nk; k++) {
      w.key[k] = n.in.cols[agg_key_col(nd.d, k)];
      const ValueOrigin& o = nd.origin[k];
      if (o.node < 0) continue;
      const NodeInfo& src = nodes[o.node];   // the arrays are scratch of the execution that wrote them (bind_values)
      if (src.values_run != run) fail(RDFGPU_ERR_INVALID, "a value column of node %d is grouped by before the node ran", o.node);
      w.value_mask |= 1u << k; w.val[k] = src.values[o.agg]; w.val_n[k] = src.n_values;
      n.group_row_bytes += 24;
    }
  }
  n.group_row_bytes += 4ull * nk;
  a.n_dev = n.in.n_dev; a.cap = n.in.cap; a.n_aggs = nd.n_aggs;
  for (u32 i = 0; i < a.n_aggs; i++) {
    const u32 fn = nd.agg_fn[i];
    a.fn[i] = fn; a.in[i] = fn == RDFGPU_AGG_COUNT_STAR || nd.agg_prog[i] >= 0 ? nullptr : n.in.cols[nd.agg_col[i]];
    if (agg_is_minmax(fn)) a.minmax = 1;
    if (nd.agg_prog[i] < 0) continue;
    a.prog[i] = upload_program(nd.agg_progs[nd.agg_prog[i]]);
    a.exprs = a.exprs == 2 || program_has_lex(nd.agg_progs[nd.agg_prog[i]]) ? 2 : 1;
    for (u32 c = 0; c < n.in.n_cols; c++) a.col[c] = n.in.cols[c];
  }
  a.tt = typed_table();
  while (n.slots < 2 * a.cap && n.slots < (1ull << 32)) n.slots <<= 1;
}

// Word 0 counts the group's rows; behind it every aggregate's words as kernels.hpp states them.  A row costs 4 bytes per id read, 16 more per typed value.
static void agg_layout_words(AggNode& n) {
  AggArgs& a = n.a;
  a.n_words = 1; a.word_op[0] = kAggAdd;
  for (u32 i = 0; i < a.n_aggs; i++) {
    const u32 fn = a.fn[i], words = agg_words(fn);
    a.word0[i] = a.n_words;
    for (u32 w = 0; w < words; w++) a.word_op[a.n_words++] = agg_word_op(fn, w);
    n.accum_row_bytes += fn == RDFGPU_AGG_COUNT_STAR ? 0 : agg_is_sum(fn) || agg_is_minmax(fn) ? 20 : 4;
    if (agg_is_minmax(fn)) n.refine_row_bytes += 20;
  }
}

// The one read-back: the group count sizes the accumulators and is the output's row count.  Zero keys: one group and no group pass.
void Plan::agg_group_pass(AggNode& n) {
  AggArgs& a = n.a;
  if (a.n_keys) n.G = 0;
  if (a.n_keys && a.cap) {
    a.slots = scratch<u32>(n.slots); a.slot_mask = (u32)(n.slots - 1);
    a.row_slot = scratch<u32>(a.cap); a.slot_gid = scratch<u32>(n.slots); a.rep_row = scratch<u32>(a.cap);
    a.n_groups_dev = new_counter();
    RDFGPU_HIP(hipMemsetAsync(a.slots, 0, n.slots * sizeof(u32), stream));
    if (n.wide) {   // per row 4 bytes per key column and the 24-byte record of every value key
      AggWideArgs& w = n.w;
      w.slots = a.slots; w.slot_mask = a.slot_mask; w.row_slot = a.row_slot; w.slot_gid = a.slot_gid; w.rep_row = a.rep_row; w.n_groups_dev = a.n_groups_dev;
      timed(KC_AGG_GROUPS_WIDE, 0, a.cap, a.n_dev, n.group_row_bytes, nullptr, 0, 0, [&] { launch_agg_groups_wide(w, stream); });
    } else
    timed(KC_AGG_GROUPS, 0, a.cap, a.n_dev, 4ull * a.n_keys, nullptr, 0, 0, [&] { launch_agg_groups(a, stream); });
    n.G = read_back<u64>(a.n_groups_dev);
  }
  a.n_groups = (u32)n.G;
}

// The output: the keys; with aggregate values as columns, one more per aggregate.  The value arrays are the node's, of this execution.
DevTable Plan::agg_outputs(AggNode& n) {
  AggArgs& a = n.a;
  DevTable t; t.n_cols = n.nd.width; t.cap = n.G;
  const u32 nk = n.nd.d.n_keys;   // (a.n_keys is the first four of them in the wide form)
  for (u32 k = 0; k < nk; k++) {
    u32* const c = scratch<u32>(n.G);
    t.cols[k] = c;
    if (k < a.n_keys) a.out_key[k] = c;
    if (n.wide) n.w.out_key[k] = c;
  }
  n.w.n_groups = (u32)n.G;
  for (u32 i = 0; i < a.n_aggs; i++) {
    a.out[i] = scratch<rdfgpu_agg_value>(n.G); n.nd.values[i] = a.out[i];
    if (agg_columns) { a.out_val[i] = scratch<u32>(n.G); t.cols[nk + i] = a.out_val[i]; }
  }
  n.nd.n_values = n.G; n.nd.values_run = run;
  if (&n.nd == &nodes[root] && !agg_columns) agg_out.assign(a.out, a.out + a.n_aggs);
  return t;
}

// Zeroed accumulators (and COUNT DISTINCT sets); LDS partials when all words fit; no read-back decides the refinement's launch (it leaves on a device word).
void Plan::agg_accumulate(AggNode& n) {
  AggArgs& a = n.a;
  a.acc = scratch<unsigned long long>(a.n_words * n.G);
  RDFGPU_HIP(hipMemsetAsync(a.acc, 0, a.n_words * n.G * sizeof(unsigned long long), stream));
  if (!a.cap) return;
  for (u32 i = 0; i < a.n_aggs; i++) {
    if (a.fn[i] != RDFGPU_AGG_COUNT_DISTINCT) continue;
    a.dset[i] = scratch<unsigned long long>(n.slots); a.dset_mask = (u32)(n.slots - 1);
    RDFGPU_HIP(hipMemsetAsync(a.dset[i], 0, n.slots * sizeof(unsigned long long), stream));
  }
  a.lds = !opt.on(RDFGPU_OPT_NO_AGG_LDS) && (u64)a.n_words * n.G * sizeof(unsigned long long) <= kAggLdsBytes;
  if (a.minmax) a.mm_dec_seen = new_counter();   // (zeroed with the other counters when the execution began)
  timed(agg_accum_class(a), 0, a.cap, a.n_dev, n.accum_row_bytes, nullptr, 0, 0, [&] { launch_agg_accum(a, stream); });
  if (a.minmax) timed(KC_AGG_MINMAX_REFINE, 0, a.cap, a.n_dev, n.refine_row_bytes, nullptr, 0, 0, [&] { launch_agg_minmax_refine(a, stream); });
}

// The value columns: per group and aggregate the tag read (the value was just written: cache) and 4 bytes written.
void Plan::agg_finish(AggNode& n) {
  const AggArgs& a = n.a;
  timed(KC_AGG_FINAL, 0, 0, nullptr, 0, nullptr, n.G, 4ull * a.n_keys + 24ull * a.n_aggs, [&] { launch_agg_final(a, stream); });
  if (n.wide && n.w.n_keys > RDFGPU_MAX_KEYS) timed(KC_AGG_WIDE_KEYS, 0, 0, nullptr, 0, nullptr, n.G, 4ull * (n.w.n_keys - RDFGPU_MAX_KEYS), [&] { launch_agg_wide_keys(n.w, stream); });
  if (agg_columns && a.n_aggs) timed(KC_AGG_VALUE_COLS, 0, 0, nullptr, 0, nullptr, n.G, 4ull * a.n_aggs, [&] { launch_agg_value_cols(a, stream); });
}

// AggregateExec.  Compulsory bytes: per input row 4 per key column, 4 + 16 per SUM / AVG / MIN / MAX input (id + typed
// value), 4 per COUNT / COUNT DISTINCT input; per output group 4 per key column + 24 per aggregate.  A MIN / MAX input is read once more
// by the refinement launch (agg_minmax_refine_kernel), which is counted as if decimals were there: 4 + 16 per row again.
DevTable Plan::exec_aggregate(NodeInfo& nd) {
  const DevTable in = exec_sub_plan((u32)nd.d.left);
  flush_pending_oj();   // a held-back ordered-join write must have happened before the input is read
  if (in.cap >= (1ull << 32)) fail(RDFGPU_ERR_UNSUPPORTED, "AggregateExec over %llu rows (at most 2^32 - 1)", (unsigned long long)in.cap);
  AggNode n(nd, in);
  agg_bind_inputs(n);
  agg_layout_words(n);
  agg_group_pass(n);
  const DevTable t = agg_outputs(n);
  if (n.G == 0) return t;
  agg_accumulate(n);
  agg_finish(n);
  return t;
}

}  // namespace rdfgpu
