// plan.cpp — execution (device) of a compiled plan: the driver, timing, scans and the small operators.
// Compilation: plan_compile.cpp; FilterExec: plan_filter.cpp; the joins: plan_join.cpp; chain fusion and the band join: plan_band.cpp;
// SortExec: plan_sort.cpp; AggregateExec: plan_aggregate.cpp.
//
// What replaces what (reference paths relative to the rdf-fusion tree):
//   Plan::exec_source       DataSource::open + MemQuadIndexScanIterator::next  pattern_data_source.rs:42-58, scan.rs:104-212
#include "plan_exec.hpp"

#include <functional>

namespace rdfgpu {

// The scan of a pattern from its G,S,P,O instructions: index choice (IndexPermutations::choose_index, permutations.rs:81-96),
// the instructions in that index's order, the pruning levels and what they make redundant, the output columns in G,S,P,O
// order of first binding (patterns/mod.rs:68-107).
void Plan::derive_source(SourceInfo& src, const ScanInstructions& gspo) {
  src.components = choose_index(gspo, 0b111);
  src.ix = reorder(gspo, src.components);
  src.prune = plan_pruning(src.ix);
  src.n_out = 0; src.has_residual = false;
  for (int k = 0; k < 4; k++) {
    if (gspo.in[k].kind != RDFGPU_SCAN) continue;
    bool first = true;
    for (int j = 0; j < k; j++) if (gspo.in[j].kind == RDFGPU_SCAN && gspo.in[j].var == gspo.in[k].var) first = false;
    if (!first) continue;
    for (int lvl = 0; lvl < 4; lvl++)
      if (src.ix.in[lvl].kind == RDFGPU_SCAN && src.ix.in[lvl].var == gspo.in[k].var) src.out_level[src.n_out] = lvl;
    src.n_out++;
  }
  for (int k = 0; k < 4; k++)
    if (src.ix.in[k].pred.kind != RDFGPU_PRED_NONE && !(src.prune.dropped_mask & (1u << k))) src.has_residual = true;
}
// IN sets of residual predicates live on the device: uploaded at compile time and again when push-down changed them
void Plan::upload_pool() {
  pool.clear();
  for (SourceInfo& s : sources)
    for (int k = 0; k < 4; k++)
      if (s.ix.in[k].pred.kind == RDFGPU_PRED_IN && !(s.prune.dropped_mask & (1u << k))) {
        s.ix.in[k].pred.from = (u32)pool.size();
        pool.insert(pool.end(), s.ix.in[k].pred.ids.begin(), s.ix.in[k].pred.ids.end());
      }
  store->activate();
  if (stream) RDFGPU_HIP(hipStreamSynchronize(stream));
  if (pool_dev) { RDFGPU_HIP(hipFree(pool_dev)); pool_dev = nullptr; }
  if (!pool.empty()) {
    RDFGPU_HIP(hipMalloc((void**)&pool_dev, pool.size() * 4));
    RDFGPU_HIP(hipMemcpy(pool_dev, pool.data(), pool.size() * 4, hipMemcpyHostToDevice));
  }
}

namespace {
// MemStoragePredicateExpr -> MemIndexScanPredicate (to_scan_predicate, predicate_pushdown.rs:120-157); false = `true` (no predicate)
bool filter_to_predicate(const rdfgpu_pushdown_filter& f, ScanPredicate* out) {
  if (f.kind == RDFGPU_PUSH_TRUE) return false;
  if (f.kind == RDFGPU_PUSH_BINARY) { *out = pushdown_to_scan_predicate(f.op, f.value); return true; }
  if (f.kind == RDFGPU_PUSH_BETWEEN) {
    ScanPredicate p;
    if (f.from > f.to) p.kind = RDFGPU_PRED_FALSE; else { p.kind = RDFGPU_PRED_BETWEEN; p.from = f.from; p.to = f.to; }
    *out = p; return true;
  }
  fail(RDFGPU_ERR_INVALID, "push-down filter of kind %u", f.kind);
}
// MemIndexScanInstructions::apply_filter (scan_instructions.rs:101-133)
void and_into_instructions(ScanInstructions& gspo, u32 var, const ScanPredicate& p) {
  int at = -1;
  for (int k = 0; k < 4 && at < 0; k++) if (gspo.in[k].kind == RDFGPU_SCAN && gspo.in[k].var == var) at = k;   // instructions_for_column: the first binding
  if (at < 0) fail(RDFGPU_ERR_INVALID, "Could not find scan instruction for column: variable %u", var);
  ScanPredicate combined = p;
  if (gspo.in[at].pred.kind != RDFGPU_PRED_NONE && !predicate_and(gspo.in[at].pred, p, &combined))
    fail(RDFGPU_ERR_INVALID, "Could not apply predicate to scan instruction.");
  gspo.in[at].pred = combined;
}
}  // namespace

void Plan::pushdown_filters(u32 node, const rdfgpu_pushdown_filter* filters, u32 n, u8* pushed) {
  if (node >= nodes.size() || nodes[node].source < 0) fail(RDFGPU_ERR_INVALID, "node %u is not a data source", node);
  SourceInfo& src = sources[nodes[node].source];
  ScanInstructions gspo = src.gspo;
  bool any = false;
  for (u32 i = 0; i < n; i++) {
    const bool yes = filters[i].kind != RDFGPU_PUSH_UNSUPPORTED;   // rewritten => PushedDown::Yes (pattern_data_source.rs:121-127)
    if (pushed) pushed[i] = yes ? 1 : 0;
    if (!yes) continue;
    any = true;
    ScanPredicate p;
    if (filter_to_predicate(filters[i], &p)) and_into_instructions(gspo, filters[i].var, p);
  }
  if (!any) return;                       // "Don't create a new node if no filters were pushed down"
  src.gspo = gspo;
  derive_source(src, src.gspo);           // apply_pushdown_filters ends in try_find_better_index
  src.dynamic_dirty = !src.dynamic.empty();
  upload_pool();
  located_version = ~0ull;                // the cached ranges belong to the old instructions
  for (NodeInfo& nd : nodes) { nd.has_last = false; nd.last_rows = 0; }   // and so do the cardinalities
}

void Plan::set_dynamic_filters(u32 node, const rdfgpu_pushdown_filter* filters, u32 n) {
  if (node >= nodes.size() || nodes[node].source < 0) fail(RDFGPU_ERR_INVALID, "node %u is not a data source", node);
  SourceInfo& src = sources[nodes[node].source];
  std::vector<std::pair<u32, ScanPredicate>> dyn;
  for (u32 i = 0; i < n; i++) {
    if (filters[i].kind == RDFGPU_PUSH_UNSUPPORTED) continue;      // `current_predicate_expr().ok()`: unsupported ones are skipped (scan.rs:246-249)
    ScanPredicate p;
    if (filter_to_predicate(filters[i], &p)) dyn.emplace_back(filters[i].var, p);
  }
  // validate now, against the static instructions, so that execute cannot fail on them
  ScanInstructions probe = src.gspo;
  for (auto& d : dyn) and_into_instructions(probe, d.first, d.second);
  src.dynamic = dyn;
  src.dynamic_dirty = true;
}

Plan::~Plan() {
  if (store) (void)hipSetDevice(store->device);
  try { complete(); } catch (...) {}
  if (stream) (void)hipStreamSynchronize(stream);
  if (store) { store->tails.remove(this); tail_waited(); }   // (whatever complete() could not do)
  release_intermediates();
  if (pool_dev) (void)hipFree(pool_dev);
  if (regex_dev) (void)hipFree(regex_dev);
  if (str_consts_dev) (void)hipFree(str_consts_dev);
  if (mark_values_dev) (void)hipFree(mark_values_dev);

  if (store && ctx) store->release_context(ctx);
  if (store) store->release();
}

// Names as rocprofv3 --kernel-trace prints them (prefix up to the argument list).
const char* kernel_class_name(int kc) {
  static const char* const fixed[KC_LDS_JOIN0] = {
      "rdfgpu::locate_kernel", "rdfgpu::scan_count_kernel", "rdfgpu::scan_write_kernel",
      "void rdfgpu::filter_kernel<1>", "void rdfgpu::filter_kernel<2>", "void rdfgpu::filter_kernel<0>",
      "rdfgpu::cross_kernel", "rdfgpu::join_build_kernel", "void rdfgpu::join_probe_kernel<false>",
      "void rdfgpu::join_probe_kernel<true>", "rdfgpu::join_left_unmatched_kernel", "void rdfgpu::nlj_kernel<false>",
      "void rdfgpu::nlj_kernel<true>", "rocprim device scan", "rdfgpu::gjoin_build_kernel", "rdfgpu::gdirect_build_kernel",
      "rdfgpu::minmax_u32_kernel", "rdfgpu::csr_rel_keys_kernel", "rocprim radix sort (CSR rows)",
      "rdfgpu::topk_max_kernel", "rdfgpu::topk_hist_kernel", "rdfgpu::topk_scatter_kernel", "rdfgpu::topk_select_kernel",
      "rdfgpu::topk_write_kernel", "void rdfgpu::filter_kernel<3>", "rdfgpu::regex_verdict_kernel", "rdfgpu::union_kernel",
      "rdfgpu::band_slow_kernel", "rocprim radix sort", "rdfgpu::band_bounds_kernel", "rdfgpu::band_blocks_kernel",
      "rdfgpu::band_decode_kernel", "void rdfgpu::band_mask_kernel", "void rdfgpu::band_emit_kernel", "rdfgpu::band_entries_kernel",
      "rdfgpu::band_desc_kernel", "rdfgpu::band_pt_kernel", "rdfgpu::band_rows_kernel",
      "void rdfgpu::filter_bits_kernel<1>", "void rdfgpu::filter_bits_kernel<2>", "void rdfgpu::filter_bits_kernel<3>", "void rdfgpu::filter_bits_kernel<4>", "rdfgpu::value_verdict_kernel",
      "rdfgpu::value_runs_kernel", "void rdfgpu::run_scan_kernel", "rdfgpu::run_copy_kernel",
      "rdfgpu::oj_probe_kernel", "rdfgpu::oj_count_kernel", "void rdfgpu::oj_write_kernel",
      "void rdfgpu::filter_write_kernel", "rdfgpu::part_keys_kernel", "void rdfgpu::part_join_kernel",
      "rdfgpu::oj_band_records_kernel", "rdfgpu::oj_write_band_kernel", "void rdfgpu::small_scan_kernel",
      "rdfgpu::part_pass (hist + scan + scatter)", "void rdfgpu::stream_join_kernel",
      "rdfgpu::oj_write_band_kernel(rdfgpu::OrderedJoinArgs, rdfgpu::OjBandFuse, rdfgpu::OjInPlace)", "void rdfgpu::semi_build_kernel",
      "void rdfgpu::semi_join_kernel<0, false", "void rdfgpu::semi_join_kernel<0, true", "void rdfgpu::semi_join_kernel<1, false",
      "void rdfgpu::semi_join_kernel<1, true", "void rdfgpu::semi_nested_kernel<false", "void rdfgpu::semi_nested_kernel<true",
      "rdfgpu::agg_groups_kernel", "void rdfgpu::agg_accum_kernel<false>", "void rdfgpu::agg_accum_kernel<true>", "rdfgpu::agg_final_kernel",
      "void rdfgpu::agg_accum_expr_kernel<false>", "void rdfgpu::agg_accum_expr_kernel<true>",
      "rdfgpu::band_row_win_keys_kernel", "rdfgpu::band_row_win_rows_kernel", "void rdfgpu::band_pair_bits_kernel",
      "rdfgpu::band_pair_list_count_kernel", "rdfgpu::band_pair_list_write_kernel",
      "rdfgpu::agg_value_cols_kernel", "rdfgpu::extend_kernel",
      "rdfgpu::sort_keys_kernel", "rdfgpu::sort_tile_kernel", "rdfgpu::sort_merge_kernel", "rdfgpu::sort_gather_kernel",
      "void rdfgpu::agg_accum_minmax_kernel<false>", "void rdfgpu::agg_accum_minmax_kernel<true>",
      "void rdfgpu::agg_accum_minmax_expr_kernel<false>", "void rdfgpu::agg_accum_minmax_expr_kernel<true>",
      "void rdfgpu::agg_minmax_refine_kernel",
      "rdfgpu::oj_probe_kernel(rdfgpu::OrderedJoinArgs, rdfgpu::OjBandFuse, rdfgpu::OjKeyValues)",
      "rdfgpu::agg_groups_wide_kernel", "rdfgpu::agg_wide_keys_kernel",
      "void rdfgpu::mark_join_kernel<0", "void rdfgpu::mark_join_kernel<1", "void rdfgpu::mark_nested_kernel"};
  if (kc < KC_LDS_JOIN0) return fixed[kc];
  static std::string names[192];
  static std::once_flag once;
  std::call_once(once, [] {
    const char* items[2] = {"4", "1"};
    for (int f = 0; f < 4; f++) for (int p = 0; p < 3; p++) for (int w = 0; w < 2; w++) for (int m = 0; m < 4; m++) for (int c = 0; c < 2; c++)
      names[(((f * 3 + p) * 2 + w) * 4 + m) * 2 + c] = "void rdfgpu::lds_join_kernel<" + std::to_string(f) + ", " + std::to_string(p) + ", " +
                                                       items[w] + ", " + std::to_string(m) + ", " + (c ? "true" : "false");   // (a prefix: the key-count argument follows)
  });
  return names[kc - KC_LDS_JOIN0].c_str();
}

// After the final sync: event durations + byte counts (device-side cardinalities come from the
// counters mirror copied back with the result count).
void Plan::resolve_timing() {
  for (KernelStat& k : kstats) k = KernelStat{};
  if (!timing) return;
  auto live = [&](const u64* dev, u64 fallback) -> u64 {
    if (!dev) return fallback;
    const u64 v = ctx->counters_host[dev - counters];
    return v < fallback || fallback == 0 ? v : fallback;
  };
  for (const PendingLaunch& p : pending) {
    float ms = 0;
    RDFGPU_HIP(hipEventElapsedTime(&ms, p.start, p.stop));
    KernelStat& k = kstats[p.kc];
    const u64 rows = live(p.rows_dev, p.rows_cap);
    const u64 out = p.out_dev ? ctx->counters_host[p.out_dev - counters] : p.out_rows;
    k.launches++; k.ms += ms; k.rows += rows;
    k.bytes += p.fixed_bytes + rows * p.bytes_per_row + out * p.bytes_per_out;
  }
  pending.clear();
  if (timing_focus < 0) {   // every launch was timed: remember the class that took longest (rdfgpu_plan_enable_kernel_timing(plan, 2))
    double top = 0;
    for (int kc = 0; kc < (int)(sizeof kstats / sizeof kstats[0]); kc++) if (kstats[kc].ms > top) { top = kstats[kc].ms; last_top_kc = kc; }
  }
}

// ------------------------------------------------------------------------------------------------
// execute
// ------------------------------------------------------------------------------------------------
void Plan::release_intermediates() {
  for (void* p : allocs) store->pool.free(p);
  allocs.clear();
}
// A host wait that is stream-ordered behind the predecessor's tail has returned (this execution's count wait or final wait, complete()): nothing on the device
// uses what that tail kept alive any more.  The blocks go to the pool, where any plan may take them.
void Plan::tail_waited() {
  retired.release([&](void* p) { store->pool.free(p); });
  retired_held.reset();
}
// What an execute that returned at its count point left undone: the one wait for the stream, the execution's elapsed time, the retired memory, the plan's entry among
// the store's pending tails.  Called by everything that reads result memory or finished metrics, or hands result memory to a consumer on another stream.
void Plan::complete() {
  if (!tail_pending) return;
  store->activate();
  RDFGPU_HIP(hipStreamSynchronize(stream));
  tail_pending = false;
  store->tails.remove(this);
  tail_waited();
  float ms = 0;
  if (executed && hipEventElapsedTime(&ms, ctx->event(0), ctx->event(1)) == hipSuccess) metrics.elapsed_compute_ms = ms;
  else (void)hipGetLastError();
  resolve_timing();
}
// Generic (VM) programs of the LDS join live in device memory; staged through the context's pinned slots.
const ExprProgram* Plan::upload_program(const ExprProgram& p) {
  if (progs_used >= ExecContext::kProgSlots) fail(RDFGPU_ERR_UNSUPPORTED, "plan needs more than %u device expression programs", ExecContext::kProgSlots);
  const u32 slot = progs_used++;
  ctx->progs_host[slot] = p;
  bind_values(ctx->progs_host[slot]);
  RDFGPU_HIP(hipMemcpyAsync(ctx->progs_dev + slot, ctx->progs_host + slot, sizeof(ExprProgram), hipMemcpyHostToDevice, stream));
  return ctx->progs_dev + slot;
}
// A value load names its AggregateExec and aggregate; the arrays are scratch of the execution that wrote them, so every execution binds
// its programs anew (the AggregateExec below has run by the time an operator above it prepares its launch).
void Plan::bind_values(ExprProgram& p) const {
  if (!agg_columns) return;
  for (u32 i = 0; i < p.n; i++) {
    rdfgpu_expr_node& e = p.nodes[i];
    if (e.op != kExAggValue) continue;
    const u32 node = e.u >> 8, agg = e.u & 0xffu;
    if (node >= nodes.size() || nodes[node].values_run != run) fail(RDFGPU_ERR_INVALID, "a value column of node %u is read before the node ran", node);
    e.lo = (int64_t)reinterpret_cast<uintptr_t>(nodes[node].values[agg]);
    e.hi = (int64_t)nodes[node].n_values;
  }
}
const rdfgpu_agg_value* Plan::result_values(u32 col, u64* n) const {
  const ValueOrigin& o = nodes[root].origin[col];
  if (n) *n = o.node < 0 ? 0 : nodes[o.node].n_values;
  return o.node < 0 ? nullptr : nodes[o.node].values[o.agg];
}
u64* Plan::new_counter() {
  if (counters_used >= 255) fail(RDFGPU_ERR_UNSUPPORTED, "plan needs more than 255 cardinality counters");   // slot 255: run-time error flags
  return counters + counters_used++;
}
void Plan::read_back(void* host, const void* dev, size_t bytes) {
  RDFGPU_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, stream));
  RDFGPU_HIP(hipStreamSynchronize(stream));
  metrics.host_syncs++;
}

// First execution of a plan over big caller-supplied tables (a batch of query instances): nothing is known yet, so every
// join would be sized exactly and run un-fused — on the full batch that materialises every candidate pair (126 GiB of
// intermediates for 262 144 BSBM Q5 instances).  Instead the plan first runs over the first kPrimeRows rows of each
// bound table: that builds every join table of the store slices (cached per store version) and leaves cardinalities,
// which are extrapolated by the row ratio; the full batch then takes the speculative, fused path at once.  A wrong
// extrapolation is caught like any failed speculation (overflow flag -> exact re-run).
constexpr u64 kPrimeRows = 2048;
void Plan::prime() {
  primed = true;
  if (!allow_speculation || opt.on(RDFGPU_OPT_NO_SPECULATION) || opt.on(RDFGPU_OPT_NO_PRIMING) || opt.on(RDFGPU_OPT_NO_TABLE_CACHE) || opt.on(RDFGPU_OPT_NO_CHAIN_FUSION)) return;
  u64 full = 0;
  for (const BoundTable& b : tables) if (b.bound) full = std::max(full, b.n_rows);
  if (full < 16 * kPrimeRows) return;
  for (const NodeInfo& nd : nodes) if (nd.has_last) return;
  std::vector<u64> saved(tables.size());
  for (size_t i = 0; i < tables.size(); i++) { saved[i] = tables[i].n_rows; tables[i].n_rows = std::min<u64>(tables[i].n_rows, kPrimeRows); }
  priming = true;
  try { execute(); } catch (...) { priming = false; for (size_t i = 0; i < tables.size(); i++) tables[i].n_rows = saved[i]; throw; }
  priming = false;
  for (size_t i = 0; i < tables.size(); i++) tables[i].n_rows = saved[i];
  // operators above a bound table scale with it; pure store subtrees keep their exact history
  std::vector<int> dep(nodes.size(), -1);
  std::function<bool(u32)> depends = [&](u32 i) -> bool {
    if (dep[i] >= 0) return dep[i] != 0;
    const NodeInfo& nd = nodes[i];
    bool d = false;
    if (nd.d.kind == RDFGPU_NODE_TABLE) d = true;
    else if (nd.d.kind != RDFGPU_NODE_DATA_SOURCE) {
      const bool binary = is_binary(nd.d.kind);
      if (nd.d.left >= 0) d = depends((u32)nd.d.left);
      if (binary && nd.d.right >= 0) d = depends((u32)nd.d.right) || d;
    }
    dep[i] = d ? 1 : 0;
    return d;
  };
  const u64 ratio = (full + kPrimeRows - 1) / kPrimeRows;
  for (u32 i = 0; i < nodes.size(); i++) {
    NodeInfo& nd = nodes[i];
    if (nd.has_last && depends(i)) { nd.last_rows = nd.last_rows * ratio + 1024; nd.last_scaled = true; }
  }
}

// The measurements this execution's band joins left in the counters -> NodeInfo::band.  true: one of them speculated wrongly.
bool Plan::record_band_history() {
  bool missed = false;
  for (const BandFeedback& f : band_feedback) {
    BandHistory& h = f.node->band;
    h.ran = true; h.blocks = f.known_blocks ? f.known_blocks : ctx->counters_host[f.blocks];
    h.slow_rows = ctx->counters_host[f.slow_rows] & 0xFFFFFFFFull; h.run_stats = ctx->counters_host[f.run_stats];
    if (f.slow_skipped && h.slow_rows) missed = true;   // rows with non-integer operands, and their pass was not launched
    if (f.multi_rows >= 0) h.multi_rows = ctx->counters_host[f.multi_rows] & 0xFFFFFFFFull;
    if (f.multi_rows >= 0 && f.in_place && h.multi_rows) missed = true;   // a key with 2+ table rows: the in-place records held one of them
  }
  return missed;
}

void Plan::execute() {
  if (!primed && !priming) prime();
  store->activate();
  std::shared_lock<std::shared_mutex> lock(store->mu);   // a plan holds the snapshot while it runs (snapshot.rs:35-37)
  // An execution that fails behind a pending tail leaves nothing in flight: its half-launched work would outlive this hold of the store with no event behind it.
  struct TailGuard {
    Plan* p; bool done = false;
    ~TailGuard() {
      if (done || !p->tail_pending) return;
      (void)hipStreamSynchronize(p->stream);
      p->tail_pending = false; p->store->tails.remove(p); p->tail_waited();
    }
  } tail_guard{this};
  const bool behind_tail = tail_pending;
  if (behind_tail) {   // the predecessor returned at its count point: no wait, the stream orders this execution behind its emit pass; its blocks are retired, not freed
    for (void* p : allocs) retired.retire(p, store->pool.block_bytes(p));
    allocs.clear();
    retired_held = held;
  } else {
    RDFGPU_HIP(hipStreamSynchronize(stream));
    release_intermediates();
  }
  // the pool keeps what an execution hands back for the next one — bounded by twice what the previous executions (this plan's, or any plan's of the store) used
  // (+ 1 GiB): the giant blocks of a one-off exact run go back to the device instead of staying cached for ever
  store->pool.trim_to(2 * std::max(std::max(scratch_hist[0], scratch_hist[1]), std::max(store->scratch_recent[0].load(), store->scratch_recent[1].load())) + (1ull << 30));
  held = store->gen;         // ... and the generation it read until its next execute: the result may be zero-copy slices of it
  metrics = rdfgpu_metrics{};
  const u64 mallocs0 = store->pool.mallocs() + store->table_pool.mallocs();
  const double malloc_ms0 = store->pool.malloc_ms() + store->table_pool.malloc_ms();
  run++;
  counters_used = 0;
  progs_used = 0;
  arg_slots_used = 0;
  events_used = 2;   // events 0/1 bracket the whole execute
  pending.clear();
  host_valid = false; cursor = 0; executed = false;
  agg_out.clear();
  const hipEvent_t ev_start = ctx->event(0), ev_stop = ctx->event(1);
  RDFGPU_HIP(hipEventRecord(ev_start, stream));
  RDFGPU_HIP(hipMemsetAsync(counters, 0, 256 * sizeof(u64), stream));

  spec_checks.clear();
  count_point = CountPoint{};
  pending_oj.active = false;
  band_feedback.clear();
  memo.assign(nodes.size(), DevTable{}); memo_valid.assign(nodes.size(), 0);
  speculative = allow_speculation && !opt.on(RDFGPU_OPT_NO_SPECULATION);

  refresh_dynamic_sources(lock);
  locate_sources();

  result = exec_node(root);
  flush_pending_oj();
  // The early result count: the root band join sent the counters and its total to the host in front of its emit pass (Plan::band_blocks_and_emit), and that pass
  // was the last thing launched.  The one wait is then for the count event, and the execution returns while emit runs.
  const bool early = count_point.armed && result.n_dev == count_point.n_out_dev && !pending_oj.active;
  // else one copy brings back every device-side cardinality (the result's and, for timing, the others')
  if (!early) RDFGPU_HIP(hipMemcpyAsync(ctx->counters_host, counters, 256 * sizeof(u64), hipMemcpyDeviceToHost, stream));
  RDFGPU_HIP(hipEventRecord(ev_stop, stream));
  if (early) RDFGPU_HIP(hipEventSynchronize(ctx->count_event)); else RDFGPU_HIP(hipStreamSynchronize(stream));
  metrics.host_syncs++;
  RDFGPU_HIP(hipGetLastError());
  if (behind_tail) tail_waited();   // either wait was ordered behind the predecessor's emit pass
  if (early) {   // the mirror as emit will leave the device's words: the exact total, and the overflow flag when it did not fit
    const u64 total = ctx->counters_host[256];
    ctx->counters_host[count_point.n_out] = total;
    if (total > count_point.out_cap) ctx->counters_host[count_point.overflow] |= 1ull;
    tail_pending = true;
    store->tails.add(this, ev_stop);   // (entered before this execution's hold of the store goes: a mutation waits for ev_stop)
  } else if (behind_tail) { tail_pending = false; store->tails.remove(this); }
  // a failed speculation or a run-time error is known here: the tail is completed before the exact re-run or the error
  auto settle = [&] { if (early) complete(); };
  if (const u32 rt = (u32)(ctx->counters_host[255] & 0xFFFFFFFFull)) {   // a row asked for something that is refused loudly, not answered differently
    settle();
    if (rt & 1u) fail(RDFGPU_ERR_UNSUPPORTED, "REGEX with \\d \\w \\s or \\b over a string with non-ASCII characters needs the regex crate's Unicode tables (not restated)");
    if (rt & 8u) fail(RDFGPU_ERR_UNSUPPORTED, "a numeric CAST met a simple literal: the lexical forms of numbers are not parsed on the device");
    if (rt & kRtExtendKind) fail(RDFGPU_ERR_UNSUPPORTED, "a computed column (ProjectionExec with expressions) met a value that is a string, IRI, blank node, dateTime, date, time or duration: "
                                                         "its 24-byte value has no room for the language / datatype (numeric and boolean values are carried)");
    if (rt & kRtLexParse) fail(RDFGPU_ERR_UNSUPPORTED, "a lexical cast (RDFGPU_EX_CAST_LEX, xsd:float / xsd:double of a simple literal) met a literal the device cannot decide: "
                                                       "its value lies at a rounding boundary where Eisel-Lemire declines (the big-decimal path is not restated), or it is a signed NaN");
    if (rt & kRtMinMaxKind) fail(RDFGPU_ERR_UNSUPPORTED, "MIN / MAX met a bound value that is not numeric (a string, IRI, blank node, boolean, dateTime, date, time or duration): "
                                                         "the reference's order between those kinds is partial and its 24-byte value has no room for them (numeric values are answered)");
    if (rt & kRtSortTerm) fail(RDFGPU_ERR_UNSUPPORTED, "SortExec: SORT_BY_TERM over a column that is not all strings / IRIs / blank nodes");
    if (rt & 4u) fail(RDFGPU_ERR_UNSUPPORTED, "a string expression met what the device does not restate: UCASE / LCASE of a string with non-ASCII characters (Unicode case tables), "
                                               "a float / double / decimal SUBSTR position, or a comparison with a string that has no bytes on the device");
    fail(RDFGPU_ERR_UNSUPPORTED, "REGEX with a per-row pattern: a row's pattern literal was not announced in the plan's pattern table");
  }
  // speculative joins: did the band joins take the right route, did every output fit the size taken from the previous run?
  bool spec_failed = record_band_history();
  for (const SpecCheck& c : spec_checks) {
    if ((ctx->counters_host[c.counter + 1] & 0xFFFFFFFFull) != 0) spec_failed = true;
    else { c.node->last_rows = ctx->counters_host[c.counter]; c.node->has_last = true; c.node->last_scaled = false; }
  }
  if (spec_failed) {   // rare: run again with exact sizes (one sync per join), then speculate again next time
    settle();
    tail_guard.done = true;
    metrics.host_syncs++;
    lock.unlock();
    allow_speculation = false;
    try { execute(); } catch (...) { allow_speculation = true; throw; }
    allow_speculation = true;
    metrics.exact_reruns = 1;
    return;
  }
  result_rows = result.n_dev ? ctx->counters_host[result.n_dev - counters] : result.cap;
  if (result_rows > result.cap) result_rows = result.cap;
  for (NodeInfo& nd : nodes)   // a computed column over rows counted on the device: its array holds that many values, not its capacity
    if (nd.values_run == run && nd.n_values_dev) { nd.n_values = std::min<u64>(nd.n_values, ctx->counters_host[nd.n_values_dev - counters]); nd.n_values_dev = nullptr; }
  float ms = 0;
  if (!early) RDFGPU_HIP(hipEventElapsedTime(&ms, ev_start, ev_stop));   // (early: ev_stop lies behind the running emit pass — complete() reads it)
  metrics.elapsed_compute_ms = ms;
  metrics.output_rows = result_rows;
  metrics.device_mallocs = (u32)(store->pool.mallocs() + store->table_pool.mallocs() - mallocs0);
  metrics.device_malloc_ms = store->pool.malloc_ms() + store->table_pool.malloc_ms() - malloc_ms0;
  resolve_timing();
  executed = true;
  scratch_hist[1] = scratch_hist[0]; scratch_hist[0] = metrics.device_bytes;
  store->scratch_recent[1] = store->scratch_recent[0].load(); store->scratch_recent[0] = metrics.device_bytes;
  tail_guard.done = true;
}

// Dynamic filters (scan.rs:217-261): the effective instructions of a leaf = its static ones AND the filters' current
// predicates, index re-chosen for them; derived when the filters changed (`lock` is given up while their IN sets are
// uploaded), the ranges located again.
void Plan::refresh_dynamic_sources(std::shared_lock<std::shared_mutex>& lock) {
  bool changed = false;
  for (SourceInfo& s : sources) {
    if (!s.dynamic_dirty) continue;
    ScanInstructions eff = s.gspo;
    for (auto& dflt : s.dynamic) and_into_instructions(eff, dflt.first, dflt.second);
    derive_source(s, eff);
    s.dynamic_dirty = false;
    changed = true;
  }
  if (changed) {
    lock.unlock();
    upload_pool();
    lock.lock();
    located_version = ~0ull;
    for (NodeInfo& nd : nodes) { nd.has_last = false; nd.last_rows = 0; }
    speculative = false;
  }
}

// K1: locate every data source's range in one launch, one host round trip for all of them.  The ranges
// depend only on the plan's constants and the store's content: a re-execution on an unchanged store
// reuses them (no launch, no sync).
void Plan::locate_sources() {
  if (!sources.empty() && located_version == store->version.load()) {
    for (const SourceInfo& s : sources) metrics.input_rows += s.hi - s.lo;
  } else if (!sources.empty()) {
    located_version = store->version.load();
    LocateJob* jobs = static_cast<LocateJob*>(ctx->jobs_host);
    for (size_t i = 0; i < sources.size(); i++) {
      const SourceInfo& s = sources[i];
      const Permutation& ix = store->idx[s.components];
      LocateJob& j = jobs[i];
      for (int k = 0; k < 4; k++) j.col[k] = ix.col[k];
      j.n = ix.n;
      j.n_levels = s.prune.n_levels;
      for (int k = 0; k < 4; k++) { j.from[k] = s.prune.from[k]; j.to[k] = s.prune.to[k]; }
    }
    LocateJob* jobs_dev = static_cast<LocateJob*>(ctx->jobs_dev);
    RDFGPU_HIP(hipMemcpyAsync(jobs_dev, jobs, sources.size() * sizeof(LocateJob), hipMemcpyHostToDevice, stream));
    timed(KC_LOCATE, 0, sources.size(), nullptr, 0, nullptr, 0, 0, [&] { launch_locate(jobs_dev, (u32)sources.size(), ctx->lohi_dev, stream); });
    read_back(ctx->lohi_host, ctx->lohi_dev, sources.size() * kLocateWords * sizeof(u64));
    for (size_t i = 0; i < sources.size(); i++) {
      const u64* w = ctx->lohi_host + kLocateWords * i;
      SourceInfo& s = sources[i];
      s.lo = w[0]; s.hi = w[1]; s.sorted_level = (u32)(w[2] >> 32); s.key_min = (u32)w[2]; s.key_max = (u32)w[3];
      metrics.input_rows += s.hi - s.lo;
    }
  }
}

DevTable Plan::exec_node(u32 idx) {
  if (memo_valid[idx]) return memo[idx];   // a node runs once per execution, however many operators consume it
  NodeInfo& nd = nodes[idx];
  DevTable t;
  switch (nd.d.kind) {
    case RDFGPU_NODE_DATA_SOURCE: t = exec_source(nd); break;
    case RDFGPU_NODE_FILTER: t = exec_filter(nd); break;
    case RDFGPU_NODE_PROJECTION: t = exec_projection(nd); break;
    case RDFGPU_NODE_HASH_JOIN: case RDFGPU_NODE_CROSS_JOIN: case RDFGPU_NODE_NESTED_LOOP_JOIN:
      // semi / anti / mark joins leave before anything of exec_join (chain planning, filter fusion, side choice) sees them
      t = nd.d.join_type == RDFGPU_JOIN_LEFT_SEMI || nd.d.join_type == RDFGPU_JOIN_LEFT_ANTI ? exec_semi_join(nd)
        : nd.d.join_type == RDFGPU_JOIN_LEFT_MARK ? exec_mark_join(nd) : exec_join(nd);
      break;
    case RDFGPU_NODE_TOPK: t = exec_topk(nd); break;
    case RDFGPU_NODE_AGGREGATE: t = exec_aggregate(nd); break;
    case RDFGPU_NODE_EXTEND: t = exec_extend(nd); break;
    case RDFGPU_NODE_SORT: t = exec_sort(nd); break;
    case RDFGPU_NODE_CLOSURE: t = exec_closure(nd); break;
    case RDFGPU_NODE_UNION: t = exec_union(nd); break;
    case RDFGPU_NODE_TABLE: t = exec_table(nd); break;
    default: fail(RDFGPU_ERR_INVALID, "unknown node kind");
  }
  if (idx != root) metrics.intermediate_rows += t.cap;   // upper bound when the exact count stays on the device
  if (!(pending_chain && pending_chain->consumed)) { memo[idx] = t; memo_valid[idx] = 1; }   // (a fused chain's output belongs to its top node)
  return t;
}

// Executes node `idx` as a sub-plan of its own: a chain request pending for the caller must not reach the joins below it.
DevTable Plan::exec_sub_plan(u32 idx) {
  ChainRequest* const for_caller = pending_chain;
  pending_chain = nullptr;
  const DevTable t = exec_node(idx);
  pending_chain = for_caller;
  return t;
}

// ProjectionExec: the input's columns, selected (no launch).
DevTable Plan::exec_projection(NodeInfo& nd) { return project(exec_node((u32)nd.d.left), nd); }

// KleenePlusClosureExec (closure.hip): its row count comes back to the host, so does every iteration's.
DevTable Plan::exec_closure(NodeInfo& nd) {
  DevTable t;
  const DevTable in = exec_node((u32)nd.d.left);
  const u64 n = in.n_dev && in.cap ? read_back<u64>(in.n_dev) : in.cap;
  u32* out[3] = {nullptr, nullptr, nullptr};
  ClosureStats cs;
  const u64 rows = closure_exec(in.cols[0], in.cols[1], in.cols[2], n, nd.d.join_type == 1, stream, [&](u64 m) { return scratch<u32>(m); }, out, &cs);
  metrics.host_syncs += 4 + 3 * cs.iterations;
  t.n_cols = nd.n_proj; t.cap = rows; t.n_dev = nullptr;
  for (u32 c = 0; c < nd.n_proj; c++) t.cols[c] = out[nd.proj[c]];
  return t;
}

// UnionExec: both inputs' projected columns copied into one table.
DevTable Plan::exec_union(NodeInfo& nd) {
  DevTable t;
  const DevTable L = exec_node((u32)nd.d.left), R = exec_node((u32)nd.d.right);
  t.n_cols = nd.n_proj;
  const u64 cap = L.cap + R.cap;
  if (cap >= 0xFFFFFFF0ull) fail(RDFGPU_ERR_UNSUPPORTED, "UnionExec of %llu rows", (unsigned long long)cap);
  if (cap == 0) { t.cap = 0; return t; }
  UnionArgs a{};
  a.n_cols = nd.n_proj;
  for (u32 c = 0; c < nd.n_proj; c++) {
    a.left[c] = L.cap ? L.cols[nd.proj[c]] : nullptr; a.right[c] = R.cap ? R.cols[nd.proj[c]] : nullptr;
    a.out[c] = scratch<u32>(cap); t.cols[c] = a.out[c];
  }
  a.n_left_dev = L.n_dev; a.n_left_cap = L.cap; a.n_right_dev = R.n_dev; a.n_right_cap = R.cap;
  const bool dyn = L.n_dev || R.n_dev;
  a.n_out_dev = dyn ? new_counter() : nullptr;
  // bytes: every projected cell read once and written once
  timed(KC_UNION, R.n_dev ? 0 : 8ull * nd.n_proj * R.cap, L.cap, L.n_dev, 8ull * nd.n_proj, nullptr, 0, 0, [&] { launch_union(a, stream); });
  t.cap = cap; t.n_dev = a.n_out_dev;
  return t;
}

// A caller-supplied table (rdfgpu_plan_bind_table): its columns as they are.
DevTable Plan::exec_table(NodeInfo& nd) {
  DevTable t;
  const BoundTable& b = tables[nd.d.table_slot];
  if (!b.bound) fail(RDFGPU_ERR_INVALID, "table slot %u is not bound", nd.d.table_slot);
  if (b.cols.size() != nd.d.table_cols) fail(RDFGPU_ERR_INVALID, "table slot %u: %zu columns bound, node declares %u", nd.d.table_slot, b.cols.size(), nd.d.table_cols);
  t.n_cols = nd.d.table_cols; t.cap = b.n_rows;
  for (u32 c = 0; c < t.n_cols; c++) t.cols[c] = b.cols[c];
  return t;
}

// DataSourceExec: a prefix-bound pattern is a zero-copy slice of the permutation (like the
// reference's untouched row-group slices, scan.rs:146-170); residual predicates go through K2.
DevTable Plan::exec_source(NodeInfo& nd) {
  SourceInfo& s = sources[nd.source];
  const Permutation& ix = store->idx[s.components];
  DevTable t;
  t.n_cols = s.n_out;
  const u64 n = s.hi - s.lo;
  if (n == 0) { t.cap = 0; return t; }
  if (!s.has_residual) {
    for (u32 c = 0; c < s.n_out; c++) t.cols[c] = ix.col[s.out_level[c]] + s.lo;
    t.cap = n;
    t.stable_id = (u64)nd.source + 1;   // a pure slice of the store: identical on every execution until the store changes
    for (u32 c = 0; c < s.n_out; c++) if (s.out_level[c] == s.sorted_level && t.sorted_col < 0) { t.sorted_col = (int)c; t.key_min = s.key_min; t.key_max = s.key_max; }
    return t;
  }
  ScanJob job{};
  for (int k = 0; k < 4; k++) {
    job.col[k] = ix.col[k] + s.lo;
    const ScanPredicate& p = s.ix.in[k].pred;
    ScanLevelPred& q = job.pred[k];
    q.kind = (s.prune.dropped_mask & (1u << k)) ? (u32)RDFGPU_PRED_NONE : p.kind;
    if (q.kind == RDFGPU_PRED_BETWEEN) { q.a = p.from; q.b = p.to; }
    else if (q.kind == RDFGPU_PRED_IN) { q.b = (u32)p.ids.size(); q.ids = pool_dev + p.from; }
    else if (q.kind == RDFGPU_PRED_EQUAL_TO) {
      int other = -1;
      for (int l = 0; l < 4; l++) if (s.ix.in[l].kind == RDFGPU_SCAN && s.ix.in[l].var == p.equal_to) { other = l; break; }
      if (other < 0) q.kind = RDFGPU_PRED_NONE;   // `position(..)?` => no mask (scan.rs:310-313)
      else q.a = (u32)other;
    }
  }
  job.n = n;
  job.n_out = s.n_out;
  for (u32 c = 0; c < s.n_out; c++) job.out_level[c] = s.out_level[c];
  const u64 n_blocks = (n + kScanTile - 1) / kScanTile;
  u32* counts = scratch<u32>(n_blocks + 1);
  u32* offs = scratch<u32>(n_blocks + 1);
  const size_t tb = scan_temp_bytes(n_blocks + 1);
  void* temp = scratch<u8>(tb);
  RDFGPU_HIP(hipMemsetAsync(counts + n_blocks, 0, 4, stream));
  u32 n_pred_cols = 0;   // columns the residual predicates read
  for (int k = 0; k < 4; k++) n_pred_cols += job.pred[k].kind != RDFGPU_PRED_NONE && job.pred[k].kind != RDFGPU_PRED_FALSE;
  timed(KC_SCAN_COUNT, 0, n, nullptr, 4ull * n_pred_cols, nullptr, 0, 0, [&] { launch_scan_count(job, counts, stream); });
  timed(scan_class(n_blocks + 1), 0, n_blocks + 1, nullptr, 8, nullptr, 0, 0, [&] { exclusive_scan_u32(counts, offs, n_blocks + 1, temp, tb, stream); });
  const u32 total = read_back<u32>(offs + n_blocks);
  t.cap = total;
  if (total == 0) return t;
  for (u32 c = 0; c < s.n_out; c++) { job.out[c] = scratch<u32>(total); t.cols[c] = job.out[c]; }
  // scan+filter+compact: 4·c_r·N + 4·c_w·σN, c_r = predicate ∪ output columns (upper bound: both)
  if (s.n_out) timed(KC_SCAN_WRITE, 0, n, nullptr, 4ull * n_pred_cols, nullptr, total, 8ull * s.n_out, [&] { launch_scan_write(job, offs, stream); });
  return t;
}

// DISTINCT + ORDER BY keys LIMIT k (per group): counting sort of row ids by group, one wave per group selecting the k
// smallest distinct key tuples, compaction by offsets.  Two host round trips (largest group id; final count + the
// "unsupported kind in a SORT_BY_TERM column" flag): this operator ends a query, it is not inside the join pipeline.
DevTable Plan::exec_topk(NodeInfo& nd) {
  const DevTable in = exec_node((u32)nd.d.left);
  DevTable t;
  t.n_cols = nd.n_proj;
  if (in.cap == 0) { t.cap = 0; return t; }
  if (in.cap >= (1ull << 32)) fail(RDFGPU_ERR_UNSUPPORTED, "TopK over %llu rows", (unsigned long long)in.cap);
  TopkArgs a{};
  for (u32 c = 0; c < in.n_cols; c++) a.in[c] = in.cols[c];
  a.n_in_dev = in.n_dev; a.n_in_cap = in.cap;
  a.has_group = nd.d.table_slot != 0; a.group_col = a.has_group ? nd.d.table_slot - 1 : 0;
  a.n_keys = nd.d.n_keys;
  for (u32 k = 0; k < a.n_keys; k++) { a.key_col[k] = nd.d.left_keys[k]; a.key_by_term[k] = nd.d.right_keys[k]; }   // RDFGPU_SORT_BY_*
  a.k = nd.d.table_cols;
  a.tt = typed_table();
  u64* n_out = new_counter();
  u32* flags = reinterpret_cast<u32*>(new_counter());   // {largest group id, unsupported-kind flag}
  a.n_out_dev = n_out; a.bad = flags + 1;
  a.n_groups = 1;
  if (a.has_group) {
    timed(KC_TOPK_MAX, 0, in.cap, in.n_dev, 4, nullptr, 0, 0, [&] { launch_topk_max(a.in[a.group_col], in.n_dev, in.cap, flags, stream); });
    const u32 mx = read_back<u32>(flags);
    if (mx >= (1u << 24)) fail(RDFGPU_ERR_UNSUPPORTED, "TopK: group ids up to %u (dense ids below 2^24 expected)", mx);
    a.n_groups = mx + 1;
  }
  const u64 ng = a.n_groups;
  a.counts = scratch<u32>(ng + 1); a.offsets = scratch<u32>(ng + 1); a.cursor = scratch<u32>(ng);
  a.perm = scratch<u32>(in.cap); a.picked = scratch<u32>(ng * a.k);
  a.out_counts = scratch<u32>(ng + 1); a.out_offsets = scratch<u32>(ng + 1);
  const u64 out_cap = std::min<u64>(in.cap, ng * a.k);
  a.n_out_cols = nd.n_proj;
  for (u32 c = 0; c < nd.n_proj; c++) { a.proj[c] = nd.proj[c]; a.out[c] = scratch<u32>(out_cap); t.cols[c] = a.out[c]; }
  RDFGPU_HIP(hipMemsetAsync(a.counts, 0, (ng + 1) * sizeof(u32), stream));
  RDFGPU_HIP(hipMemsetAsync(a.out_counts, 0, (ng + 1) * sizeof(u32), stream));
  const size_t tb = scan_temp_bytes(ng + 1);
  void* temp = scratch<unsigned char>(tb);
  u32 key_bytes = 4 * a.n_keys;
  for (u32 k = 0; k < a.n_keys; k++) key_bytes += a.key_by_term[k] ? 16 : 0;
  timed(KC_TOPK_HIST, 0, in.cap, in.n_dev, 4, nullptr, 0, 0, [&] { launch_topk_hist(a, stream); });
  exclusive_scan_u32(a.counts, a.offsets, ng + 1, temp, tb, stream);
  RDFGPU_HIP(hipMemcpyAsync(a.cursor, a.offsets, ng * sizeof(u32), hipMemcpyDeviceToDevice, stream));
  timed(KC_TOPK_SCATTER, 0, in.cap, in.n_dev, 8, nullptr, 0, 0, [&] { launch_topk_scatter(a, stream); });
  timed(KC_TOPK_SELECT, 0, in.cap, in.n_dev, (4ull + key_bytes) * a.k, nullptr, 0, 0, [&] { launch_topk_select(a, stream); });
  exclusive_scan_u32(a.out_counts, a.out_offsets, ng + 1, temp, tb, stream);
  timed(KC_TOPK_WRITE, 0, 0, nullptr, 0, n_out, 0, 8ull * nd.n_proj, [&] { launch_topk_write(a, stream); });
  const u32 i0 = (u32)(n_out - counters);
  read_back(ctx->counters_host + i0, counters + i0, 2 * sizeof(u64));
  if ((ctx->counters_host[i0 + 1] >> 32) != 0) fail(RDFGPU_ERR_UNSUPPORTED, "TopK: SORT_BY_TERM over a column that is not all strings / IRIs / blank nodes");
  t.cap = std::min<u64>(out_cap, ctx->counters_host[i0]);
  t.n_dev = n_out;
  return t;
}

// ProjectionExec with expressions (extend.hip): one launch over the input's rows writes, per computed column, every row's 24-byte value
// and its entry (row + 1, or 0).  The kept columns are the input's own buffers, handed on: nothing of them is copied.  The input's row
// count may live on the device only: the arrays are sized by its capacity, the kernel stops at the live rows.  Behind the capacity of
// every array lies one guard element, set before the launch, which a test can read (rdfgpu_plan_result_values' length is the capacity
// when the row count is known on the host): a write past the input's rows would show there.
// Compulsory bytes: per input row 4 per column a program reads, 16 per ENC_TV gather, 24 + 4 per computed column.
constexpr int kExtendGuard = 0xA5;
DevTable Plan::exec_extend(NodeInfo& nd) {
  const DevTable in = exec_sub_plan((u32)nd.d.left);
  flush_pending_oj();   // a held-back ordered-join write must have happened before the input is read
  if (in.cap >= 0xFFFFFFFFull) fail(RDFGPU_ERR_UNSUPPORTED, "ProjectionExec with expressions over %llu rows (fewer than 2^32 - 1)", (unsigned long long)in.cap);
  const u32 k = (u32)nd.agg_progs.size();
  DevTable t = project(in, nd);
  t.n_cols = nd.width;
  ExtendArgs a{};
  a.n_dev = in.n_dev; a.cap = in.cap;
  for (u32 c = 0; c < in.n_cols; c++) a.col[c] = in.cols[c];
  a.n_exprs = k;
  a.tt = typed_table();
  for (u32 q = 0; q < k; q++) {   // one guard record / word (bytes of kExtendGuard) behind each array: the kernel writes the live rows and nothing else
    a.out[q] = scratch<rdfgpu_agg_value>(in.cap + 1); a.out_val[q] = scratch<u32>(in.cap + 1);
    RDFGPU_HIP(hipMemsetAsync(a.out[q] + in.cap, kExtendGuard, sizeof(rdfgpu_agg_value), stream));
    RDFGPU_HIP(hipMemsetAsync(a.out_val[q] + in.cap, kExtendGuard, sizeof(u32), stream));
    nd.values[q] = a.out[q]; t.cols[nd.n_proj + q] = a.out_val[q];
  }
  nd.n_values = in.cap; nd.n_values_dev = in.cap ? in.n_dev : nullptr; nd.values_run = run;
  if (in.cap == 0) return t;
  for (u32 q = 0; q < k; q++) a.prog[q] = upload_program(nd.agg_progs[q]);
  timed(KC_EXTEND, 0, in.cap, in.n_dev, 4ull * nd.n_cols_read + 16ull * nd.n_enc_tv + 28ull * k, nullptr, 0, 0, [&] { launch_extend(a, nd.lex, stream); });
  return t;
}

void Plan::ensure_host_copy() {
  if (host_valid) return;
  if (!executed) fail(RDFGPU_ERR_INVALID, "plan has not been executed");
  complete();
  store->activate();
  host_cols.assign(result.n_cols, std::vector<u32>());
  for (u32 c = 0; c < result.n_cols; c++) {
    host_cols[c].resize(result_rows);
    if (result_rows) RDFGPU_HIP(hipMemcpyAsync(host_cols[c].data(), result.cols[c], result_rows * 4, hipMemcpyDeviceToHost, stream));
  }
  host_aggs.assign(agg_out.size(), std::vector<rdfgpu_agg_value>());
  for (size_t i = 0; i < agg_out.size(); i++) {
    host_aggs[i].resize(result_rows);
    if (result_rows) RDFGPU_HIP(hipMemcpyAsync(host_aggs[i].data(), agg_out[i], result_rows * sizeof(rdfgpu_agg_value), hipMemcpyDeviceToHost, stream));
  }
  RDFGPU_HIP(hipStreamSynchronize(stream));
  // a value column's rows index their AggregateExec's array: one value per result row, tag 0 where the binding is unbound.  Each array comes
  // over once, however many columns index it, and all of them behind one wait.
  host_values.assign(result.n_cols, std::vector<rdfgpu_agg_value>());
  std::vector<const rdfgpu_agg_value*> origins; std::vector<std::vector<rdfgpu_agg_value>> copies;
  std::vector<int> copy_of(result.n_cols, -1);
  for (u32 c = 0; c < result.n_cols; c++) {
    u64 n = 0;
    const rdfgpu_agg_value* dev = result_values(c, &n);
    if (!dev) continue;
    const size_t at = std::find(origins.begin(), origins.end(), dev) - origins.begin();
    if (at == origins.size()) { origins.push_back(dev); copies.emplace_back(result_rows ? n : 0); }
    copy_of[c] = (int)at;
  }
  for (size_t i = 0; i < origins.size(); i++)
    if (!copies[i].empty()) RDFGPU_HIP(hipMemcpyAsync(copies[i].data(), origins[i], copies[i].size() * sizeof(rdfgpu_agg_value), hipMemcpyDeviceToHost, stream));
  if (!origins.empty()) RDFGPU_HIP(hipStreamSynchronize(stream));
  for (u32 c = 0; c < result.n_cols; c++) {
    if (copy_of[c] < 0) continue;
    const std::vector<rdfgpu_agg_value>& all = copies[copy_of[c]];
    host_values[c].assign(result_rows, rdfgpu_agg_value{});
    for (u64 r = 0; r < result_rows; r++) { const u32 id = host_cols[c][r]; if (id != 0 && id <= all.size()) host_values[c][r] = all[id - 1]; }
  }
  host_valid = true;
}

}  // namespace rdfgpu
