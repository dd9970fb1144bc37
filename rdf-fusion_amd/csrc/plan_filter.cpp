// plan_filter.cpp — FilterExec: the routes a predicate takes over a binding table (kernels.hip).
//   Plan::exec_filter       FilterExec over ENC_TV/GT/ADD/EBV UDFs  (DataFusion 52 + lib/functions)
#include "plan_exec.hpp"

namespace rdfgpu {

DevTable Plan::exec_filter(NodeInfo& nd) {
  const DevTable in = exec_node((u32)nd.d.left);
  return apply_filter(nd, in);
}

// FilterExec over `in`: nothing to do, a plain projection, or one of four routes.  They all leave the survivors in a.out (= t.cols)
// and their count in a.n_out_dev.
DevTable Plan::apply_filter(NodeInfo& nd, const DevTable& in) {
  DevTable t;
  t.n_cols = nd.n_proj;
  if (in.cap == 0) { t.cap = 0; return t; }
  if (nd.prog.n == 0) return project(in, nd);   // no predicate: a projection
  FilterArgs a{};
  for (u32 c = 0; c < in.n_cols; c++) a.in[c] = in.cols[c];
  a.n_in_cols = in.n_cols; a.n_out_cols = nd.n_proj;
  for (u32 c = 0; c < nd.n_proj; c++) { a.proj[c] = nd.proj[c]; a.out[c] = scratch<u32>(in.cap); t.cols[c] = a.out[c]; }
  a.n_in_dev = in.n_dev; a.n_in_cap = in.cap;
  a.n_out_dev = new_counter();
  a.tt = typed_table();
  a.prog = nd.prog;
  bind_values(a.prog);
  int shape = nd.shape;
  if (shape == 3 && !filter_string_verdicts(nd, in, a)) shape = 0;
  if (!filter_run_copy(nd, in, a, shape)) {
    if (filter_streams(a, shape)) filter_streamed(nd, in, a, shape);
    else filter_single_pass(nd, in, a, shape);
  }
  t.cap = in.cap; t.n_dev = a.n_out_dev;
  return t;
}

// Shape 3, EBV(REGEX | CONTAINS | STRSTARTS | STRENDS (ENC_TV(col), constant)), per-distinct-term verdicts: worth a pass over the
// dictionary when the table has at least a quarter as many rows as there are ids (or the verdicts exist already); the table lives
// on the store, keyed by the predicate.  true: a.verdict holds it (shape 3 stands); false: the VM answers per row.
bool Plan::filter_string_verdicts(const NodeInfo& nd, const DevTable& in, FilterArgs& a) {
  const rdfgpu_expr_node& e = nd.prog.nodes[2];
  const rdfgpu_regex& rx = regex_text[e.u];
  std::string key(1, (char)e.op);
  key.append(reinterpret_cast<const char*>(&e.lo), sizeof e.lo);
  key.append(rx.flags ? std::string(rx.flags, rx.flags_len) : std::string()).push_back('\0');
  key.append(rx.pattern ? std::string(rx.pattern, rx.pattern_len) : std::string());
  const u64 n_ids = std::min<u64>(store->n_ids, store->n_str_ids);
  unsigned char* verdict = nullptr;
  if (!opt.on(RDFGPU_OPT_NO_STRING_VERDICTS) && n_ids > 0) {
    std::unique_lock<std::mutex> building(store->slice_build_mu);
    { std::lock_guard<std::mutex> l(store->slice_mu); auto it = store->string_verdicts.find(key); if (it != store->string_verdicts.end()) verdict = it->second; }
    if (!verdict && in.cap * 4 >= n_ids) {
      // bounded cache: a workload of ever-changing patterns must not pile up one table per pattern — beyond 64
      // entries the table is this execution's scratch
      bool cache_it;
      { std::lock_guard<std::mutex> l(store->slice_mu); cache_it = store->string_verdicts.size() < 64; }
      if (cache_it) RDFGPU_HIP(hipMalloc((void**)&verdict, n_ids)); else verdict = scratch<unsigned char>(n_ids);
      const int64_t lang = e.op == RDFGPU_EX_REGEX ? -1 : (e.lo < 0 ? 0 : e.lo);
      timed(KC_REGEX_VERDICTS, 0, n_ids, nullptr, 16 + 8 + 1, nullptr, 0, 0, [&] { TypedTable vt = a.tt; vt.rt_error = nullptr;   // a verdict pass covers the whole dictionary: what it cannot answer is verdict 3, an error only for a row that reads it
                                                                                             launch_regex_verdicts(regex_dev + e.u, vt, lang, verdict, n_ids, stream); });
      if (cache_it) {
        RDFGPU_HIP(hipStreamSynchronize(stream)); metrics.host_syncs++;   // complete before other plans may see it
        std::lock_guard<std::mutex> l(store->slice_mu);
        store->string_verdicts[key] = verdict;
      }
    }
  }
  if (verdict) { a.verdict = verdict; a.n_verdict = n_ids; }
  return verdict != nullptr;
}

// Run copy, for a typed comparison on the sorted column of a big store slice with few distinct ids: the qualifying runs are copied, the
// predicate column is not streamed at all.  Carries its own eligibility test; true: it ran.
bool Plan::filter_run_copy(const NodeInfo& nd, const DevTable& in, FilterArgs& a, int shape) {
  if (shape == 2 && !opt.on(RDFGPU_OPT_NO_VALUE_VERDICTS) && !opt.on(RDFGPU_OPT_NO_RUN_COPY) && in.sorted_col >= 0 && (u32)in.sorted_col == nd.prog.nodes[0].u &&
      in.key_max >= in.key_min && !in.n_dev && in.cap >= (1ull << 20) && in.cap < (1ull << 32) && nd.n_proj <= 2) {
    const u64 span = (u64)in.key_max - in.key_min + 1;
    if (span <= kRunCopyMaxIds && span * 1024 <= in.cap) {
      a.value_min = in.key_min; a.value_span = span;
      a.stream_bits = reinterpret_cast<unsigned short*>(scratch<u32>(1)); a.stream_counts = scratch<u32>(1); a.stream_offs = a.stream_counts;   // (the argument block wants them non-null)
      // Where every id's run starts is a function of the slice alone: kept with the slice's other tables per store version (the searches
      // that find them are five dependent HBM round trips per id: 10 of the operator's 68 us); with the table at hand the comparison of
      // every id is answered in the scan kernel — one launch plans the copy.
      const u32* pcol = in.cols[in.sorted_col];
      const bool cacheable = in.stable_id != 0 && !opt.on(RDFGPU_OPT_NO_TABLE_CACHE);
      u32* cached_lo = nullptr;
      SliceTable* vst = nullptr;
      std::unique_lock<std::mutex> building(store->slice_build_mu, std::defer_lock);
      if (cacheable) {
        SliceKey sk; sk.n_keys = 1; sk.rows = in.cap; sk.key[0] = pcol;
        vst = store->slice_table(sk);
        building.lock();
        for (const auto& v : vst->value_starts) if (v.first == in.key_min && v.span == span) cached_lo = v.lo;
      }
      const bool own = cacheable && !cached_lo && vst->value_starts.size() < 4;
      u32* run_lo = cached_lo ? cached_lo : own ? store->table_alloc<u32>(span + 1) : scratch<u32>(span + 1);   // (one entry past the last id)
      RunCopyBuffers b{run_lo, scratch<u32>(span), scratch<u32>(span + 1), scratch<u32>(span + 1), scratch<u32>(span + 1), scratch<u32>(1)};
      if (!cached_lo) timed(KC_VALUE_RUNS, 0, span, nullptr, 16, nullptr, 0, 0, [&] { launch_value_runs(a, b, stream); });
      // (one launch for scan + copy — 2048 workgroups that each scan the run lengths in LDS and copy an equal share — was tried: 68 us
      //  against 6 + 51: the big chunks do not hide their memory latency the way 16 K small workgroups do)
      timed(KC_RUN_SCAN, 0, span, nullptr, cached_lo ? 16 + 8 : 8, nullptr, 0, 0, [&] { launch_run_scan(a, b, cached_lo != nullptr, stream); });
      if (own) {   // publish only when complete
        RDFGPU_HIP(hipStreamSynchronize(stream)); metrics.host_syncs++; metrics.tables_built++;
        vst->value_starts.push_back(SliceTable::ValueStarts{in.key_min, span, run_lo});
      }
      if (building.owns_lock()) building.unlock();
      timed(KC_RUN_COPY, 0, 0, nullptr, 0, a.n_out_dev, 0, 8ull * nd.n_proj, [&] { launch_run_copy(a, b, stream); });
      return true;
    }
  }
  return false;
}

// Streamed: two passes without atomics — verdict bits + tile counts, device scan, ordered write.
void Plan::filter_streamed(const NodeInfo& nd, const DevTable& in, FilterArgs& a, int shape) {
  const u64 tiles = filter_stream_tiles(a);
  a.stream_bits = scratch<unsigned short>(tiles * 256);
  a.stream_counts = scratch<u32>(tiles + 1); a.stream_offs = scratch<u32>(tiles + 1);
  a.stream_temp_bytes = scan_temp_bytes(tiles + 1);
  a.stream_temp = scratch<unsigned char>(a.stream_temp_bytes);
  RDFGPU_HIP(hipMemsetAsync(a.stream_counts + tiles, 0, sizeof(u32), stream));
  // compulsory bytes: pass 1 streams the predicate column (its typed-value gathers hit a table that is cache-resident or
  // not: not counted) and writes one bit per row; pass 2 reads the bits and the output columns and writes the survivors
  // a typed comparison over the sorted column of a store slice: answered once per id of the slice's id range when that
  // range is small next to the rows (a GPOS slice of one predicate: its objects), then one bit per row
  if (shape == 2 && !opt.on(RDFGPU_OPT_NO_VALUE_VERDICTS) && in.sorted_col >= 0 && (u32)in.sorted_col == nd.prog.nodes[0].u && in.key_max >= in.key_min) {
    const u64 span = (u64)in.key_max - in.key_min + 1;
    if (span * 4 <= in.cap) {
      u32* words = scratch<u32>(((span + 63) / 64) * 2);
      a.value_bits = words; a.value_min = in.key_min; a.value_span = span;
      timed(KC_VALUE_VERDICTS, 0, span, nullptr, 16, nullptr, 0, 0, [&] { launch_value_verdicts(a, stream); });
      shape = 4;
    }
  }
  const int kc1 = shape == 1 ? KC_FILTER_BITS_ID : shape == 2 ? KC_FILTER_BITS_TV : shape == 4 ? KC_FILTER_BITS_VALUE : KC_FILTER_BITS_VERDICT;
  timed(kc1, tiles * 4, in.cap, in.n_dev, 4, nullptr, 0, 0, [&] { launch_filter_bits(a, shape, stream); });
  timed(scan_class(tiles + 1), 0, tiles + 1, nullptr, 8, nullptr, 0, 0, [&] { exclusive_scan_u32(a.stream_counts, a.stream_offs, tiles + 1, a.stream_temp, a.stream_temp_bytes, stream); });
  timed(KC_FILTER_WRITE, tiles * 8, in.cap, in.n_dev, 4ull * nd.n_proj, a.n_out_dev, 0, 4ull * nd.n_proj, [&] { launch_filter_write(a, shape, stream); });
}

// Single pass.  FilterExec bytes: 4·c_r·N + t·N + 4·c_w·σN with t = 9 B per typed gather (tag + i64); shape 3: t = 1 B
void Plan::filter_single_pass(const NodeInfo& nd, const DevTable& in, FilterArgs& a, int shape) {
  const int kc = shape == 1 ? KC_FILTER_ID : shape == 2 ? KC_FILTER_TV : shape == 3 ? KC_FILTER_VERDICT : KC_FILTER_VM;
  timed(kc, 0, in.cap, in.n_dev, shape == 3 ? 4ull * nd.n_cols_read + 1 : 4ull * nd.n_cols_read + 9ull * nd.n_enc_tv, a.n_out_dev, 0, 4ull * nd.n_proj,
        [&] { launch_filter(a, shape, stream); });
}

}  // namespace rdfgpu
