// plan_band.cpp — a run of look-up joins fused into its base join (chain fusion), and the chain run as a band join (band_join.hip).
#include "plan_exec.hpp"

namespace rdfgpu {

namespace {
bool range_op(u8 op) { return op == RDFGPU_EX_GT || op == RDFGPU_EX_LT || op == RDFGPU_EX_GEQ || op == RDFGPU_EX_LEQ; }
}  // namespace

// Fused lookup chain (R4): walks down from `top` through inner single-key hash joins whose one input is a pure store
// slice with a cached DIRECT-address table and whose other input is a hash join consumed only here.  Only tried on
// speculative re-executions (cardinalities and tables known from the first run).
bool Plan::plan_chain(NodeInfo& top, ChainRequest& req) {
  if (!speculative || !top.has_last || opt.on(RDFGPU_OPT_NO_CHAIN_FUSION) || opt.on(RDFGPU_OPT_NO_TABLE_CACHE)) return false;
  req.top = &top;
  std::vector<ChainLink> down;
  NodeInfo* cur = &top;
  while ((int)down.size() < kMaxChain) {
    const rdfgpu_plan_node& d = cur->d;
    if (d.kind != RDFGPU_NODE_HASH_JOIN || d.join_type != RDFGPU_JOIN_INNER || d.n_keys != 1) break;
    if (cur->prog.n != 0 && cur->shape != 2 && cur->shape != 3) break;
    bool found = false;
    for (int side = 0; side < 2 && !found; side++) {
      const u32 cs = (u32)(side == 0 ? d.left : d.right), co = (u32)(side == 0 ? d.right : d.left);
      const NodeInfo& sn = nodes[cs]; const NodeInfo& on = nodes[co];
      if (sn.d.kind != RDFGPU_NODE_DATA_SOURCE || sources[sn.source].has_residual) continue;
      if (on.d.kind != RDFGPU_NODE_HASH_JOIN || on.d.join_type > RDFGPU_JOIN_LEFT || on.refs != 1) continue;   // (a semi / anti join is no chain base)
      const DevTable S = exec_node(cs);   // a slice: no launch
      if (S.cap == 0 || S.stable_id == 0) continue;
      SliceKey sk; sk.n_keys = 1; sk.rows = S.cap; sk.key[0] = S.cols[side == 0 ? d.left_keys[0] : d.right_keys[0]];
      const SliceTable* st = store->find_slice_table(sk);
      if ((!st || !st->dense_tried) && S.n_dev == nullptr && S.cap > std::min<u64>(opt.v[RDFGPU_OPT_LDS_MAX_BUILD], kLdsJoinMaxBuild) && !opt.on(RDFGPU_OPT_NO_DIRECT_TABLE)) {
        // the store changed since this chain last ran (its history is still good): the slice's table is built here, inside
        // the execution, and the chain stays fused — no un-fused execution just to get the tables back
        SliceTable* fresh = store->slice_table(sk);
        std::unique_lock<std::mutex> building(store->slice_build_mu);
        if (!fresh->dense_tried) build_dense_table(fresh, sk.key[0], S.cap);
        st = fresh;
      }
      if (!st || !st->direct) continue;
      down.push_back(ChainLink{cur, side == 0, S, st});
      cur = &nodes[co];
      found = true;
    }
    if (!found) break;
  }
  if (down.empty()) return false;
  req.links.assign(down.rbegin(), down.rend());   // bottom-up: links[0] sits directly above the base join
  return true;
}

// Resolves the chain against the base join `j` and leaves it in j.a: as a band join where it has that shape (j.use_band, j.band), else with the range index
// of its first stage where that applies.  false (j.a.n_chain stays 0: the stages written so far are not read) if some column cannot be addressed the way the kernel needs.
bool Plan::apply_chain(const ChainRequest& req, LdsJoin& j) {
  if (!resolve_chain(req, j)) return false;
  j.use_band = chain_band_args(req, j);
  if (!j.use_band) chain_range_index(j, j.a.chain[0]);
  j.a.n_chain = (u32)req.links.size(); j.a.n_out_cols = (u32)j.chain_cols.size();
  for (size_t k = 0; k < j.chain_cols.size(); k++) j.a.chain_out[k] = j.chain_cols[k];
  return true;
}

// The chain's stages bottom-up (j.a.chain): each stage's key, table, filter operands and output columns (j.chain_cols) as references to base columns or to its own slice's.
bool Plan::resolve_chain(const ChainRequest& req, LdsJoin& j) {
  const NodeInfo& base = j.nd; std::vector<ColRef>& cur = j.chain_cols;
  cur.resize(base.n_proj);
  for (u32 k = 0; k < base.n_proj; k++) {
    const u32 col = base.proj[k];
    const bool from_left = col < j.L.n_cols;
    cur[k] = ColRef{from_left ? j.L.cols[col] : j.R.cols[col - j.L.n_cols], (from_left == j.build_left) ? 1u : 0u, 0u};
  }
  j.stage_bytes = 0;
  for (size_t t = 0; t < req.links.size(); t++) {
    const ChainLink& ln = req.links[t];
    const NodeInfo& N = *ln.node;
    const u32 wl = nodes[N.d.left].width;
    const u32 prev_w = ln.slice_is_left ? nodes[N.d.right].width : wl;
    if (prev_w != cur.size()) return false;
    bool bad = false;
    auto resolve = [&](u32 col) -> ColRef {
      const bool in_left = col < wl; const u32 local = in_left ? col : col - wl;
      if (in_left == ln.slice_is_left) { if (local >= ln.slice.n_cols) { bad = true; return ColRef{}; } return ColRef{ln.slice.cols[local], 2u + (u32)t, 0u}; }
      if (local >= cur.size()) { bad = true; return ColRef{}; }
      return cur[local];
    };
    ChainStage& st = j.a.chain[t]; std::memset(&st, 0, sizeof st);
    const u32 prev_key = ln.slice_is_left ? N.d.right_keys[0] : N.d.left_keys[0];
    if (prev_key >= cur.size()) return false;
    st.key = cur[prev_key];
    if (st.key.src > 1) return false;                       // the kernel looks a stage up from a BASE column
    st.direct = ln.table->direct; st.kmin = ln.table->kmin; st.kn = ln.table->kn;
    u32 n_fcols = 0;
    if (N.prog.n == 0) st.fs = 0;
    else if (N.shape == 2) {
      st.fs = 2; n_fcols = 2;
      st.f[0] = resolve(N.prog.nodes[0].u); st.f[1] = resolve(N.prog.nodes[1].u);
      st.is_eq = N.prog.nodes[2].op == RDFGPU_EX_ID_EQ;
    } else if (N.shape == 3) {
      const rdfgpu_expr_node* e = N.prog.nodes;
      st.fs = 3; n_fcols = 4;
      st.f[0] = resolve(e[0].u); st.f[1] = resolve(e[2].u); st.f[2] = resolve(e[8].u); st.f[3] = resolve(e[10].u);
      st.l0 = window_literal(e, 0); st.l1 = window_literal(e, 8);
    } else return false;
    for (u32 q = 0; q < n_fcols; q++) if (st.f[q].src > 1 && st.f[q].src != 2u + (u32)t) return false;   // base columns or this stage's
    // integer window whose x operand is a column of this stage's slice and whose y operands are base columns: use the slice's decoded value table
    if (st.fs == 3 && st.f[0].src == 2u + (u32)t && st.f[2].src == st.f[0].src && st.f[2].ptr == st.f[0].ptr && st.f[1].src <= 1 && st.f[3].src <= 1 &&
        !opt.on(RDFGPU_OPT_NO_VALUE_TABLES)) {
      const SliceTable::ValueColumn vc = slice_value_column(ln, st.f[0].ptr);
      if (vc.usable) { st.val = vc.val; j.chain_vc[t] = vc; }
    }
    std::vector<ColRef> next(N.n_proj);
    for (u32 k = 0; k < N.n_proj; k++) next[k] = resolve(N.proj[k]);
    if (bad) return false;
    cur.swap(next);
    j.stage_bytes += base.last_rows * (8ull + 4ull * n_fcols);   // per candidate: key + table slot + filter operands (estimate)
  }
  return cur.size() == req.top->n_proj && cur.size() <= (size_t)kMaxCols;
}

// The decoded value table of column `col` of a chain link's slice: found (one entry per column: pushed only after a failed look-up under the same lock) or built now, once per store version.  A copy: the list may grow.
SliceTable::ValueColumn Plan::slice_value_column(const ChainLink& ln, const u32* col) {
  SliceTable* tab = const_cast<SliceTable*>(ln.table);
  std::unique_lock<std::mutex> building(store->slice_build_mu);
  for (const auto& v : tab->values) if (v.col == col) return v;
  const u32 key_local = ln.slice_is_left ? ln.node->d.left_keys[0] : ln.node->d.right_keys[0];
  long long* val = store->table_alloc<long long>(tab->kn); metrics.tables_built++;
  u32* bad = reinterpret_cast<u32*>(new_counter());
  launch_fill_i64(val, INT64_MIN, tab->kn, stream);
  launch_direct_values(ln.slice.cols[key_local], col, ln.slice.cap, tab->kmin, tab->kn, typed_table(), val, bad, stream);
  if (read_back<u32>(bad)) { store->table_free(val); val = nullptr; }
  SliceTable::ValueColumn fresh{col, val, val != nullptr};
  if (val) {   // value range: the bias of the band join's 32-bit window intervals
    long long got[2]; device_minmax_i64(got, [&](long long* mm) { launch_val_minmax(val, tab->kn, mm, stream); });
    fresh.vmin = got[0]; fresh.vmax = got[1];
  }
  tab->values.push_back(fresh);
  return fresh;
}

// Band join (band_join.hip): when the groups of the CSR base are small, every stage hangs off a BUILD column and the stage filters are integer windows between a stage value
// and probe columns, the chain runs group by group — both sides partitioned by the key, the pair tests in registers — instead of probe row by probe row.  true: j.band is filled.
bool Plan::chain_band_args(const ChainRequest& req, LdsJoin& j) {
  const LdsJoinArgs& a = j.a; BandArgs b{};
  if (!a.csr_off || !j.slice || opt.on(RDFGPU_OPT_NO_BAND_JOIN) || arg_slots_used >= ExecContext::kArgSlots) return false;
  if (a.n_keys != 1 || (a.has_filter != 0 && a.has_filter != 2) || a.has_probe_filter != 0 || a.visited != nullptr) return false;
  if (a.has_filter == 2) {
    const bool ab = on_build_side(a, a.idp.a), bb = on_build_side(a, a.idp.b);
    if (ab == bb) return false;
    b.has_neq = 1; b.neq_is_eq = a.idp.is_eq; b.neq_build = a.cols[ab ? a.idp.a : a.idp.b]; b.neq_probe = a.cols[ab ? a.idp.b : a.idp.a];
  }
  if (a.has_post) {
    if (!on_build_side(a, a.post.col)) return false;
    b.has_post = 1; b.post_col = a.cols[a.post.col]; b.post_lit = a.post.lit; b.post_is_eq = a.post.is_eq;
  }
  b.n_stages = (u32)req.links.size();
  bool pack16 = !opt.on(RDFGPU_OPT_NO_BAND_PACK16);
  for (size_t t = 0; t < req.links.size(); t++) {
    const ChainStage& st = a.chain[t];
    if (st.key.src != 1 || (st.fs != 0 && st.fs != 3)) return false;
    b.stage[t] = BandStage{st.key.ptr, st.direct, st.kmin, st.kn};
    if (st.fs == 0) continue;
    const SliceTable::ValueColumn& vc = j.chain_vc[t];
    if (st.val == nullptr || b.n_win >= 2 || st.f[1].src != 0 || st.f[3].src != 0 || !range_op(st.l0.cmp_op) || !range_op(st.l1.cmp_op) ||
        vc.vmin > vc.vmax || (unsigned long long)vc.vmax - (unsigned long long)vc.vmin >= 0xFFFFFFE0ull) return false;   // (unsigned: the spread of two i64 may exceed i64)
    BandWin& w = b.win[b.n_win++];
    if ((unsigned long long)vc.vmax - (unsigned long long)vc.vmin > 65530ull) pack16 = false;   // biased values 1 .. range + 1 have to fit 16 bits
    w.key_col = st.key.ptr; w.val = st.val; w.vkmin = st.kmin; w.vkn = st.kn; w.vbase = vc.vmin;
    w.y0 = st.f[1].ptr; w.y1 = st.f[3].ptr; w.l0 = st.l0; w.l1 = st.l1; w.stage = (u32)t;
  }
  b.pack16 = pack16 ? 1u : 0u;
  for (size_t k = 0; k < j.chain_cols.size(); k++) {
    const ColRef& col = j.chain_cols[k];
    if (col.src == 0 ? b.n_row_cols >= kBandMaxRowCols : b.n_entry_cols >= kBandMaxSideCols) return false;
    if (col.src == 0) { b.out_from_row[k] = 1; b.out_sel[k] = (u8)b.n_row_cols; b.row_col[b.n_row_cols++] = col.ptr; }
    else { b.out_from_row[k] = 0; b.out_sel[k] = (u8)(2 + b.n_entry_cols); b.entry_col[b.n_entry_cols++] = col; }
  }
  // group sizes: the largest decides (one wave joins a whole group)
  if (csr_max_group(j.slice, a) > kBandMaxGroup || j.B.cap < 4ull * a.direct_n || j.P.cap * 4 < a.direct_n || j.P.cap >= (1ull << 31)) return false;
  j.band = b;
  return true;
}

// Rows of the largest group of a slice's CSR table: measured once per table, under the lock.
u32 Plan::csr_max_group(SliceTable* tab, const LdsJoinArgs& a) {
  std::unique_lock<std::mutex> building(store->slice_build_mu);
  if (tab->csr_max_group) return tab->csr_max_group;
  u32* mx = reinterpret_cast<u32*>(new_counter());
  launch_csr_max_group(a.csr_off, a.direct_n, mx, stream);
  return tab->csr_max_group = std::max(1u, read_back<u32>(mx));
}

// Range index: a CSR base whose first stage `s0` is an integer window (GT / LT / GEQ / LEQ) between the stage's decoded value and probe-side columns expands, per probe row,
// only the part of the key's group whose value can pass — the group is kept sorted by that value (found on the CSR table or built now, once per store version, under the lock).
void Plan::chain_range_index(LdsJoin& j, const ChainStage& s0) {
  LdsJoinArgs& a = j.a;
  if (!a.csr_off || !j.slice || !s0.val || s0.fs != 3 || s0.key.src != 1 || s0.f[1].src != 0 || s0.f[3].src != 0 ||
      !range_op(s0.l0.cmp_op) || !range_op(s0.l1.cmp_op) || opt.on(RDFGPU_OPT_NO_RANGE_INDEX)) return;
  std::unique_lock<std::mutex> building(store->slice_build_mu);
  SliceTable::RangeIndex* ri = nullptr;
  for (auto& r : j.slice->ranges) if (r.val == s0.val && r.link_col == s0.key.ptr) ri = &r;
  if (!ri) {
    SliceTable::RangeIndex fresh{s0.val, s0.key.ptr, nullptr, nullptr, 0, nullptr, false};
    const u64 n = j.B.cap;
    long long got[2]; device_minmax_i64(got, [&](long long* mm) { launch_range_minmax(s0.key.ptr, a.csr_rows, n, s0.val, s0.kmin, s0.kn, mm, stream); });
    if (got[0] <= got[1] && (unsigned long long)got[1] - (unsigned long long)got[0] < 0xFFFFFFF0ull && n < (1ull << 32)) {
      u64* key_in = scratch<u64>(n); u64* key_out = scratch<u64>(n); u32* rows_in = scratch<u32>(n);
      fresh.rows = store->table_alloc<u32>(n); fresh.vals = store->table_alloc<u32>(n);
      metrics.tables_built++; fresh.vbase = got[0];
      launch_range_keys(a.build_key[0], a.direct_min, s0.key.ptr, a.csr_rows, n, s0.val, s0.kmin, s0.kn, got[0], key_in, rows_in, stream);
      const size_t tb = sort_temp_bytes(n); void* temp = scratch<unsigned char>(tb);
      sort_pairs_u64_u32(key_in, key_out, rows_in, fresh.rows, n, temp, tb, stream);
      launch_range_decode(key_out, n, fresh.vals, stream);
      fresh.link = store->table_alloc<u32>(n);
      launch_gather_u32(s0.key.ptr, fresh.rows, fresh.link, n, stream);   // the link column in index order
      RDFGPU_HIP(hipStreamSynchronize(stream)); metrics.host_syncs++;
      fresh.usable = true;
    }
    j.slice->ranges.push_back(fresh);
    ri = &j.slice->ranges.back();
  }
  if (ri->usable) { a.range_rows = ri->rows; a.range_vals = ri->vals; a.range_vbase = ri->vbase; a.range_link = ri->link; a.range_link_col = ri->link_col; }
}

// The fused chain as a key-partitioned band join (band_join.hip).  j.a is complete (chain, output columns, out_cap, counters), j.band holds what apply_chain
// resolved; everything allocated here is scratch of this execution.  Bytes recorded per kernel = what that kernel has to move once (compulsory).  The route flags
// (BandJoin says what each means) and the step's form are all set here, before the first launch; in_place alone has to wait for band_slice_tables, which finds or builds the layout it needs.
void Plan::exec_band_join(LdsJoin& j) {
  BandJoin bj(j);
  BandHistory& hist = j.nd.band; const DevTable& P = j.P; const bool ordered = !opt.on(RDFGPU_OPT_NO_ORDERED_JOIN);
  bj.presorted = ordered && P.sorted_col >= 0 && P.cols[P.sorted_col] == j.a.probe_key[0] && P.key_min >= std::max<u32>(1u, j.a.direct_min);
  bj.skip_slow = speculative && hist.ran && hist.slow_rows == 0;   // a row that needs the pass after all is caught at the end of the plan like any failed speculation
  const u64 runs_seen = hist.run_stats & 0xFFFFFFFFull, run_rows = hist.run_stats >> 32;
  bj.counting = !bj.presorted && ordered && (bj.np <= (1ull << 21) || (runs_seen && run_rows >= 4 * runs_seen));
  bj.cache_entries = j.B.stable_id != 0 && !opt.on(RDFGPU_OPT_NO_TABLE_CACHE);
  // the packed pair test reads 8 bytes of window, the id operand and at most one output value per row: 16 bytes per row instead of 32 whenever no full-semantics pass will want the flags
  j.band.compact = (j.band.pack16 && j.band.n_row_cols <= 1 && bj.skip_slow && !opt.on(RDFGPU_OPT_NO_BAND_COMPACT)) ? 1u : 0u;
  bj.fused = take_pending_oj(bj);     // not fused: that join's write pass has run by now
  hist.takes_records = bj.presorted && bj.skip_slow && ordered;
  band_probe_side(bj);
  band_slice_tables(bj);
  hist.in_place = bj.lay.boff != nullptr;   // the layout exists: next time the ordered join below may leave its matches uncounted
  // In place: the ordered join below skipped its count pass, and the slice it streamed IS this join's build side.  Anything else counts the matches now and compacts them (the write-band pass).
  hist.row_cache = bj.rw.row_win != nullptr;   // .. and its probe pass may prepare the values by key instead of the 16-byte records
  // (the ordered join prepared what the last execution's flags said: values by key when the windows were cached — it then owes its probe pass, PendingOj::probe_owed —, records by
  // key otherwise; a step whose cached windows are gone, a non-integer operand having entered the store, counts and compacts once, behind the full probe pass: count_pending_oj)
  BandStepShape step;
  step.row_static = bj.fused && bj.rw.row_win && pending_oj.o.key_val;
  bj.in_place = bj.fused && !pending_oj.counted && bj.fuse.self_index && hist.in_place && (step.row_static || pending_oj.o.key_rec);
  step.row_static = step.row_static && bj.in_place;   // (implies skip_slow: the full-semantics pass, which patches the bits, never runs over the slice's)
  step.has_verdicts = bj.rw.pair_bits != nullptr; step.has_list = bj.rw.pair_list != nullptr; step.n_row_cols = j.band.n_row_cols; step.n_blocks = bj.lay.n_blocks;
  step.list_option_off = !opt.on(RDFGPU_OPT_NO_BAND_PAIR_LIST); step.counts_option_off = !opt.on(RDFGPU_OPT_NO_BAND_PAIR_COUNTS); step.min_blocks = opt.v[RDFGPU_OPT_BAND_PAIR_COUNT_BLOCKS];
  bj.form = band_step_form(step);
  if (bj.fused && !bj.in_place) count_pending_oj();
  band_row_records(bj);
  band_blocks_and_emit(bj);
}

// The probe side is the held-back output of an ordered slice join (Plan::pending_oj).  true: everything this join reads of it travels in that join's packed
// table record and its key is the slice's sorted column, so that join writes this join's row records itself (bj.fuse).  Otherwise its write pass runs now.
bool Plan::take_pending_oj(BandJoin& bj) {
  if (!pending_oj.active) return false;
  const LdsJoinArgs& a = bj.j.a; const DevTable& B = bj.j.B; const DevTable& P = bj.j.P; BandArgs& b = bj.j.band; OjBandFuse& fuse = bj.fuse; const OrderedJoinArgs& o = pending_oj.o;
  bool ok = bj.presorted && bj.skip_slow && P.cols[0] == pending_oj.first_col && P.n_cols == o.n_out_cols;
  auto slot_of = [&](const u32* col, u8& slot) {      // the word of the packed record that holds output column `col`
    slot = 0xFFu;
    for (u32 c = 0; c < o.n_out_cols; c++) if (o.out[c] == col && o.out_slot[c] != 0xFFu) { slot = o.out_slot[c]; return true; }
    return false;
  };
  fuse.y0_slot[0] = fuse.y0_slot[1] = fuse.y1_slot[0] = fuse.y1_slot[1] = fuse.neq_slot = fuse.row_slot[0] = fuse.row_slot[1] = 0xFFu;
  for (u32 w = 0; ok && w < b.n_win; w++) ok = slot_of(b.win[w].y0, fuse.y0_slot[w]) && slot_of(b.win[w].y1, fuse.y1_slot[w]);
  if (ok && b.has_neq) ok = slot_of(b.neq_probe, fuse.neq_slot);
  for (u32 u = 0; ok && u < b.n_row_cols; u++) ok = slot_of(b.row_col[u], fuse.row_slot[u]);
  for (u32 c = 0; ok && c < o.n_out_cols; c++) if (o.out[c] == a.probe_key[0] && o.out_slot[c] == 0xFFu && o.out_ref[c].src == 1) fuse.key_col = o.out_ref[c].ptr;
  if (!ok || fuse.key_col == nullptr) { flush_pending_oj(); return false; }
  fuse.compact = b.compact;   // (16 bytes per match instead of 32)
  // self_index, `entry id != row id` by entry index: the band join's groups are the rows of the very slice the ordered join streamed (same sorted column, same rows, identity CSR),
  // the entry's id is that join's build key, the row's id its probe key — equal keys are what made the match, and a store slice holds every (key, sorted column) pair once:
  // the only entry of the group whose id equals the row's is the slice row the match came from
  if (fuse.compact && b.has_neq && !b.neq_is_eq && a.csr_rows == nullptr && a.build_key[0] == fuse.key_col && B.cap == pending_oj.n_build &&
      b.neq_build == o.build_key && B.stable_id != 0 && !opt.on(RDFGPU_OPT_NO_BAND_COMPACT))
    for (u32 c = 0; c < o.n_out_cols; c++)
      if (o.out[c] == b.neq_probe && o.out_slot[c] != 0xFFu && o.out_ref[c].src == 0 && o.out_ref[c].ptr == o.probe_key) fuse.self_index = 1;
  b.neq_self = fuse.self_index;
  return true;
}

// The kernel arguments that repeat the LDS join's (table, probe side, output), and what partitions the probe rows by the key: the counting
// sort's key histogram or the radix sort's pairs and temp, the unsorted rows' records, the two counts the row passes leave behind.
void Plan::band_probe_side(BandJoin& bj) {
  const LdsJoinArgs& a = bj.j.a; BandArgs& b = bj.j.band;
  if (bj.counting) {
    b.key_hist = scratch<u32>((u64)bj.kn + 2); b.key_cursor = scratch<u32>((u64)bj.kn + 2);
    RDFGPU_HIP(hipMemsetAsync(b.key_hist, 0, ((size_t)bj.kn + 2) * sizeof(u32), stream));
  }
  b.presorted = bj.presorted ? 1u : 0u; b.tt = a.tt;
  b.csr_off = a.csr_off; b.csr_rows = a.csr_rows; b.kmin = a.direct_min; b.kn = bj.kn; b.n_entries = bj.nb;
  b.probe_key = a.probe_key[0]; b.n_probe_dev = bj.j.P.n_dev; b.n_probe_cap = bj.np;
  b.n_out_cols = a.n_out_cols; b.out_cap = a.out_cap; b.n_out_dev = a.n_out_dev; b.overflow = a.overflow; for (u32 c = 0; c < a.n_out_cols; c++) b.out[c] = a.out[c];
  b.skey = bj.skey = scratch<u32>(bj.np); b.perm = bj.perm = scratch<u32>(bj.np);
  if (bj.presorted) { b.skey_in = bj.skey; b.sval_in = bj.perm; b.rec = nullptr; }
  else { b.skey_in = scratch<u32>(bj.np); b.sval_in = scratch<u32>(bj.np); b.rec = scratch<uint4>((b.compact ? 1 : 2) * bj.np); }
  b.slow_rows = reinterpret_cast<u32*>(new_counter()); b.run_stats = reinterpret_cast<unsigned long long*>(new_counter());
  while ((1ull << bj.sort_bits) <= bj.kn) bj.sort_bits++;            // keys 0 .. kn (kn = joins nothing)
  bj.sort_temp_bytes = sort_u32_temp_bytes(bj.np, bj.sort_bits); bj.sort_temp = scratch<unsigned char>(bj.sort_temp_bytes);
}

// The two tables a band join keeps on its build slice's SliceTable (per store version, like every other join table): found or built under
// ONE hold of the lock, taken only when they are kept at all; each is published only once the stream has been waited for, and the layout is
// copied before the lock goes.  bj.ekey: the bytes the decoded entries depend on, the store's slices and the chain's constants.
void Plan::band_slice_tables(BandJoin& bj) {
  const BandArgs& b = bj.j.band;
  auto put = [&](const void* p, size_t n) { bj.ekey.append(reinterpret_cast<const char*>(p), n); };
  put(&b.csr_off, sizeof b.csr_off); put(&b.csr_rows, sizeof b.csr_rows); put(&b.kmin, 4); put(&b.kn, 4); put(&b.n_stages, 4); put(&b.n_win, 4);
  for (u32 t = 0; t < b.n_stages; t++) put(&b.stage[t], sizeof(BandStage));
  for (u32 w = 0; w < b.n_win; w++) { put(&b.win[w].key_col, sizeof(void*)); put(&b.win[w].val, sizeof(void*)); put(&b.win[w].vkmin, 4); put(&b.win[w].vkn, 4); put(&b.win[w].vbase, 8); }
  put(&b.has_post, 4); put(&b.post_lit, 4); put(&b.post_is_eq, 4); put(&b.post_col, sizeof(void*)); put(&b.has_neq, 4); put(&b.neq_build, sizeof(void*));
  put(&b.n_entry_cols, 4); for (u32 u = 0; u < b.n_entry_cols; u++) { put(&b.entry_col[u].ptr, sizeof(void*)); put(&b.entry_col[u].src, 4); }
  put(&bj.nb, 8);
  std::unique_lock<std::mutex> building(store->slice_build_mu, std::defer_lock);
  if (bj.cache_entries) building.lock();
  band_entries(bj);
  if (const SliceTable::BandEntries* layout = band_layout(bj)) bj.lay = *layout;
  band_row_windows(bj);
}

// The build side's decoded entries (the pair test's operands, the entries' output values), found on the slice's table (keys are unique there: an entry is
// pushed only after a failed look-up under the same lock) or built: a steady-state step does not decode 5.4 M build rows again.  The caller holds the lock when bj.cache_entries.
void Plan::band_entries(BandJoin& bj) {
  const LdsJoinArgs& a = bj.j.a; BandArgs& b = bj.j.band; SliceTable* tab = bj.j.slice;
  if (bj.cache_entries) for (const auto& e : tab->band_entries) if (e.key == bj.ekey) { b.et = e.et; for (u32 u = 0; u < b.n_entry_cols; u++) b.eo[u] = e.eo[u]; return; }
  // stages all keyed by one build column: their look-ups once per distinct key value instead of once per entry
  const u32* kc = a.n_chain ? b.stage[0].key_col : nullptr;
  bool same = kc != nullptr; u64 lo = ~0ull, hi = 0;
  for (u32 t = 0; t < b.n_stages; t++) { same = same && b.stage[t].key_col == kc; lo = std::min<u64>(lo, b.stage[t].kmin); hi = std::max<u64>(hi, (u64)b.stage[t].kmin + b.stage[t].kn); }
  for (u32 w = 0; w < b.n_win; w++) same = same && b.win[w].key_col == kc;
  if (same && hi > lo && hi - lo <= (64ull << 20) && hi - lo <= 8 * bj.nb + 1024) {
    b.pt_min = (u32)lo; b.pt_n = (u32)(hi - lo); b.pt_key_col = kc; b.pt = scratch<uint4>(2ull * b.pt_n);
    timed(KC_BAND_PT, 0, b.pt_n, nullptr, 4ull * b.n_stages + 8ull * b.n_win + 4ull * b.n_entry_cols + 32, nullptr, 0, 0, [&] { launch_band_pt(b, stream); });
  }
  // the build side, once: per row its columns + stage look-ups read, 16 B of operands + the output values written
  u64 entry_bytes = 4ull * (1 + bj.j.build_payload) + (a.csr_rows ? 4 : 0) + (a.has_post ? 4 : 0);
  for (u32 t = 0; t < a.n_chain; t++) entry_bytes += 4 + (a.chain[t].val ? 8 : 0);
  const bool own_entries = bj.cache_entries && tab->band_entries.size() < 8;   // kept on the slice, else scratch of this execution
  b.et = own_entries ? store->table_alloc<uint4>(bj.nb + 64) : scratch<uint4>(bj.nb + 64);   // padded: the pair test reads whole groups of 8 entries
  for (u32 u = 0; u < b.n_entry_cols; u++) b.eo[u] = own_entries ? store->table_alloc<u32>(bj.nb) : scratch<u32>(bj.nb);
  timed(KC_BAND_ENTRIES, 0, bj.nb, bj.j.B.n_dev, entry_bytes + 4ull * b.n_entry_cols + 16 + 4ull * b.n_entry_cols, nullptr, 0, 0, [&] { launch_band_entries(b, stream); });
  if (own_entries) {   // publish only when complete
    RDFGPU_HIP(hipStreamSynchronize(stream)); metrics.host_syncs++; metrics.tables_built++;
    SliceTable::BandEntries e{bj.ekey, b.et, {nullptr, nullptr, nullptr, nullptr}};
    for (u32 u = 0; u < b.n_entry_cols; u++) e.eo[u] = b.eo[u];
    tab->band_entries.push_back(e);
  }
}

// In place: the band join's rows of key k are the CSR group k itself (poff = csr_off), so its blocks depend on the slice alone — laid out once per store version beside the
// entries (same key, same lock), their exact number read back, published when complete; by the first execution that could take the route, so that the first one that does finds
// them.  The route pays for every slice row, matched or not, and for ceil(E/64)² blocks per key: it is taken when the ordered join's last measured rows cover at least half of the
// slice, and when the block count, bounded here in 64 bits (sum over keys of ceil(E/64)² <= cmax · (rows / 64 + keys)), stays below 2^31 — the device counts in 32.
// Null: the route is not available (entries that could not be cached among the reasons: the counted route); a layout returned has its boff.
SliceTable::BandEntries* Plan::band_layout(BandJoin& bj) {
  const LdsJoinArgs& a = bj.j.a; const u32 kn = bj.kn;
  SliceTable::BandEntries* layout = nullptr;
  if (bj.fused && bj.fuse.self_index && bj.cache_entries && bj.cmax * (bj.nb / 64 + kn) < (1ull << 31) && pending_oj.rows_seen * 2 >= bj.nb)
    for (auto& e : bj.j.slice->band_entries) if (e.key == bj.ekey) layout = &e;
  if (layout && !layout->boff) {
    u32* boff = store->table_alloc<u32>((u64)kn + 1);
    const size_t tb = band_blocks_scan_temp_bytes(kn); void* temp = scratch<unsigned char>(tb);
    timed(scan_class((u64)kn + 1), 12ull * kn, (u64)kn + 1, nullptr, 4, nullptr, 0, 0, [&] { band_blocks_scan(a.csr_off, a.csr_off, kn, boff, temp, tb, stream); });
    const u32 n = read_back<u32>(boff + kn);
    BandArgs d = bj.j.band; d.poff = const_cast<u32*>(a.csr_off); d.boff = boff; d.bdesc = store->table_alloc<uint4>(n); d.max_blocks = n; d.n_blocks_out = nullptr;
    timed(KC_BAND_DESC, 12ull * kn, 0, nullptr, 0, nullptr, 0, 0, [&] { launch_band_desc(d, stream); });
    RDFGPU_HIP(hipStreamSynchronize(stream)); metrics.host_syncs++;
    layout->boff = boff; layout->bdesc = d.bdesc; layout->n_blocks = n; metrics.tables_built++;
  }
  return layout;
}

// In place, the ROW side of the pair test as tables of the slice (SliceTable::BandRowWindows; at most 8 entries per slice, beside the entries: same lock, which the caller holds —
// the layout exists only when bj.cache_entries).  Three tiers, each behind the one before: the rows' WINDOWS, when both operands of every window are reached from the ordered
// join's key alone (band_row_operands); the pair test's VERDICTS over them (host_logic.hpp: band_pair_cache_eligible); the LIST of the verdicts' set bits with its per-row
// counts (band_pair_list_eligible).  One path: the entry is found or started, the tiers it lacks and this plan's options want are launched behind one another, waited for
// once — no wait when nothing is built — and published only then; a fresh entry is one that lacks all three.  A store in which some key's operands are not plain xsd:integers
// declines the windows: remembered as an entry without tables, everything built behind them freed.  The step is handed what this plan's options accept (bj.rw).
void Plan::band_row_windows(BandJoin& bj) {
  std::vector<SliceTable::BandRowWindows>& kept = bj.j.slice->band_row_windows;
  if (!bj.lay.boff) return;                              // the in-place route is closed
  BandRowWinArgs w{};
  if (!band_row_operands(bj, w)) return;
  std::string key = band_row_win_key(bj, w);
  SliceTable::BandRowWindows fresh, *e = &fresh;
  for (auto& x : kept) if (x.key == key) e = &x;
  if (e == &fresh && kept.size() >= 8) return;
  const BandRowTiers t = band_row_tiers(bj, *e, e == &fresh);
  // one counter pair for the one wait: {keys declined, survivors} (the windows exist: the first half stays 0)
  u32* const count = t.build_windows || t.build_list ? reinterpret_cast<u32*>(new_counter()) : nullptr;
  uint2* const row_win = t.build_windows ? build_row_win(bj, w, count) : e->row_win;
  u64* const bits = t.build_verdicts ? build_pair_bits(bj, row_win) : e->pair_bits;
  BandPairListArgs la{};
  if (t.build_list) la = build_pair_list(bj, bits, count + 1);
  uint2 got = make_uint2(0u, 0u);
  if (count) got = read_back<uint2>(count);
  else if (t.build_verdicts) { RDFGPU_HIP(hipStreamSynchronize(stream)); metrics.host_syncs++; }
  const bool declined = got.x != 0;                      // (only a fresh entry's windows can be: whatever was built, was built behind them)
  if (declined) { store->table_free(row_win); store->table_free(bits); }
  else {
    if (t.build_windows) { e->row_win = row_win; metrics.tables_built++; }
    if (t.build_verdicts) { e->pair_bits = bits; metrics.tables_built++; }
  }
  if (t.build_list && !declined && band_pair_list_eligible(BandPairListShape{true, true, got.y, bj.lay.n_blocks})) {   // kept when it meets the condition (the counts are no table of their own)
    e->pair_list = la.list; e->pair_list_off = const_cast<u32*>(la.off); e->pair_cnt = la.pair_cnt; e->pair_survivors = got.y; metrics.tables_built++;
  } else if (t.build_list) {                             // larger than its bound: freed, and not built again
    store->table_free(la.list); store->table_free(const_cast<u32*>(la.off)); store->table_free(la.pair_cnt); e->list_declined = !declined;
  }
  if (e == &fresh) { fresh.key = std::move(key); kept.push_back(fresh); e = &kept.back(); }
  bj.rw.row_win = e->row_win;                            // (a plan whose options decline a tier does not use one another plan left)
  if (t.use_verdicts) bj.rw.pair_bits = e->pair_bits;
  if (t.use_list && e->pair_list) { bj.rw.pair_list = e->pair_list; bj.rw.pair_list_off = e->pair_list_off; bj.rw.pair_cnt = e->pair_cnt; bj.rw.pair_survivors = e->pair_survivors; }
}

// The window operands as the ordered join below reaches them (w.y0, w.y1: the stage's direct table and the column), and whether their shape lets the rows' windows be
// a table of the slice (host_logic.hpp, band_row_cache_eligible).
bool Plan::band_row_operands(const BandJoin& bj, BandRowWinArgs& w) {
  const BandArgs& b = bj.j.band; const OjBandFuse& fuse = bj.fuse; const OrderedJoinArgs& o = pending_oj.o;
  BandRowCacheShape shape;
  shape.in_place = true; shape.compact = fuse.compact != 0 && b.compact != 0; shape.pack16 = b.pack16 != 0;
  shape.option_off = !opt.on(RDFGPU_OPT_NO_BAND_ROW_CACHE); shape.n_win = b.n_win;
  auto operand = [&](u8 slot, BandRowOperand& op, BandRowOperandShape& sh) {   // the ordered join's output column held in word `slot` of its packed record
    for (u32 c = 0; c < o.n_out_cols; c++) {
      if (slot == 0xFFu || o.out_slot[c] != slot) continue;
      const ColRef ref = o.out_ref[c];
      sh.src = ref.src;
      if (ref.src >= 2 && ref.src - 2 < o.n_stages) {
        const OrderedJoinStage& st = o.stage[ref.src - 2];
        sh.stage_keyed_by_join_key = st.key_col == o.probe_key;
        op = BandRowOperand{st.direct, st.kmin, st.kn, ref.ptr};
      }
      return;
    }
  };
  for (u32 k = 0; k < b.n_win && k < 2; k++) { operand(fuse.y0_slot[k], w.y0[k], shape.y0[k]); operand(fuse.y1_slot[k], w.y1[k], shape.y1[k]); }
  return band_row_cache_eligible(shape);
}

// The key of a slice's BandRowWindows entry: the entries' key + everything band_row_record reads.
std::string Plan::band_row_win_key(const BandJoin& bj, const BandRowWinArgs& w) {
  const BandArgs& b = bj.j.band; const OrderedJoinArgs& o = pending_oj.o;
  std::string key = bj.ekey;
  auto put = [&](const void* p, size_t n) { key.append(reinterpret_cast<const char*>(p), n); };
  for (u32 k = 0; k < b.n_win; k++) {
    put(&b.win[k].l0, sizeof(TvLiteral)); put(&b.win[k].l1, sizeof(TvLiteral)); put(&b.win[k].vbase, 8);
    for (const BandRowOperand* op : {&w.y0[k], &w.y1[k]}) { put(&op->direct, sizeof(void*)); put(&op->kmin, 4); put(&op->kn, 4); put(&op->val, sizeof(void*)); }
  }
  put(&b.pack16, 4); put(&b.has_neq, 4); put(&b.tt.tv, sizeof(void*)); put(&b.tt.n_ids, sizeof b.tt.n_ids);
  put(&o.build_key, sizeof(void*)); put(&o.kmin, 4); put(&o.kn, 4);
  return key;
}

// Which tiers of entry `e` this plan's options accept, and which of those it lacks.  A plan that wants a tier an earlier plan declined to build, builds it then.
BandRowTiers Plan::band_row_tiers(const BandJoin& bj, const SliceTable::BandRowWindows& e, bool fresh) {
  const BandArgs& b = bj.j.band; BandRowTiers t;
  BandPairCacheShape pair;
  pair.row_windows = fresh || e.row_win != nullptr;      // (fresh: whether the store's operands accept the windows is known only after the wait — built behind them, freed if not)
  pair.neq_self = b.neq_self != 0; pair.pack16 = b.pack16 != 0; pair.option_off = !opt.on(RDFGPU_OPT_NO_BAND_PAIR_CACHE);
  pair.n_blocks = bj.lay.n_blocks; pair.cap = opt.v[RDFGPU_OPT_BAND_PAIR_CACHE_BLOCKS];
  t.use_verdicts = band_pair_cache_eligible(pair);
  BandPairListShape list;                                // (survivors = 0: asked before the build, when only the layout is known)
  list.pair_cached = t.use_verdicts && bj.lay.n_blocks != 0; list.option_off = !opt.on(RDFGPU_OPT_NO_BAND_PAIR_LIST); list.n_blocks = bj.lay.n_blocks;
  t.use_list = band_pair_list_eligible(list);
  t.build_windows = fresh; t.build_verdicts = t.use_verdicts && !e.pair_bits; t.build_list = t.use_list && !e.pair_list && !e.list_declined;
  return t;
}

// The windows: per key two look-ups, two ids and two typed values per window read, 8 B written; per slice row its key read, 8 B gathered and written.  *declined = keys whose operands decline the form.
uint2* Plan::build_row_win(const BandJoin& bj, BandRowWinArgs& w, u32* declined) {
  const BandArgs& b = bj.j.band; const OrderedJoinArgs& o = pending_oj.o;
  w.kmin = o.kmin; w.kn = o.kn; w.by_key = scratch<uint2>(o.kn); w.slow_keys = declined;
  w.build_key = o.build_key; w.n_rows = bj.nb; w.row_win = store->table_alloc<uint2>(bj.nb + 64);
  timed(KC_BAND_ROW_WIN_KEYS, 0, o.kn, nullptr, 48ull * b.n_win + 8, nullptr, 0, 0, [&] { launch_band_row_win_keys(b, w, stream); });
  timed(KC_BAND_ROW_WIN_ROWS, 0, bj.nb, nullptr, 4 + 8 + 8, nullptr, 0, 0, [&] { launch_band_row_win_rows(w, stream); });
  return w.row_win;
}

// The verdicts: 512 B written per block; its descriptor, 64 entries and 64 rows' windows read.
u64* Plan::build_pair_bits(const BandJoin& bj, const uint2* row_win) {
  u64* bits = store->table_alloc<u64>(64ull * bj.lay.n_blocks);
  BandArgs d = bj.j.band; d.bdesc = bj.lay.bdesc; d.max_blocks = bj.lay.n_blocks; d.row_win = row_win; d.masks = bits;
  timed(KC_BAND_PAIR_BITS, (512ull + 16) * bj.lay.n_blocks + 16ull * bj.nb, bj.nb, nullptr, 8, nullptr, 0, 0, [&] { launch_band_pair_bits(d, stream); });
  return bits;
}

// The list of the verdicts' set bits: per block its 512 B of bits read twice, 64 B of per-row counts written, 4 B of count written and read, 4 B of offset written and read; 2 B per
// survivor written.  Its size is the condition's bound, 256 items per block, not a read-back: the write pass leaves a longer list unwritten, and the total (*total_out) travels with
// the wait that is there anyway.  pair_cnt is the list's companion: every word's own count, one more store of the count pass — no launch, no wait, no table of its own.
BandPairListArgs Plan::build_pair_list(const BandJoin& bj, const u64* bits, u32* total_out) {
  const u64 nbk = bj.lay.n_blocks; BandPairListArgs la{};
  la.bits = bits; la.n_blocks = (u32)nbk; la.counts = scratch<u32>(nbk + 1); la.cap = 256ull * nbk; la.total_out = total_out;
  u32* off = store->table_alloc<u32>(nbk + 1); la.off = off; la.list = store->table_alloc<unsigned short>(la.cap + 64);   // (padded: the emit pass reads whole rounds of 64 items)
  la.pair_cnt = store->table_alloc<u8>(64ull * nbk);
  const size_t tb = scan_temp_bytes(nbk + 1); void* temp = scratch<unsigned char>(tb);
  timed(KC_BAND_PAIR_LIST_COUNT, 0, nbk, nullptr, 512 + 4 + 64, nullptr, 0, 0, [&] { launch_band_pair_list_count(la, stream); });
  timed(scan_class(nbk + 1), 0, nbk + 1, nullptr, 8, nullptr, 0, 0, [&] { exclusive_scan_u32(la.counts, off, nbk + 1, temp, tb, stream); });
  timed(KC_BAND_PAIR_LIST_WRITE, 0, nbk, nullptr, 512 + 4 + 2 * 256, nullptr, 0, 0, [&] { launch_band_pair_list_write(la, stream); });
  return la;
}

// What the step's form reads (the table: band_join.hip), set here and nowhere else; a form leaves what it does not read null.  Everything is scratch of this
// execution but the slice's own tables, which a step reads and never writes.
void Plan::band_form_args(BandJoin& bj) {
  BandArgs& b = bj.j.band; const SliceTable::BandRowWindows& rw = bj.rw;
  b.row_win = nullptr; b.row_val = nullptr; b.masks = nullptr; b.bvalid = nullptr; b.pair_list = nullptr; b.pair_list_off = nullptr; b.pair_cnt = nullptr;
  if (bj.row_static()) { bj.fuse.key_val = pending_oj.o.key_val; bj.fuse.row_val = scratch<u32>(bj.nb); b.row_win = rw.row_win; b.row_val = bj.fuse.row_val; }
  switch (bj.form) {
    case BandForm::RECORDS: case BandForm::ROW_WINDOWS: b.masks = scratch<u64>(bj.max_blocks * 64); break;
    case BandForm::VERDICTS: b.masks = rw.pair_bits; b.bvalid = scratch<u64>(bj.max_blocks); break;
    case BandForm::VERDICTS_LIST: b.masks = rw.pair_bits; b.bvalid = scratch<u64>(bj.max_blocks); b.pair_list = rw.pair_list; b.pair_list_off = rw.pair_list_off; break;
    case BandForm::COUNTS_LIST: b.pair_cnt = rw.pair_cnt; b.pair_list = rw.pair_list; b.pair_list_off = rw.pair_list_off; break;
  }
}

// The bytes the two block passes have to move once in the step's form: the mask pass's fixed and per-row bytes, the emit pass's fixed bytes (per row and per output row it is the same in every form).
struct BandPassBytes { u64 mask_fixed, mask_row, emit_fixed; };
static BandPassBytes band_pass_bytes(const BandJoin& bj) {
  const BandArgs& b = bj.j.band; const u64 blocks = bj.max_blocks, entries = 4ull * b.n_entry_cols * bj.nb;
  const u64 list = 2ull * bj.rw.pair_survivors + 4ull * (blocks + 1);   // the list forms' emit pass: 2 B per survivor of the slice's list, 4 B per block + 4 of its offsets
  switch (bj.form) {
    // the pair test, per entry 16 B read, per pair one bit written (the pair count is not known on the host); per probe row 4 (sorted position) + 24 (record) read, compact: its 16 bytes
    case BandForm::RECORDS: return {16ull * bj.nb, b.compact ? 16ull : 4ull + 24, entries};
    case BandForm::ROW_WINDOWS: return {16ull * bj.nb, 8 + 4, entries};   // .. per row its cached windows and its value
    // the verdicts cached: per block its 512 B of bits and its descriptor read, 4 + 8 B of count and valid rows written; per row its value read
    case BandForm::VERDICTS: return {(512ull + 16 + 4 + 8) * blocks, 4, entries};
    case BandForm::VERDICTS_LIST: return {(512ull + 16 + 4 + 8) * blocks, 4, list + entries};
    // .. counted from the per-row counts: per block its 64 B of counts and its descriptor read, 4 B of count written; per row its value read
    case BandForm::COUNTS_LIST: return {(64ull + 16 + 4) * blocks, 4, list + entries};
  }
  fail(RDFGPU_ERR_INVALID, "band join: form %u", (u32)bj.form);
}

// The probe rows' records in key order, with the rows per key (poff) and the blocks' counts zeroed: written by the ordered slice join below (fused; in place: one per slice row), else decoded from the probe columns.
void Plan::band_row_records(BandJoin& bj) {
  const LdsJoinArgs& a = bj.j.a; BandArgs& b = bj.j.band; OjBandFuse& fuse = bj.fuse;
  const u32 kn = bj.kn; const u64 np = bj.np, nb = bj.nb; const bool in_place = bj.in_place, row_static = bj.row_static();
  bj.nrows = in_place ? nb : np; b.rec_s = row_static ? nullptr : scratch<uint4>(bj.nrows); b.aux_s = b.compact ? nullptr : scratch<uint4>(bj.nrows);
  b.poff = in_place ? const_cast<u32*>(a.csr_off) : scratch<u32>((u64)kn + 2);
  // blocks: sum over keys of ceil(E/64) * ceil(R/64) <= cmax * (rows / 64) + sum of ceil(E/64) over the keys
  bj.max_blocks = in_place ? bj.lay.n_blocks : bj.cmax * (np / 64 + 1) + nb / 64 + kn + 1;
  if (bj.max_blocks >= (1ull << 31)) fail(RDFGPU_ERR_UNSUPPORTED, "band join of %llu blocks", (unsigned long long)bj.max_blocks);
  b.max_blocks = (u32)bj.max_blocks; b.bcount = scratch<u32>(bj.max_blocks + 1); b.bofs = scratch<u32>(bj.max_blocks + 1);   // (bcount is zeroed by the decode / records pass: a memset is two more launches, ~10 us of launch gap each on this part; a row_static step has neither pass — its mask pass writes every block's count, its in-place pass the scan's closing zero)
  band_form_args(bj);
  // decode, per probe row: key + the window operands + the id operand read, 24 B of record + 8 B of sort pair written
  if (!bj.fused) return timed(KC_BAND_DECODE, 0, np, bj.j.P.n_dev, 4 + 4ull * (b.n_win + b.has_neq) + 9ull * b.n_win + 24 + 8, nullptr, 0, 0, [&] { launch_band_decode(b, stream); });
  const OrderedJoinArgs& o = pending_oj.o; pending_oj.active = false;
  fuse.key_rec = in_place && !row_static ? o.key_rec : nullptr;
  fuse.brec = in_place ? nullptr : scratch<uint4>((fuse.compact ? 1 : 2) * o.n_probe_cap);
  fuse.rec_s = b.rec_s; fuse.aux_s = b.aux_s; fuse.poff = b.poff; fuse.bcount = b.bcount; fuse.max_blocks = b.max_blocks; fuse.kmin = b.kmin; fuse.kn = b.kn;
  // per table row: its packed record read + two typed-value gathers + 32 B written; per slice row the count pass's 5 bytes + its key; per match a 32-byte record gathered and stored (in place: per slice row its key read, its key's 16-byte record gathered and stored)
  // (the rows' windows cached: per table row its packed record read and 4 B written by key; per slice row its key read, 4 B gathered, 4 B written)
  const u64 rec_bytes = fuse.compact ? 16 : 32;
  // An owed probe pass is settled here when the step reads the values by key (host_logic.hpp, oj_probe_form; a step that does not has had count_pending_oj run the full one): the fill of
  // key_val and the values-by-key pass in the place of the records pass.  Per table row: its key, per stage its key and its direct entry, the value read; 4 B exchanged by key.
  OjProbeShape owed = pending_oj.probe; owed.row_static = row_static;
  const OjProbeForm probe = pending_oj.probe_owed ? oj_probe_form(owed) : OjProbeForm::FULL;
  if (probe == OjProbeForm::FULL_NOW || (probe == OjProbeForm::FULL && row_static)) fail(RDFGPU_ERR_INVALID, "band join: a step of form %s over a probe pass of form %s", band_form_name(bj.form), oj_probe_form_name(probe));
  if (probe == OjProbeForm::LEAN) {
    pending_oj.probe_owed = false;
    fuse.slow_rows = b.slow_rows; fuse.val_ref = ColRef{nullptr, 0u, 0u};
    for (u32 c = 0; c < o.n_out_cols; c++) if (fuse.row_slot[0] != 0xFFu && o.out_slot[c] == fuse.row_slot[0]) fuse.val_ref = o.out_ref[c];
    if (fuse.val_ref.src == 1 || (fuse.val_ref.src >= 2 && fuse.val_ref.src - 2 >= o.n_stages)) fail(RDFGPU_ERR_INVALID, "band join: the row's value comes from source %u of the ordered join", fuse.val_ref.src);
    RDFGPU_HIP(hipMemsetAsync(fuse.key_val, 0xFF, (size_t)o.kn * sizeof(u32), stream));
    timed(KC_OJ_PROBE_VALUES, 0, o.n_probe_cap, o.n_probe_dev, 4 + 8ull * o.n_stages + (fuse.val_ref.ptr ? 4 : 0) + 4, nullptr, 0, 0, [&] { launch_ordered_join_probe(o, fuse, OjKeyValues{}, stream); });
  } else
  timed(KC_OJ_BAND_RECORDS, 0, o.n_probe_cap, o.n_probe_dev, row_static ? 16ull * o.n_rec + 4 : 16ull * o.n_rec + 9ull * b.n_win + rec_bytes, nullptr, 0, 0, [&] { launch_oj_band_records(o, b, fuse, stream); });
  if (in_place) timed(KC_OJ_WRITE_BAND_IN_PLACE, 0, nb, nullptr, row_static ? 4 + 4 + 4 : 4 + 2 * rec_bytes, nullptr, 0, 0, [&] { launch_ordered_join_write_band(o, fuse, OjInPlace{}, stream); });
  else timed(KC_OJ_WRITE_BAND, 0, pending_oj.n_build, nullptr, 4 + 1 + 4, a.n_probe_dev, 0, 2 * rec_bytes, [&] { launch_ordered_join_write_band(o, fuse, stream); });
}

// The blocks (64 entries x 64 rows) and what runs over them.  First the radix sort of a probe side that came neither sorted nor small (in the time, not in the algorithmic bytes:
// SURVEY 8d), the blocks' buffers, the launch of the block kernels sized from the previous execution's count (+ 25 %), not from the upper bound (in place: exactly), where this execution
// leaves its own counts, the rows per key and the blocks of every key laid out; then the pair test, the full-semantics pass where rows may need it, the scan of the blocks' counts, the output rows.
void Plan::band_blocks_and_emit(BandJoin& bj) {
  const LdsJoinArgs& a = bj.j.a; BandArgs& b = bj.j.band;
  const u32 kn = bj.kn; const u64 np = bj.np, max_blocks = bj.max_blocks;
  if (!bj.presorted && !bj.counting) timed(KC_RADIX_SORT, 0, np, nullptr, 0, nullptr, 0, 0, [&] { sort_pairs_u32_u32(b.skey_in, bj.skey, b.sval_in, bj.perm, np, bj.sort_bits, bj.sort_temp, bj.sort_temp_bytes, stream); });
  b.boff = bj.in_place ? bj.lay.boff : scratch<u32>((u64)kn + 1); b.n_blocks_out = new_counter();
  // the multi-row count is the ordered join's (pending_oj.o stays as it was when that join was taken over); a band join that was not fused has none
  band_feedback.push_back({&bj.j.nd, (u32)(b.n_blocks_out - counters), (u32)(reinterpret_cast<u64*>(b.slow_rows) - counters), (u32)(reinterpret_cast<u64*>(b.run_stats) - counters),
                           bj.fused ? (int)(reinterpret_cast<u64*>(pending_oj.o.multi_rows) - counters) : -1, bj.skip_slow, bj.in_place, bj.in_place ? max_blocks : 0});
  const u64 hist = bj.j.nd.band.blocks; b.launch_blocks = (u32)(bj.in_place ? max_blocks : std::min<u64>(max_blocks, hist ? hist + hist / 4 + 1024 : max_blocks));
  b.bdesc = bj.in_place ? bj.lay.bdesc : scratch<uint4>(max_blocks);
  const size_t tb = std::max(scan_temp_bytes(std::max<u64>((u64)kn + 1, max_blocks + 1)), band_blocks_scan_temp_bytes(kn)); void* temp = scratch<unsigned char>(tb);
  if (bj.counting) {   // poff = exclusive scan of the rows per key (entry kn = the rows that join something); then the scatter
    timed(scan_class((u64)kn + 1), 0, (u64)kn + 1, nullptr, 8, nullptr, 0, 0, [&] { exclusive_scan_u32(b.key_hist, b.poff, (u64)kn + 1, temp, tb, stream); });
    RDFGPU_HIP(hipMemcpyAsync(b.key_cursor, b.poff, ((size_t)kn + 1) * sizeof(u32), hipMemcpyDeviceToDevice, stream));
    timed(KC_BAND_ROWS, 0, np, bj.j.P.n_dev, 8 + 32 + 32, nullptr, 0, 0, [&] { launch_band_scatter(b, stream); });
  } else if (!bj.presorted) timed(KC_BAND_BOUNDS, 0, np, nullptr, 4, nullptr, 0, 0, [&] { launch_band_bounds(bj.skey, np, kn, b.poff, stream); });   // (presorted: the decode pass wrote poff)
  if (!bj.in_place) {
    timed(scan_class((u64)kn + 1), 12ull * kn, (u64)kn + 1, nullptr, 4, nullptr, 0, 0, [&] { band_blocks_scan(a.csr_off, b.poff, kn, b.boff, temp, tb, stream); });   // (blocks per key: the scan's input iterator)
    timed(KC_BAND_DESC, 12ull * kn, 0, nullptr, 0, nullptr, 0, 0, [&] { launch_band_desc(b, stream); });
  }
  if (!bj.presorted && !bj.counting) timed(KC_BAND_ROWS, 0, np, bj.j.P.n_dev, 4 + 32 + 32, nullptr, 0, 0, [&] { launch_band_rows(b, stream); });
  const u64* const nrows_dev = bj.in_place ? nullptr : bj.j.P.n_dev;
  const BandPassBytes bytes = band_pass_bytes(bj);
  timed(KC_BAND_MASK, bytes.mask_fixed, bj.nrows, nrows_dev, bytes.mask_row, nullptr, 0, 0, [&] { launch_band_mask(b, bj.form, stream); });
  if (!bj.skip_slow) {
    if (bj.row_static()) fail(RDFGPU_ERR_INVALID, "band join: the full-semantics pass over a step of form %s", band_form_name(bj.form));
    // the full-semantics pass needs the chain's literals and columns: the fused join kernel's argument block, by pointer
    static_assert(sizeof(LdsJoinArgs) <= ExecContext::kArgBytes, "argument staging slot too small");
    const u32 slot = arg_slots_used++;
    LdsJoinArgs* a_host = reinterpret_cast<LdsJoinArgs*>(ctx->args_host + (size_t)slot * ExecContext::kArgBytes);
    LdsJoinArgs* a_dev = reinterpret_cast<LdsJoinArgs*>(ctx->args_dev + (size_t)slot * ExecContext::kArgBytes);
    *a_host = a; RDFGPU_HIP(hipMemcpyAsync(a_dev, a_host, sizeof(LdsJoinArgs), hipMemcpyHostToDevice, stream));
    timed(KC_BAND_SLOW, 0, 0, nullptr, 0, nullptr, 0, 0, [&] { launch_band_slow(a_dev, b, stream); });
  }
  timed(scan_class(max_blocks + 1), 0, max_blocks + 1, nullptr, 8, nullptr, 0, 0, [&] { exclusive_scan_u32(b.bcount, b.bofs, max_blocks + 1, temp, tb, stream); });
  // The count point (host_logic.hpp, early_count_eligible): the scan has made the result's row count final (bofs[max_blocks]: emit's thread 0 merely copies it into
  // n_out_dev and derives the overflow flag), and every counter the host reads after an execution was written by the passes up to here.  Counters and total go to
  // the host's mirror now, the count event behind them: Plan::execute waits for that event, not for emit.
  const NodeInfo* top = &nodes[root];   // (a ProjectionExec selects columns and launches nothing)
  while (top->d.kind == RDFGPU_NODE_PROJECTION) top = &nodes[top->d.left];
  EarlyCountShape early;
  early.is_root = bj.j.out_node == top; early.result_is_output = !bj.j.left_join && !pending_oj.active; early.skip_slow = bj.skip_slow; early.form = bj.form;
  early.speculative = speculative; early.priming = priming; early.timing = timing; early.option_off = !opt.on(RDFGPU_OPT_NO_EARLY_RESULT_COUNT);
  if (early_count_eligible(early)) {
    launch_band_count_point(counters, b.bofs + max_blocks, ctx->counters_host_dev, stream);
    RDFGPU_HIP(hipEventRecord(ctx->count_event, stream));
    count_point.armed = true; count_point.n_out_dev = b.n_out_dev; count_point.n_out = (u32)(b.n_out_dev - counters);
    count_point.overflow = (u32)(reinterpret_cast<u64*>(b.overflow) - counters); count_point.out_cap = b.out_cap;
  }
  timed(KC_BAND_EMIT, bytes.emit_fixed, bj.nrows, nrows_dev, 4 + 4ull * b.n_row_cols, a.n_out_dev, 0, 4ull * a.n_out_cols, [&] { launch_band_emit(b, bj.form, stream); });
}

}  // namespace rdfgpu
