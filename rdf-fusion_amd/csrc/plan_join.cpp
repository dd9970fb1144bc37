// plan_join.cpp — the joins: CrossJoinExec, the generic hash / nested-loop join, semi / anti joins, and the join against one table
// (LDS copy, store slice, partitions) with its ordered-slice form.
//   Plan::exec_join         HashJoinExec(CollectLeft) / CrossJoinExec / NestedLoopJoinExec (DataFusion 52),
//                           semantics from lib/logical/src/join/rewrite.rs:71-221
#include "plan_exec.hpp"

namespace rdfgpu {

namespace {
u32 pow2_at_least(u64 v) { u64 p = 1024; while (p < v && p < (1ull << 31)) p <<= 1; return (u32)p; }
}  // namespace

// The held-back write pass of an ordered slice join runs before anything reads its table, except the band join that consumes
// it: it may stay pending into a join only while the table is that join's probe side — an inner LDS join whose band join took
// the records last time (the sides as exec_join chooses them below).  exec_lds_join then hands it on to the band join or runs
// it just before the probe side is read.
bool Plan::keeps_pending_oj(const NodeInfo& nd, const DevTable& L, const DevTable& R, bool left_join, bool lf, bool rf) const {
  if (!nd.band.takes_records || nd.d.kind != RDFGPU_NODE_HASH_JOIN || left_join || lf || rf || opt.on(RDFGPU_OPT_NO_LDS_JOIN) || nd.lex) return false;
  const bool build_left = choose_build_left(nd, L, R, false, false, false);
  const DevTable& B = build_left ? L : R; const DevTable& P = build_left ? R : L;
  return (B.cap <= kLdsJoinMaxBuild || !opt.on(RDFGPU_OPT_NO_GLOBAL_TABLE_JOIN)) && P.cols[0] == pending_oj.first_col && B.cols[0] != pending_oj.first_col;
}

// The held-back write pass of an ordered slice join, run after all: its consumer turned out not to take the band join's records.
void Plan::flush_pending_oj() {
  if (!pending_oj.active) return;
  count_pending_oj();
  pending_oj.active = false;
  const OrderedJoinArgs& o = pending_oj.o;
  timed(KC_OJ_WRITE, 0, pending_oj.n_build, nullptr, 4, o.n_out_dev, 0, 8ull * o.n_out_cols, [&] { launch_ordered_join_write(o, stream); });
}

// The full probe pass of an ordered slice join: the multimap of the table's rows by key, every row's stage rows and its packed record (and, on the way, the fill of key_rec / key_val).
void Plan::probe_ordered_join(OrderedJoinArgs& o) {
  o.head = scratch<uint2>(o.kn); o.next = scratch<u32>(o.n_probe_cap);
  RDFGPU_HIP(hipMemsetAsync(o.head, 0xFF, (size_t)o.kn * sizeof(uint2), stream));
  for (u32 s = 0; s < o.n_stages; s++) o.stage[s].row = scratch<u32>(o.n_probe_cap);
  o.trec = scratch<uint4>(o.n_probe_cap * o.n_rec);
  timed(KC_OJ_PROBE, 0, o.n_probe_cap, o.n_probe_dev, 8 + 12ull * o.n_stages, nullptr, 0, 0, [&] { launch_ordered_join_probe(o, stream); });
}
// The count pass of an ordered slice join and the scan of its per-tile counts: where every match goes.
void Plan::count_ordered_join(OrderedJoinArgs& o) {
  const u64 tiles = ordered_join_tiles(o.n_build);
  o.tile_count = scratch<u32>(tiles + 1); o.tile_off = scratch<u32>(tiles + 1);
  o.row_head = scratch<u32>(o.n_build); o.row_cnt = scratch<unsigned char>(o.n_build);
  const size_t tb = scan_temp_bytes(tiles + 1);
  void* temp = scratch<unsigned char>(tb);
  timed(KC_OJ_COUNT, 0, o.n_build, nullptr, 4, nullptr, 0, 0, [&] { launch_ordered_join_count(o, stream); });
  timed(scan_class(tiles + 1), 0, tiles + 1, nullptr, 8, nullptr, 0, 0, [&] { exclusive_scan_u32(o.tile_count, o.tile_off, tiles + 1, temp, tb, stream); });
}
// The held-back ordered slice join skipped its count pass for an in-place band join that does not take it after all: it runs now,
// and so does the check of the count its write pass will write.
// An owed probe pass (PendingOj::probe_owed) is the full one now: the band join did not take a form that reads the values by key, or it is not the band join that
// takes the table.  From here the step is what it is when the windows were declined after a mutation: it counts and compacts once.
void Plan::count_pending_oj() {
  if (!pending_oj.active || pending_oj.counted) return;
  pending_oj.counted = true;
  if (pending_oj.probe_owed) {
    pending_oj.probe.row_static = false;
    if (oj_probe_form(pending_oj.probe) != OjProbeForm::FULL_NOW) fail(RDFGPU_ERR_INVALID, "ordered join: an owed probe pass of form %s", oj_probe_form_name(oj_probe_form(pending_oj.probe)));
    pending_oj.probe_owed = false;
    probe_ordered_join(pending_oj.o);
  }
  count_ordered_join(pending_oj.o);
  spec_checks.push_back(pending_oj.check);
}

// HashJoinExec / CrossJoinExec / NestedLoopJoinExec (inner and left; the semi / anti joins are exec_semi_join's).
DevTable Plan::exec_join(NodeInfo& nd) {
  DevTable fused;
  if (try_fused_chain(nd, fused)) return fused;
  const JoinInputs in = join_inputs(nd);
  const DevTable& L = in.L; const DevTable& R = in.R;
  if (nd.d.kind == RDFGPU_NODE_CROSS_JOIN) return exec_cross_join(nd, L, R);
  const bool left_join = nd.d.join_type == RDFGPU_JOIN_LEFT;
  DevTable t;
  t.n_cols = nd.n_proj;
  if (L.cap == 0 || (R.cap == 0 && !left_join)) { t.cap = 0; return t; }
  // (a filter with an op of kOpExtended, expr_ops.hpp, takes the generic join: those cases are compiled into join_probe_lex_kernel /
  // nlj_lex_kernel, not into the LDS / partitioned join forms, whose instantiations stay what they were)
  if (nd.d.kind == RDFGPU_NODE_HASH_JOIN && !opt.on(RDFGPU_OPT_NO_LDS_JOIN) && !nd.lex) {
    const bool build_left = choose_build_left(nd, L, R, left_join, in.lf, in.rf);
    if ((build_left ? L.cap : R.cap) <= kLdsJoinMaxBuild || !opt.on(RDFGPU_OPT_NO_GLOBAL_TABLE_JOIN)) {
      const NodeInfo* pf = in.lf ? &nodes[nd.d.left] : in.rf ? &nodes[nd.d.right] : nullptr;
      if (in.post && build_left != (in.post == &nodes[nd.d.left])) fail(RDFGPU_ERR_DEVICE, "join: build side changed under a residual filter");
      return exec_lds_join(nd, L, R, build_left, pf, in.post);
    }
  }
  return exec_generic_join(nd, L, R);
}

// A fusable run of look-up joins with `nd` on top (plan_chain) is handed to its base join, which runs it inside its resolve phase.
// true: `fused` is this node's output.  false: nothing was fused; a base join that ran normally is memoised.
bool Plan::try_fused_chain(NodeInfo& nd, DevTable& fused) {
  if (pending_chain) return false;
  ChainRequest req;
  if (!plan_chain(nd, req)) return false;
  NodeInfo* base = req.links.front().slice_is_left ? &nodes[req.links.front().node->d.right] : &nodes[req.links.front().node->d.left];
  req.base = base;
  pending_chain = &req;
  fused = exec_node((u32)(base - nodes.data()));
  pending_chain = nullptr;
  return req.consumed;   // consumed: `fused` already has this node's schema
}

// The inputs of join `nd`, executed: which FilterExec child is fused into the probe (lf / rf), which becomes a conjunct of the join
// filter (post), which is materialised after all; a held-back ordered-join write this join does not keep is flushed.
Plan::JoinInputs Plan::join_inputs(NodeInfo& nd) {
  const bool left_join = nd.d.join_type == RDFGPU_JOIN_LEFT;
  // Pipeline fusion: a FilterExec child (identity projection, consumed by this join only) is not
  // materialised when it ends up on the probe side of the LDS join — its predicate runs inside the probe.
  auto fusable = [&](int32_t ci) {
    if (nd.d.kind != RDFGPU_NODE_HASH_JOIN || opt.on(RDFGPU_OPT_NO_FILTER_FUSION) || opt.on(RDFGPU_OPT_NO_LDS_JOIN) || nd.lex) return false;
    const NodeInfo& c = nodes[ci];
    if (c.lex) return false;   // (its FilterExec runs filter_kernel<kFilterVmLex>; the probe filter of the LDS join has no such form)
    if (c.d.kind != RDFGPU_NODE_FILTER || c.prog.n == 0 || c.refs != 1 || c.n_proj != nodes[c.d.left].width) return false;
    for (u32 k = 0; k < c.n_proj; k++) if (c.proj[k] != k) return false;
    return true;
  };
  JoinInputs ji;
  DevTable& L = ji.L; DevTable& R = ji.R; bool& lf = ji.lf; bool& rf = ji.rf; const NodeInfo*& post = ji.post;
  lf = !left_join && fusable(nd.d.left); rf = fusable(nd.d.right);
  // the inputs are sub-plans of their own: a chain request pending for THIS join must not keep the joins below from
  // planning theirs (the batched Q5 has two: the constants' look-ups by X, and window 1 / window 2 / label above the
  // candidate join)
  L = exec_sub_plan((u32)(lf ? nodes[nd.d.left].d.left : nd.d.left));
  R = exec_sub_plan((u32)(rf ? nodes[nd.d.right].d.left : nd.d.right));
  if (pending_oj.active && !keeps_pending_oj(nd, L, R, left_join, lf, rf)) flush_pending_oj();
  if (lf || rf) {   // (post: a build-side FilterExec kept as a conjunct of the join filter)
    // `col <=|!=> literal` over a store slice: if the join builds on that slice (index join through the slice's cached
    // table) the FilterExec is neither materialised nor fused into the probe — it becomes one more conjunct of the
    // join filter, evaluated on the candidate pairs
    auto postable = [&](bool has, int32_t ci, const DevTable& in) {
      return has && nodes[ci].shape == 1 && in.stable_id != 0 && in.n_dev == nullptr && in.cap > 1024 && nd.d.n_keys == 1 && !opt.on(RDFGPU_OPT_NO_INDEX_JOIN);
    };
    const bool lpost = postable(lf, nd.d.left, L), rpost = postable(rf, nd.d.right, R);
    const bool build_left = choose_build_left(nd, L, R, left_join, lf, rf, lpost, rpost);
    const bool lds = ((build_left ? L.cap : R.cap) <= kLdsJoinMaxBuild || !opt.on(RDFGPU_OPT_NO_GLOBAL_TABLE_JOIN)) && L.cap && R.cap;
    if (lds && lf && build_left && lpost) { post = &nodes[nd.d.left]; lf = false; }
    else if (lds && rf && !build_left && rpost) { post = &nodes[nd.d.right]; rf = false; }
    // a fused filter survives only on the probe side of the LDS join; anything else is materialised now
    if (lf && (!lds || build_left)) { L = apply_filter(nodes[nd.d.left], L); lf = false; }
    if (rf && (!lds || !build_left)) { R = apply_filter(nodes[nd.d.right], R); rf = false; }
  }
  return ji;
}

// CrossJoinExec: every pair.
DevTable Plan::exec_cross_join(const NodeInfo& nd, const DevTable& L, const DevTable& R) {
  DevTable t;
  t.n_cols = nd.n_proj;
  const u64 cap = L.cap * R.cap;
  if (cap == 0) { t.cap = 0; return t; }
  if (cap >= (1ull << 40)) fail(RDFGPU_ERR_UNSUPPORTED, "cross join of %llu x %llu rows", (unsigned long long)L.cap, (unsigned long long)R.cap);
  CrossArgs a{};
  for (u32 c = 0; c < L.n_cols; c++) a.left[c] = L.cols[c];
  for (u32 c = 0; c < R.n_cols; c++) a.right[c] = R.cols[c];
  a.n_left_cols = L.n_cols; a.n_right_cols = R.n_cols; a.n_out_cols = nd.n_proj;
  for (u32 c = 0; c < nd.n_proj; c++) { a.proj[c] = nd.proj[c]; a.out[c] = scratch<u32>(cap); t.cols[c] = a.out[c]; }
  a.n_left_dev = L.n_dev; a.n_left_cap = L.cap; a.n_right_dev = R.n_dev; a.n_right_cap = R.cap;
  const bool dyn = L.n_dev || R.n_dev;
  a.n_out_dev = dyn ? new_counter() : nullptr;
  // CrossJoinExec bytes: 4·c·N (both inputs read once) + 4·c_o·m·N (every output cell written)
  timed(KC_CROSS, 4ull * R.n_cols * R.cap, L.cap, L.n_dev, 4ull * L.n_cols, a.n_out_dev, dyn ? 0 : cap, 4ull * nd.n_proj,
        [&] { launch_cross(a, stream); });
  t.cap = cap; t.n_dev = a.n_out_dev;
  return t;
}

// HashJoinExec / NestedLoopJoinExec without the one-table forms: build (hash), count per probe row, scan, write; the unmatched
// left rows of a left join behind them.  One host round trip for the total.  Neither input is empty (a left join's right one may be).
DevTable Plan::exec_generic_join(const NodeInfo& nd, const DevTable& L, const DevTable& R) {
  const bool left_join = nd.d.join_type == RDFGPU_JOIN_LEFT, hash = nd.d.kind == RDFGPU_NODE_HASH_JOIN;
  DevTable t;
  t.n_cols = nd.n_proj;
  JoinArgs a{};
  for (u32 c = 0; c < L.n_cols; c++) a.left[c] = L.cols[c];
  for (u32 c = 0; c < R.n_cols; c++) a.right[c] = R.cols[c];
  a.n_left_cols = L.n_cols; a.n_right_cols = R.n_cols; a.n_out_cols = nd.n_proj;
  for (u32 c = 0; c < nd.n_proj; c++) a.proj[c] = nd.proj[c];
  a.n_keys = hash ? nd.d.n_keys : 0;
  for (u32 k = 0; k < a.n_keys; k++) { a.left_keys[k] = nd.d.left_keys[k]; a.right_keys[k] = nd.d.right_keys[k]; }
  a.n_left_dev = L.n_dev; a.n_left_cap = L.cap; a.n_right_dev = R.n_dev; a.n_right_cap = R.cap;
  a.has_filter = nd.prog.n ? 1 : 0;
  a.prog = nd.prog;
  bind_values(a.prog);
  a.tt = typed_table();
  if (L.cap >= 0xFFFFFFF0ull) fail(RDFGPU_ERR_UNSUPPORTED, "build side of %llu rows", (unsigned long long)L.cap);
  if (left_join) { a.visited = scratch<u8>(L.cap); if (!hash) RDFGPU_HIP(hipMemsetAsync(a.visited, 0, L.cap, stream)); }
  if (hash) {
    const u32 nb = pow2_at_least(2 * L.cap);
    a.heads = scratch<u32>(nb); a.bucket_mask = nb - 1;
    a.next = scratch<u32>(L.cap);
    RDFGPU_HIP(hipMemsetAsync(a.heads, 0xFF, (size_t)nb * 4, stream));
    // build: 4·k·N_b keys read + 8·N_b (one head/next slot written per row)   (build half)
    timed(KC_JOIN_BUILD, 0, L.cap, L.n_dev, 4ull * a.n_keys + 8, nullptr, 0, 0, [&] { launch_join_build(a, stream); });
  }
  // columns of the probe side the write pass has to read: keys ∪ projected right columns ∪ filter columns
  u32 probe_used = columns_read(nd.prog) >> L.n_cols;
  for (u32 k = 0; k < a.n_keys; k++) probe_used |= 1u << a.right_keys[k];
  for (u32 c = 0; c < nd.n_proj; c++) if (nd.proj[c] >= L.n_cols) probe_used |= 1u << (nd.proj[c] - L.n_cols);
  const u32 probe_cols = (u32)__builtin_popcount(probe_used);
  u64 total = 0;
  u32* offs = nullptr;
  if (R.cap) {
    u32* counts = scratch<u32>(R.cap);
    offs = scratch<u32>(R.cap);
    const size_t tb = scan_temp_bytes(R.cap);
    void* temp = scratch<u8>(tb);
    a.counts = counts;
    // count pass: 4·k·N_p keys + 8·N_p (head + first chain slot read per probe row)
    timed(hash ? KC_JOIN_COUNT : KC_NLJ_COUNT, 0, R.cap, R.n_dev, 4ull * a.n_keys + 8, nullptr, 0, 0,
          [&] { if (hash) launch_join_count(a, stream); else launch_nlj_count(a, stream); });
    timed(scan_class(R.cap), 0, R.cap, nullptr, 8, nullptr, 0, 0, [&] { inclusive_scan_u32(counts, offs, R.cap, temp, tb, stream); });
    total = read_back<u32>(offs + R.cap - 1);
  }
  const u64 cap = total + (left_join ? L.cap : 0);
  if (cap == 0) { t.cap = 0; return t; }
  for (u32 c = 0; c < nd.n_proj; c++) { a.out[c] = scratch<u32>(cap); t.cols[c] = a.out[c]; }
  if (total) {
    a.counts = offs;
    // write pass: 4·(k+p_p)·N_p + 8·N_p + 4·c_o·N_o   (probe half)
    timed(hash ? KC_JOIN_WRITE : KC_NLJ_WRITE, 0, R.cap, R.n_dev, 4ull * probe_cols + 8, nullptr, total, 4ull * nd.n_proj,
          [&] { if (hash) launch_join_write(a, stream); else launch_nlj_write(a, stream); });
  }
  t.cap = cap;
  if (left_join) {
    u64* n_out = new_counter();
    RDFGPU_HIP(hipMemcpyAsync(n_out, &total, sizeof(u64), hipMemcpyHostToDevice, stream));
    RDFGPU_HIP(hipStreamSynchronize(stream)); metrics.host_syncs++;   // `total` is a stack variable
    left_join_tail(nd, L, R, a.out, a.visited, n_out, 0);
    t.n_dev = n_out;
  }
  return t;
}

// HashJoinExec / NestedLoopJoinExec with JoinType::LeftSemi / LeftAnti (semi_join.hip).  The output has at most as many rows as the
// left input: a table of cap L.cap whose count stays on the device, like a FilterExec's — no speculation, no overflow, no re-run.
// The right input (the existence side) is the table, the left rows probe it: a set built by every workgroup in LDS when the right
// input is small, else one set in HBM built in this execution; a NestedLoopJoinExec streams the right rows through LDS.
DevTable Plan::exec_semi_join(NodeInfo& nd) {
  const bool anti = nd.d.join_type == RDFGPU_JOIN_LEFT_ANTI;
  // the inputs are sub-plans of their own (a chain pending above must not leak into them)
  const DevTable L = exec_sub_plan((u32)nd.d.left);
  const DevTable R = exec_sub_plan((u32)nd.d.right);
  flush_pending_oj();   // a held-back ordered-join write must have happened before either input is read
  DevTable t;
  t.n_cols = nd.n_proj;
  if (L.cap == 0) { t.cap = 0; return t; }
  const bool hash = nd.d.kind == RDFGPU_NODE_HASH_JOIN;
  const bool right_empty = R.cap == 0;
  // the verdict is the same for every left row when the right input is empty (nothing matches), or for a nested-loop join without a
  // filter over a right input whose row count the host knows: the left rows, projected, without a launch
  if (right_empty || (!hash && nd.prog.n == 0 && R.n_dev == nullptr)) {
    const bool keep_all = right_empty ? anti : !anti;
    if (!keep_all) { t.cap = 0; return t; }
    return project(L, nd);
  }
  if (L.cap >= 0xFFFFFFF0ull || R.cap >= 0x7FFFFFFFull) fail(RDFGPU_ERR_UNSUPPORTED, "semi / anti join of %llu x %llu rows", (unsigned long long)L.cap, (unsigned long long)R.cap);
  SemiJoinArgs a{};
  for (u32 c = 0; c < L.n_cols; c++) a.cols[c] = L.cols[c];
  for (u32 c = 0; c < R.n_cols; c++) a.cols[L.n_cols + c] = R.cols[c];
  a.n_left_cols = L.n_cols; a.n_right_cols = R.n_cols;
  a.n_out_cols = nd.n_proj;
  for (u32 c = 0; c < nd.n_proj; c++) { a.proj[c] = nd.proj[c]; a.out[c] = scratch<u32>(L.cap); t.cols[c] = a.out[c]; }
  a.n_keys = hash ? nd.d.n_keys : 0;
  for (u32 k = 0; k < a.n_keys; k++) { a.left_key[k] = L.cols[nd.d.left_keys[k]]; a.right_key[k] = R.cols[nd.d.right_keys[k]]; }
  a.n_left_dev = L.n_dev; a.n_left_cap = L.cap; a.n_right_dev = R.n_dev; a.n_right_cap = R.cap;
  a.tt = typed_table();
  a.n_out_dev = new_counter();
  int filter = kSemiNoFilter;
  u32 left_fcols = 0;   // distinct left columns the filter reads (compulsory bytes)
  if (nd.prog.n) {
    left_fcols = (u32)__builtin_popcount(columns_read(nd.prog) & ((1u << L.n_cols) - 1u));
    if (nd.shape == 2) {   // `col <ID_EQ | ID_NEQ> col`
      filter = kSemiIdPair;
      a.idp = IdPairFilter{nd.prog.nodes[0].u, nd.prog.nodes[1].u, nd.prog.nodes[2].op == RDFGPU_EX_ID_EQ ? 1u : 0u};
    } else {
      filter = nd.lex ? kSemiVmLex : kSemiVm;
      a.prog = upload_program(nd.prog);
    }
  }
  int form = kSemiNested;
  u64 build_bytes = 0;
  if (hash) {
    const u64 lds_max = std::min<u64>(opt.v[RDFGPU_OPT_LDS_MAX_BUILD], kSemiLdsMaxBuild);
    form = R.cap <= lds_max && !opt.on(RDFGPU_OPT_NO_SEMI_LDS) ? kSemiLds : kSemiHbm;
    u64 slots = 64;
    while (slots < 2 * R.cap) slots <<= 1;
    a.tbl_mask = (u32)(slots - 1);
    // build half: the right keys read once, one 8-byte slot written per row
    build_bytes = (4ull * a.n_keys + 8) * R.cap;
    if (form == kSemiHbm) {
      a.gslots = scratch<unsigned long long>(slots);
      RDFGPU_HIP(hipMemsetAsync(a.gslots, 0, slots * sizeof(unsigned long long), stream));
      timed(KC_SEMI_BUILD, 0, R.cap, R.n_dev, 4ull * a.n_keys + 8, nullptr, 0, 0, [&] { launch_semi_build(a, filter == kSemiNoFilter, stream); });
      build_bytes = 0;
    }
  } else {
    build_bytes = 4ull * R.n_cols * R.cap;   // the right rows staged once (re-reads of them come from L2)
  }
  // compulsory bytes: 4·(k + c)·N_left (keys and left filter columns) + 4·c_out·N_out (the survivors' columns, read and written:
  // 8 per cell) + the build's; right columns of candidates are not counted (their number depends on the data)
  timed(semi_join_class(form, anti), build_bytes, L.cap, L.n_dev, 4ull * (a.n_keys + left_fcols), a.n_out_dev, 0, 8ull * nd.n_proj,
        [&] { launch_semi_join(a, form, anti, filter, stream); });
  t.cap = L.cap; t.n_dev = a.n_out_dev;
  return t;
}

// HashJoinExec / NestedLoopJoinExec with JoinType::LeftMark (semi_join.hip: mark_join_kernel, mark_nested_kernel).  The output is the left
// input row for row — same capacity, same count, also when that count is known on the device only — with the mark as one further column:
// a value column of this node whose array is the plan's two records {false, true}.  Tables and their choice are the semi join's.
DevTable Plan::exec_mark_join(NodeInfo& nd) {
  const DevTable L = exec_sub_plan((u32)nd.d.left);
  const DevTable R = exec_sub_plan((u32)nd.d.right);
  flush_pending_oj();
  if (!mark_values_dev) {   // once per plan
    rdfgpu_agg_value two[2] = {};
    two[0].tag = two[1].tag = RDFGPU_TV_BOOLEAN; two[1].lo = 1;
    RDFGPU_HIP(hipMalloc((void**)&mark_values_dev, sizeof two));
    RDFGPU_HIP(hipMemcpyAsync(mark_values_dev, two, sizeof two, hipMemcpyHostToDevice, stream));
    RDFGPU_HIP(hipStreamSynchronize(stream)); metrics.host_syncs++;   // `two` is a stack variable
  }
  nd.values[0] = mark_values_dev; nd.n_values = 2; nd.n_values_dev = nullptr; nd.values_run = run;
  DevTable t;
  t.n_cols = nd.n_proj; t.cap = L.cap; t.n_dev = L.n_dev;
  if (L.cap == 0) return t;
  const u32 mark_col = L.n_cols;
  const bool hash = nd.d.kind == RDFGPU_NODE_HASH_JOIN;
  // the mark is the same for every left row when the right input is empty (false), or for a nested-loop join without a filter over a
  // right input whose row count the host knows (true): the left columns as they are, the mark filled in, no join kernel
  const bool right_empty = R.cap == 0;
  if (right_empty || (!hash && nd.prog.n == 0 && R.n_dev == nullptr)) {
    for (u32 c = 0; c < nd.n_proj; c++) {
      if (nd.proj[c] != mark_col) { t.cols[c] = L.cols[nd.proj[c]]; continue; }
      u32* m = scratch<u32>(L.cap);
      launch_fill_u32(m, right_empty ? 1u : 2u, L.cap, stream);
      t.cols[c] = m;
    }
    return t;
  }
  if (L.cap >= 0xFFFFFFF0ull || R.cap >= 0x7FFFFFFFull) fail(RDFGPU_ERR_UNSUPPORTED, "semi / anti join of %llu x %llu rows", (unsigned long long)L.cap, (unsigned long long)R.cap);
  SemiJoinArgs a{};
  for (u32 c = 0; c < L.n_cols; c++) a.cols[c] = L.cols[c];
  for (u32 c = 0; c < R.n_cols; c++) a.cols[L.n_cols + c] = R.cols[c];
  a.n_left_cols = L.n_cols; a.n_right_cols = R.n_cols;
  a.n_out_cols = nd.n_proj;
  for (u32 c = 0; c < nd.n_proj; c++) { a.proj[c] = nd.proj[c]; a.out[c] = scratch<u32>(L.cap); t.cols[c] = a.out[c]; }
  a.n_keys = hash ? nd.d.n_keys : 0;
  for (u32 k = 0; k < a.n_keys; k++) { a.left_key[k] = L.cols[nd.d.left_keys[k]]; a.right_key[k] = R.cols[nd.d.right_keys[k]]; }
  a.n_left_dev = L.n_dev; a.n_left_cap = L.cap; a.n_right_dev = R.n_dev; a.n_right_cap = R.cap;
  a.tt = typed_table();
  int filter = kSemiNoFilter;
  u32 left_fcols = 0;   // distinct left columns the filter reads (compulsory bytes)
  if (nd.prog.n) {
    left_fcols = (u32)__builtin_popcount(columns_read(nd.prog) & ((1u << L.n_cols) - 1u));
    if (nd.shape == 2) {   // `col <ID_EQ | ID_NEQ> col`
      filter = kSemiIdPair;
      a.idp = IdPairFilter{nd.prog.nodes[0].u, nd.prog.nodes[1].u, nd.prog.nodes[2].op == RDFGPU_EX_ID_EQ ? 1u : 0u};
    } else {
      filter = nd.lex ? kSemiVmLex : kSemiVm;
      a.prog = upload_program(nd.prog);
    }
  }
  int form = kSemiNested;
  u64 build_bytes = 0;
  if (hash) {   // (the rule of exec_semi_join)
    const u64 lds_max = std::min<u64>(opt.v[RDFGPU_OPT_LDS_MAX_BUILD], kSemiLdsMaxBuild);
    form = R.cap <= lds_max && !opt.on(RDFGPU_OPT_NO_SEMI_LDS) ? kSemiLds : kSemiHbm;
    u64 slots = 64;
    while (slots < 2 * R.cap) slots <<= 1;
    a.tbl_mask = (u32)(slots - 1);
    build_bytes = (4ull * a.n_keys + 8) * R.cap;
    if (form == kSemiHbm) {
      a.gslots = scratch<unsigned long long>(slots);
      RDFGPU_HIP(hipMemsetAsync(a.gslots, 0, slots * sizeof(unsigned long long), stream));
      timed(KC_SEMI_BUILD, 0, R.cap, R.n_dev, 4ull * a.n_keys + 8, nullptr, 0, 0, [&] { launch_semi_build(a, filter == kSemiNoFilter, stream); });
      build_bytes = 0;
    }
  } else {
    build_bytes = 4ull * R.n_cols * R.cap;
  }
  // compulsory bytes: per left row its keys and filter columns, its projected columns read and every output column written; the build's
  u32 left_out = 0;
  for (u32 c = 0; c < nd.n_proj; c++) left_out += nd.proj[c] != mark_col;
  timed(mark_join_class(form), build_bytes, L.cap, L.n_dev, 4ull * (a.n_keys + left_fcols + left_out + nd.n_proj), nullptr, 0, 0,
        [&] { launch_mark_join(a, form, filter, stream); });
  return t;
}

// Which input the hash join builds on.  A left join must build on the preserved (left) side.  An inner join builds
// on the smaller input — unless exactly one input is a pure slice of the store (the same rows on every execution
// until the store changes) and the other one is no larger: the slice's join table (direct-address / CSR / hash) is
// built once and cached on the node, so building there costs nothing per execution and the probe is the SMALL side
// (an index nested-loop join against the store's own permutation: `PARAMS JOIN (?s p ?o)` touches |PARAMS| rows,
// not the 5 M-row predicate partition).
bool Plan::choose_build_left(const NodeInfo& nd, const DevTable& L, const DevTable& R, bool left_join, bool lf, bool rf, bool lpost, bool rpost) const {
  if (left_join) {
    // OPTIONAL: HashJoinExec(Left) builds on its left input and probes with the right one — every row of the right input is read, however few
    // left rows there are.  When the right input is a store slice (its join table is cached per store version) and much larger than the left, the
    // join is run the other way round and PRESERVES ITS PROBE SIDE: build = the slice's table, probe = the left rows, a probe row without a match is
    // emitted once with a null right side (LdsJoinArgs::probe_outer).  Same multiset of rows.  Needs: no join filter, no fused filter.
    const bool rs = R.stable_id != 0 && R.n_dev == nullptr && !rf && !lf;
    if (rs && nd.d.kind == RDFGPU_NODE_HASH_JOIN && nd.shape == 0 && !opt.on(RDFGPU_OPT_NO_TABLE_CACHE) && !opt.on(RDFGPU_OPT_NO_INDEX_JOIN) &&
        !opt.on(RDFGPU_OPT_NO_PROBE_OUTER_JOIN) && R.cap > 1024 && L.cap * 4 <= R.cap && L.cap < (1ull << 31))
      return false;
    return true;
  }
  const bool smaller_left = L.cap <= R.cap;
  if (nd.d.kind != RDFGPU_NODE_HASH_JOIN || opt.on(RDFGPU_OPT_NO_TABLE_CACHE) || opt.on(RDFGPU_OPT_NO_INDEX_JOIN)) return smaller_left;
  // (a slice under a `col <=|!=> literal` FilterExec still counts: that filter can run as a conjunct of the join filter)
  const bool ls = L.stable_id != 0 && L.n_dev == nullptr && (!lf || lpost), rs = R.stable_id != 0 && R.n_dev == nullptr && (!rf || rpost);
  if (!ls && !rs) return smaller_left;
  // candidate: build on the slice (the larger one when both inputs are slices), probe with the other input
  const bool slice_left = ls && rs ? !smaller_left : ls;
  const DevTable& S = slice_left ? L : R; const DevTable& O = slice_left ? R : L;
  if (O.cap > S.cap) return smaller_left;                   // the slice is already the smaller side
  if (ls && rs && O.cap * 8 > S.cap) return smaller_left;   // two slices of similar size: nothing to gain
  if (S.cap <= 1024) return smaller_left;                   // LDS-table territory
  // A slice whose keys are not one dense id range (several key columns, or an earlier attempt on this very slice said
  // so) gets a cached HASH table: built once per store version, probed with the fewer rows.  It loses only to a small
  // table built on the other side that stays in L2 while the slice's would not (measured on LUBM Q9's two-key join,
  // 24.6 M rows against a 57 M-row slice: 5.9 ms building on the smaller side every run, 1.3 ms on the cached slice).
  bool hash_only = nd.d.n_keys != 1;
  if (!hash_only) {
    SliceKey sk; sk.n_keys = 1; sk.rows = S.cap; sk.key[0] = S.cols[slice_left ? nd.d.left_keys[0] : nd.d.right_keys[0]];
    const SliceTable* st = store->find_slice_table(sk);
    hash_only = st && st->dense_failed;
  }
  if (hash_only) {
    // The slice is sorted by one of the join keys and the other input is large: building on THAT input inside the step — partition passes
    // over its rows, the slice read in place as id-range partitions (part_join.hip) — beats probing the slice's cached hash table, whose
    // probes are random 64-byte reads of a table far larger than the caches.  Measured on LUBM-8000 Q9's closing two-key join (98 M rows
    // against the 229 M-row takesCourse slice): 3.0 ms with the build in the step, 4.2 - 5.0 ms on the cached table.  The partitioned join
    // walks the whole slice, so it pays only when the other input is a good fraction of it (break-even near a fifth, from those numbers).
    bool sorted_by_key = false;
    for (u32 k = 0; k < nd.d.n_keys; k++) sorted_by_key = sorted_by_key || (S.sorted_col >= 0 && (u32)S.sorted_col == (slice_left ? nd.d.left_keys[k] : nd.d.right_keys[k]));
    if (sorted_by_key && !(ls && rs) && !lf && !rf && nd.d.n_keys <= 2 && S.key_min >= 1 && S.key_max >= S.key_min &&
        !opt.on(RDFGPU_OPT_NO_PARTITIONED_JOIN) && !opt.on(RDFGPU_OPT_NO_RANGE_PARTITION) && !opt.on(RDFGPU_OPT_NO_OWN_PARTITION_PASS) &&
        O.cap >= opt.v[RDFGPU_OPT_PARTITION_MIN_BUILD] && O.cap * 5 >= S.cap && O.cap < (1ull << 31) && S.cap < (1ull << 31))
      return !slice_left;
    if (S.cap > (256ull << 20)) return smaller_left;                             // 32 B per row: keep the footprint sane
    if (O.cap * 8 > S.cap && O.cap <= (1ull << 20)) return smaller_left;
  }
  return slice_left;
}

// The two kernels both direct-address forms start with: min / max of the single key column (one read-back) and, when the id
// range is at most `max_range` ids, one store per row into a table of one slot per id with a duplicate flag (a second
// read-back).  The table is kept with the store's tables (`cached`) or is scratch of this execution; `direct` is set only when
// the keys turned out unique.
Plan::DirectTable Plan::build_direct(const u32* key, u64 n, u64 max_range, bool cached) {
  DirectTable d;
  u32* mm = reinterpret_cast<u32*>(new_counter());   // {min, max}
  d.flags = reinterpret_cast<u32*>(new_counter());   // {duplicate seen, unsorted seen (build_dense_table)}
  const u32 init[2] = {0xFFFFFFFFu, 0u};
  RDFGPU_HIP(hipMemcpyAsync(mm, init, sizeof(init), hipMemcpyHostToDevice, stream));
  timed(KC_MINMAX, 4ull * n, 0, nullptr, 0, nullptr, 0, 0, [&] { launch_minmax_u32(key, n, mm, stream); });
  u32 got[2];
  read_back(got, mm, sizeof got);
  const u64 range = got[0] <= got[1] ? (u64)(got[1] - got[0]) + 1 : ~0ull;
  if (range > max_range) return d;
  d.dense = true; d.kmin = got[0]; d.kn = got[1] - got[0] + 1;
  // more rows than ids in the range: some key repeats (pigeonhole: null keys only make it more so when they are few; with many nulls the
  // attempt below would have succeeded — then the CSR form is merely the more general table for the same join) — no direct-address attempt
  if (n > (u64)d.kn) return d;
  u32* direct = cached ? store->table_alloc<u32>(d.kn) : scratch<u32>(d.kn);
  RDFGPU_HIP(hipMemsetAsync(direct, 0xFF, (size_t)d.kn * sizeof(u32), stream));
  timed(KC_GDIRECT_BUILD, 0, n, nullptr, 8, nullptr, 0, 0, [&] { launch_gdirect_build(key, n, direct, d.kmin, d.kn, d.flags, stream); });
  if (!read_back<u32>(d.flags)) d.direct = direct;
  else if (cached) store->table_free(direct);
  return d;
}

// The dense join tables of a single-key store slice (decided once per slice and store version, with `slice_build_mu` held):
// direct-address if the keys are unique, CSR (offsets + row ids grouped by key; the identity when the slice is sorted by the
// key) if not; `dense_failed` when the id range is not worth a 4-byte-per-id table.  Costs a few small kernels and host
// syncs at that time, nothing afterwards.
void Plan::build_dense_table(SliceTable* st, const u32* key, u64 n) {
  // "dense" = the id range is worth a 4-B-per-id table: up to 4 ids per row outright; up to 64 ids per row while
  // the table stays small (16 M ids = 64 MB) — a subject-hash shard of a slice keeps the slice's id range with
  // 1/G of its rows, and must not fall off the index-join path for that
  const DirectTable d = build_direct(key, n, std::max<u64>(4 * n + 1024, std::min<u64>(64 * n + 1024, 16ull << 20)), true);
  if (!d.dense) { st->dense_failed = true; st->dense_tried = true; return; }
  metrics.tables_built++;
  const u32 kmin = d.kmin, kn = d.kn;
  st->kmin = kmin; st->kn = kn;
  if (d.direct) { st->direct = d.direct; st->dense_tried = true; return; }
  // duplicates: CSR (offsets + row ids grouped by key) — by boundary searches when the slice is sorted by the key, by one radix sort otherwise
  u32* off = store->table_alloc<u32>((u64)kn + 2); u32* rows = nullptr;
  if (n >= (1ull << 32)) fail(RDFGPU_ERR_UNSUPPORTED, "CSR table of %llu rows", (unsigned long long)n);
  u32* rel = scratch<u32>(n);
  timed(KC_CSR_HIST, 0, n, nullptr, 8, nullptr, 0, 0, [&] { launch_csr_rel_keys(key, n, kmin, kn, rel, d.flags + 1, stream); });
  const u32* grouped = rel;
  if (read_back<u32>(d.flags + 1)) {   // unsorted; else the slice is sorted by the key: rows[] is the identity and is never materialised
    rows = store->table_alloc<u32>(n);
    u32 bits = 1;
    while ((1ull << bits) <= kn) bits++;             // keys 0 .. kn (kn = joins nothing: sorts to the end)
    u32* rel_s = scratch<u32>(n); u32* iota = scratch<u32>(n);
    const size_t stb = sort_u32_temp_bytes(n, bits);
    void* stemp = scratch<unsigned char>(stb);
    launch_iota_u32(iota, n, stream);
    timed(KC_CSR_SCATTER, 0, n, nullptr, 12, nullptr, 0, 0, [&] { sort_pairs_u32_u32(rel, rel_s, iota, rows, n, bits, stemp, stb, stream); });
    grouped = rel_s;
  }
  launch_sorted_bounds(grouped, n, kn, off, stream);   // off[k] = first position with rel >= k, k = 0 .. kn (off[kn] = the rows that join something)
  RDFGPU_HIP(hipStreamSynchronize(stream)); metrics.host_syncs++;   // complete before other plans may see it
  st->csr_rows = rows; st->csr_off = off;
  st->dense_tried = true;
}

// HashJoinExec whose build side is one table — a copy per workgroup in LDS, a store slice's cached table, a table built in this
// execution, or one per partition: one fused kernel, optimistic output capacity.
DevTable Plan::exec_lds_join(NodeInfo& nd, const DevTable& L, const DevTable& R, bool build_left, const NodeInfo* probe_filter, const NodeInfo* post_filter) {
  LdsJoin j(nd, L, R, build_left, probe_filter, post_filter);
  LdsJoinArgs& a = j.a;
  if (j.B.cap >= (1ull << 30)) fail(RDFGPU_ERR_UNSUPPORTED, "build side of %llu rows", (unsigned long long)j.B.cap);
  lds_join_args(j);
  j.table = choose_join_table(j);
  if (j.P.cap >= (1ull << 32)) fail(RDFGPU_ERR_UNSUPPORTED, "probe side of %llu rows", (unsigned long long)j.P.cap);
  size_wave_queue(j);
  if (j.left_join) a.visited = scratch<u8>(L.cap);
  a.n_out_dev = new_counter();
  a.overflow = reinterpret_cast<u32*>(new_counter());
  j.tail = j.left_join ? L.cap : 0;
  if (j.table == JoinTable::ScratchHash)   // build pass: keys read + one 8-byte slot written per build row
    timed(KC_GJOIN_BUILD, 0, j.B.cap, j.B.n_dev, 4ull * a.n_keys + 8, nullptr, 0, 0, [&] { launch_gjoin_build(a, stream); });
  // Speculative mode (re-execution of a plan whose previous run is known): the output is sized from the
  // previous cardinality of this operator and NOTHING is waited for — the exact count stays on the device,
  // the overflow flag is checked once at the end of the plan (Plan::execute), which re-runs exactly if any
  // speculation failed.
  // First execution of a plan (DataFusion compiles a fresh plan per query): no history, but the table form bounds or
  // estimates the output — a direct-address table yields at most one match per probe row (exact bound), a CSR table
  // about its mean rows per key, a hash table is assumed unique-ish — so the join can run without a host round
  // trip as well; the overflow flag at the end of the plan catches a wrong guess (exact re-run).
  u64 first_guess = 0;
  if (speculative && !nd.has_last && !j.left_join && !opt.on(RDFGPU_OPT_NO_FIRST_RUN_SPECULATION)) {
    if (a.direct) first_guess = j.P.cap;
    else if (a.csr_off) first_guess = 2 * j.P.cap * ((j.B.cap + a.direct_n - 1) / (a.direct_n ? a.direct_n : 1)) + 1024;
    else first_guess = j.P.cap + 1024;
  }
  const bool spec = speculative && (nd.has_last || first_guess);
  // a fusable run of follow-up lookups above this join (Plan::plan_chain) executes inside this join's resolve
  // phase: the output is then the TOP node's, sized from the top node's history
  NodeInfo* size_node = &nd;
  if (spec && pending_chain && pending_chain->base == &nd && !pending_chain->consumed && j.global_table && j.table != JoinTable::Partitioned && !j.left_join &&
      !j.probe_outer && !probe_filter && nd.shape != 1 && apply_chain(*pending_chain, j)) {
    pending_chain->consumed = true;
    size_node = pending_chain->top;
    j.t.n_cols = a.n_out_cols;
  }
  // the probe side is read from here on: only the band join takes an ordered slice join's held-back write pass (exec_band_join)
  if (!j.use_band) flush_pending_oj();
  if (j.table == JoinTable::Partitioned) {
    // output of the previous execution (none: single pass): above ~50 M rows the reservations of a single pass (one
    // same-address atomic per 256 rows, ~88 per microsecond) cost more than walking every partition twice
    const u64 expect_out = nd.has_last ? nd.last_rows : 0;
    j.part.two_pass = expect_out >= opt.v[RDFGPU_OPT_PARTITION_TWO_PASS_ROWS] ? 1u : 0u;
    if (j.part.two_pass && nd.shape == 2 && !j.left_join) {   // `build column <=|!=> probe column`: decided during the walk (part_join.hip, INL)
      const u32 ca = nd.prog.nodes[0].u, cb = nd.prog.nodes[1].u;
      if (on_build_side(a, ca) != on_build_side(a, cb)) { j.part.inl_build = a.cols[on_build_side(a, ca) ? ca : cb]; j.part.inl_probe = a.cols[on_build_side(a, ca) ? cb : ca]; }
    }
    prepare_partitions(a, j.B, j.P, j.part);   // the build half of this HashJoinExec: inside the operator, every execution
  }
  return spec ? run_speculative(j, first_guess, *size_node) : run_exact(j);
}

// The kernel arguments that do not depend on the build side's table: both inputs' columns, the keys, the join filter, the fused
// probe-side filter, the build-side filter kept as a conjunct, and the columns each side reads (bytes).
void Plan::lds_join_args(LdsJoin& j) {
  const NodeInfo& nd = j.nd; const DevTable& L = j.L; const DevTable& R = j.R;
  LdsJoinArgs& a = j.a;
  j.t.n_cols = nd.n_proj;
  for (u32 c = 0; c < L.n_cols; c++) a.cols[c] = L.cols[c];
  for (u32 c = 0; c < R.n_cols; c++) a.cols[L.n_cols + c] = R.cols[c];
  a.n_left_cols = L.n_cols; a.n_out_cols = nd.n_proj;
  for (u32 c = 0; c < nd.n_proj; c++) a.proj[c] = nd.proj[c];
  a.build_is_left = j.build_left ? 1 : 0;
  a.probe_outer = j.probe_outer ? 1u : 0u;
  a.n_keys = nd.d.n_keys;
  for (u32 k = 0; k < a.n_keys; k++) {
    j.build_keys[k] = j.build_left ? nd.d.left_keys[k] : nd.d.right_keys[k];
    j.probe_keys[k] = j.build_left ? nd.d.right_keys[k] : nd.d.left_keys[k];
    a.build_key[k] = j.B.cols[j.build_keys[k]];
    a.probe_key[k] = j.P.cols[j.probe_keys[k]];
  }
  a.n_build_dev = j.B.n_dev; a.n_build_cap = j.B.cap; a.n_probe_dev = j.P.n_dev; a.n_probe_cap = j.P.cap;
  a.probe_col_base = j.build_left ? L.n_cols : 0;
  a.has_filter = (u32)nd.shape;   // 0 none / 1 generic VM / 2 id (in)equality / 3 window
  if (nd.shape == 1) a.prog = upload_program(nd.prog);
  if (nd.shape == 2) { a.idp.a = nd.prog.nodes[0].u; a.idp.b = nd.prog.nodes[1].u; a.idp.is_eq = nd.prog.nodes[2].op == RDFGPU_EX_ID_EQ; }
  if (nd.shape == 3) {
    const rdfgpu_expr_node* e = nd.prog.nodes;
    a.win.x0 = e[0].u; a.win.y0 = e[2].u; a.win.x1 = e[8].u; a.win.y1 = e[10].u;
    a.win.l0 = window_literal(e, 0); a.win.l1 = window_literal(e, 8);
  }
  const NodeInfo* pf = j.probe_filter;
  a.has_probe_filter = pf ? (pf->shape == 1 ? 1u : 2u) : 0u;
  if (pf) {
    if (pf->shape == 1) {
      const rdfgpu_expr_node* e = pf->prog.nodes;
      a.pid.col = a.probe_col_base + e[0].u; a.pid.lit = e[1].u; a.pid.is_eq = e[2].op == RDFGPU_EX_ID_EQ;
    } else a.probe_prog = upload_program(pf->prog);
  }
  if (j.post_filter) {   // FilterExec of the build side's input, columns relative to that input
    const rdfgpu_expr_node* e = j.post_filter->prog.nodes;
    a.has_post = 1;
    a.post.col = (j.build_left ? 0 : L.n_cols) + e[0].u; a.post.lit = e[1].u; a.post.is_eq = e[2].op == RDFGPU_EX_ID_EQ;
  }
  a.tt = typed_table();
  a.stream_direct = opt.on(RDFGPU_OPT_NO_STREAM_JOIN) ? 0u : 1u;
  // columns the kernel reads on the probe side: keys ∪ projected ∪ filter columns
  bool pu[kMaxCols] = {}, bu[kMaxCols] = {};
  auto mark = [&](u32 c) { (on_build_side(a, c) ? bu : pu)[c < L.n_cols ? c : c - L.n_cols] = true; };
  for (u32 k = 0; k < a.n_keys; k++) pu[j.probe_keys[k]] = true;
  for (u32 c = 0; c < nd.n_proj; c++) mark(nd.proj[c]);
  for (u32 i = 0; i < nd.prog.n; i++) if (nd.prog.nodes[i].op == RDFGPU_EX_COLUMN) mark(nd.prog.nodes[i].u);
  if (pf) for (u32 i = 0; i < pf->prog.n; i++) if (pf->prog.nodes[i].op == RDFGPU_EX_COLUMN) pu[pf->prog.nodes[i].u] = true;
  for (u32 k = 0; k < a.n_keys; k++) bu[j.build_keys[k]] = false;
  for (bool b : pu) j.probe_cols += b;
  for (bool b : bu) j.build_payload += b;
  j.build_bytes = (4ull * (a.n_keys + j.build_payload) + 8) * j.B.cap;
}

// Which table the join probes, built now where it has to be: the kernels this triggers run here, before the probe.
JoinTable Plan::choose_join_table(LdsJoin& j) {
  const NodeInfo& nd = j.nd;
  const DevTable& B = j.B; const DevTable& P = j.P;
  LdsJoinArgs& a = j.a;
  u32& slots = j.slots;
  while (slots < 2 * B.cap) slots <<= 1;
  // LDS copy per workgroup vs ONE table in HBM/L2: the LDS form pays the build once per workgroup and, above
  // ~16 KiB of table, costs occupancy (a 128 KiB table = one workgroup per CU = latency-bound probes).
  const u64 lds_limit = std::min<u64>(opt.v[RDFGPU_OPT_LDS_MAX_BUILD], kLdsJoinMaxBuild);
  j.global_table = B.cap > lds_limit;
  // Every lane of a wave waits for the longest chain among its 64 probes, so short chains matter more than a
  // small table: LDS tables get load <= 0.25 and at least 2048 slots (16 KiB), HBM tables under 1 MiB load <= 0.125.
  if (!j.global_table) { while ((slots < 4 * B.cap || slots < 2048) && slots < 2 * kLdsJoinMaxBuild) slots <<= 1; }
  else { while (slots < 8 * B.cap && (u64)slots * sizeof(uint2) < (1u << 20)) slots <<= 1; }
  a.tbl_mask = slots - 1;
  if (!j.global_table) return JoinTable::Lds;
  // The HBM table of a build side that is a pure slice of the store (a param-free scan: label, simProperty…) is the
  // same for every plan until the store changes: it is built once per store version and kept on the store.
  if (B.stable_id != 0 && B.n_dev == nullptr && !opt.on(RDFGPU_OPT_NO_TABLE_CACHE)) {
    SliceKey sk; sk.n_keys = a.n_keys; sk.rows = B.cap;
    for (u32 k = 0; k < a.n_keys; k++) sk.key[k] = a.build_key[k];
    SliceTable* st = store->slice_table(sk);
    j.slice = st;
    std::unique_lock<std::mutex> building(store->slice_build_mu);
    // Dense forms first (one single key over a dense id range): direct-address if the keys are unique, CSR if not.
    // Decided once per slice; costs a few small kernels and host syncs at that time, nothing afterwards.
    if (!st->dense_tried && a.n_keys == 1 && !opt.on(RDFGPU_OPT_NO_DIRECT_TABLE)) build_dense_table(st, a.build_key[0], B.cap);
    if (st->csr_off) {
      a.csr_off = st->csr_off; a.csr_rows = st->csr_rows; a.direct_min = st->kmin; a.direct_n = st->kn;
      // lanes per probe row: a small probe side with a large fan-out is spread over the chip
      // (first execution: the table's mean rows per key stands in for the unknown fan-out)
      const u64 fan = nd.has_last ? nd.last_rows / (P.cap ? P.cap : 1) : B.cap / (st->kn ? st->kn : 1);
      // measured on the BSBM candidate join (fan-out 111): 8 lanes per row is best at 75 k and at 1.2 M probe rows alike
      // (a tiny probe side — a single query's constants — is latency-bound instead: spread each row over up to a whole wave)
      const bool tiny = P.cap < 4096;
      u32 rl = 0;
      while (rl < (tiny ? 6u : 3u) && ((tiny ? 2ull : 16ull) << rl) <= fan && (P.cap << (rl + 1)) <= (1ull << 25)) rl++;
      if (opt.v[RDFGPU_OPT_CSR_ROW_LANES_LOG2]) rl = (u32)std::min<u64>(6, opt.v[RDFGPU_OPT_CSR_ROW_LANES_LOG2] - 1);
      if (j.probe_outer) rl = 0;   // (one lane per probe row: the row's null-extended candidate is produced once)
      a.row_lanes_log2 = rl;
      return JoinTable::SliceCsr;
    }
    if (st->direct) { a.direct = st->direct; a.direct_min = st->kmin; a.direct_n = st->kn; return JoinTable::SliceDirect; }
    if (!st->slots || st->mask != a.tbl_mask) {   // build the hash form now, under the lock, and publish it only when complete
      if (st->slots) { store->table_free(st->slots); st->slots = nullptr; }
      void* mem = store->table_alloc<uint2>(slots);
      metrics.tables_built++;
      a.gslots = static_cast<uint2*>(mem);
      RDFGPU_HIP(hipMemsetAsync(a.gslots, 0xFF, (size_t)slots * sizeof(uint2), stream));
      timed(KC_GJOIN_BUILD, 0, B.cap, B.n_dev, 4ull * a.n_keys + 8, nullptr, 0, 0, [&] { launch_gjoin_build(a, stream); });
      RDFGPU_HIP(hipStreamSynchronize(stream)); metrics.host_syncs++;
      st->slots = mem; st->mask = a.tbl_mask;
    }
    a.gslots = static_cast<uint2*>(st->slots);
    return JoinTable::SliceHash;
  }
  if (a.n_keys <= 2 && !j.probe_filter && !j.post_filter && !opt.on(RDFGPU_OPT_NO_PARTITIONED_JOIN) && B.cap >= opt.v[RDFGPU_OPT_PARTITION_MIN_BUILD] &&
      B.cap < (1ull << 31) && P.cap < (1ull << 31))
    return JoinTable::Partitioned;
  // The direct-address form for a build side that is NOT cached (RDFGPU_OPT_NO_TABLE_CACHE, or an intermediate with a host-known row
  // count): built inside this execution, in scratch memory, when the single key turns out unique over a dense id range.  4 bytes per ID
  // instead of 8 bytes per SLOT at load <= 0.5: the 285 k-row property slices of BSBM-100M are 1.1 MB (resident in every XCD's L2)
  // instead of an 8 MB hash table that 0.54 G random probes fetch from the Infinity Cache line by line.  A large probe side pays for
  // the two host round trips with every probe that hits a 4-byte entry in L2 instead of an 8-byte slot beyond it.
  if (a.n_keys == 1 && B.n_dev == nullptr && B.cap >= 4096 && P.cap >= (1ull << 22) && !j.nd.transient_direct_failed && !opt.on(RDFGPU_OPT_NO_DIRECT_TABLE)) {
    const DirectTable d = build_direct(a.build_key[0], B.cap, 4 * B.cap + 1024, false);   // (sparse ids: not even tried)
    j.nd.transient_direct_failed = !d.direct;
    if (d.direct) { metrics.tables_built++; a.direct = d.direct; a.direct_min = d.kmin; a.direct_n = d.kn; return JoinTable::TransientDirect; }
  }
  a.gslots = scratch<uint2>(slots);   // (filled by the build pass in exec_lds_join)
  RDFGPU_HIP(hipMemsetAsync(a.gslots, 0xFF, (size_t)slots * sizeof(uint2), stream));
  return JoinTable::ScratchHash;
}

// Candidate queue per wave: a full queue costs one output reservation (a same-address atomic, ~88 per
// microsecond chip-wide), an oversized one costs occupancy (8 queues x 8 B x entries of LDS per workgroup).
// Sized from the matches a wave can expect out of one tile (64 x rows-per-lane probe rows), which is what a
// workgroup of an HBM-table join sees in its whole life; "expected" = the previous execution's cardinality
// when known, else one match per probe row.  A direct-address table has at most one match per row.
void Plan::size_wave_queue(LdsJoin& j) {
  const NodeInfo& nd = j.nd;
  const u64 np = j.P.cap;
  LdsJoinArgs& a = j.a;
  const u32 q_env = (u32)opt.v[RDFGPU_OPT_JOIN_WAVE_Q];
  const u64 per_tile = 64ull * (u64)lds_join_items(np << a.row_lanes_log2, j.global_table);
  const u64 expect = nd.has_last ? nd.last_rows : np;
  const u64 want = a.direct ? per_tile : (expect * per_tile * 3 / 2) / (np ? np : 1);
  u32 q = 256;
  while (q < want && q < 1024) q <<= 1;
  if (!j.global_table && (size_t)j.slots * sizeof(uint2) > 64 * 1024) q = 256;
  a.wave_q = q_env ? q_env : q;
  // partitioned join: a sparse output (the previous execution found less than one match per 8 probe rows) needs no deep queues —
  // 52 KB of LDS per workgroup instead of 64: three workgroups per CU instead of two
  if (j.table == JoinTable::Partitioned) a.wave_q = nd.has_last && !nd.last_scaled && nd.last_rows * 8 < np ? 64 : 256;
}

// One launch of the join kernel: the partitioned join, the streaming form over a direct table, or lds_join_kernel.  Bytes: the
// build side's when every workgroup builds the table, `stage_bytes` of a fused chain, `out_bytes_per_row` per output row.
void Plan::run_join_kernel(LdsJoin& j, u64 stage_bytes, u64 out_bytes_per_row) {
  LdsJoinArgs& a = j.a;
  const DevTable& B = j.B; const DevTable& P = j.P;
  // SURVEY 8d hash-join bytes of a partitioned join: both sides' key + payload columns and one 8-byte slot per row, the output;
  // the partition passes are in the time of the operator, not in its bytes
  if (j.table == JoinTable::Partitioned) {
    timed(KC_PART_JOIN, j.build_bytes, P.cap, P.n_dev, 4ull * j.probe_cols + 8, a.n_out_dev, 0, out_bytes_per_row, [&] { launch_part_join(a, j.part, stream); });
    return;
  }
  const bool streamed = a.stream_direct && direct_stream_join_ok(a);
  // the streaming form over a direct table, window filter on ONE build column against probe columns, a probe side large enough to pay
  // for a kernel and a host round trip: that column decoded per KEY (a.key_vals), once per execution
  if (streamed && !j.stream_values_tried && a.direct && a.has_filter == 3 && a.has_probe_filter == 0 && B.n_dev == nullptr && a.tt.n_ids != 0 &&
      direct_stream_join_items(P.cap) == 8 && P.cap >= (1ull << 22) && !opt.on(RDFGPU_OPT_NO_VALUE_TABLES)) {
    j.stream_values_tried = true;
    if (a.win.x0 == a.win.x1 && on_build_side(a, a.win.x0) && !on_build_side(a, a.win.y0) && !on_build_side(a, a.win.y1)) {
      long long* vals = scratch<long long>(a.direct_n);
      u32* bad = reinterpret_cast<u32*>(new_counter());
      launch_fill_i64(vals, INT64_MIN, a.direct_n, stream);
      launch_direct_values(a.build_key[0], a.cols[a.win.x0], B.cap, a.direct_min, a.direct_n, a.tt, vals, bad, stream);
      if (!read_back<u32>(bad)) {
        a.key_vals = vals; metrics.tables_built++;
        a.stream_need_build_row = (a.has_post && on_build_side(a, a.post.col)) ? 1u : 0u;
        for (u32 c = 0; c < j.nd.n_proj; c++) if (on_build_side(a, j.nd.proj[c])) a.stream_need_build_row = 1u;
      }
    }
  }
  const int kc = streamed ? (int)KC_STREAM_JOIN
                          : lds_join_class(a.has_filter, a.has_probe_filter, lds_join_items(P.cap << a.row_lanes_log2, j.global_table), lds_join_mode(a), a.n_chain != 0);
  timed(kc, (j.global_table ? 0 : j.build_bytes) + stage_bytes, P.cap, P.n_dev, 4ull * j.probe_cols + 8, a.n_out_dev, 0, out_bytes_per_row, [&] { launch_lds_join(a, stream); });
}

// Speculative mode: the output sized from history (`size_node`: this join's, or the top node's of a fused chain) or from the
// table form's guess; nothing is waited for.  j.use_band: the fused chain runs as a band join.
DevTable Plan::run_speculative(LdsJoin& j, u64 first_guess, NodeInfo& size_node) {
  LdsJoinArgs& a = j.a;
  DevTable& t = j.t;
  const u64 spec_cap = j.nd.has_last ? std::max<u64>(1024, size_node.last_rows + size_node.last_rows / (size_node.last_scaled ? 2 : 4) + 256)   // 25 % head room over the previous run (50 % over an extrapolation)
                                     : std::max<u64>(1024, first_guess);
  a.out_cap = spec_cap;
  for (u32 c = 0; c < a.n_out_cols; c++) { a.out[c] = scratch<u32>(spec_cap + j.tail); t.cols[c] = a.out[c]; }
  if (j.left_join) RDFGPU_HIP(hipMemsetAsync(a.visited, 0, j.L.cap, stream));
  j.out_node = &size_node;
  if (j.use_band) exec_band_join(j);
  else if (!run_ordered_join(j, size_node, spec_cap)) run_join_kernel(j, j.stage_bytes, 4ull * a.n_out_cols);
  const SpecCheck check{&size_node, (u32)(a.n_out_dev - counters), j.left_join};
  if (pending_oj.active && !pending_oj.counted && pending_oj.o.n_out_dev == a.n_out_dev) pending_oj.check = check;   // nothing writes that count unless the count pass runs after all
  else spec_checks.push_back(check);
  t.cap = spec_cap + j.tail; t.n_dev = a.n_out_dev;
  if (j.left_join) left_join_tail(j.nd, j.L, j.R, a.out, a.visited, a.n_out_dev, spec_cap + j.tail);
  return t;
}

// A small table against a CSR slice that is sorted by another column, with an output about as large as the slice:
// the matches are emitted in the slice's order (ordered_join.hip) — what consumes them partitioned by that column
// (the band join above) then has nothing to sort; the chain's look-ups by table columns run once per table row.
// false: the join does not have that shape (nothing launched).
bool Plan::run_ordered_join(LdsJoin& j, const NodeInfo& size_node, u64 spec_cap) {
  const LdsJoinArgs& a = j.a;
  const DevTable& B = j.B; const DevTable& P = j.P;
  if (j.probe_outer || opt.on(RDFGPU_OPT_NO_ORDERED_JOIN) || !a.csr_off || a.range_rows || j.left_join || a.has_filter != 0 || a.has_probe_filter || a.has_post ||
      a.n_keys != 1 || B.sorted_col < 0 || (u32)B.sorted_col == j.build_keys[0] || B.n_dev || !B.stable_id || B.cap >= (1ull << 32) || P.cap > (1ull << 24) ||
      !size_node.has_last || size_node.last_rows * 8 < B.cap)
    return false;
  for (u32 s = 0; s < a.n_chain; s++) if (a.chain[s].key.src != 0 || a.chain[s].fs != 0) return false;
  u32 from_table = 0;   // output columns taken from the table row or a stage row travel in its packed record: at most 8
  for (u32 c = 0; c < a.n_out_cols; c++) from_table += a.n_chain ? a.chain_out[c].src != 1 : !on_build_side(a, a.proj[c]);
  if (from_table > 8 || a.n_out_cols > kOjMaxOutCols) return false;
  DevTable& t = j.t;
  OrderedJoinArgs o{};
  o.build_key = a.build_key[0]; o.n_build = B.cap;
  o.probe_key = a.probe_key[0]; o.n_probe_dev = P.n_dev; o.n_probe_cap = P.cap;
  o.kmin = a.direct_min; o.kn = a.direct_n;
  o.n_stages = a.n_chain;
  for (u32 s = 0; s < a.n_chain; s++) o.stage[s] = OrderedJoinStage{a.chain[s].key.ptr, a.chain[s].direct, a.chain[s].kmin, a.chain[s].kn, nullptr};   // (the multimap, the stage rows and the packed records: probe_ordered_join)
  o.n_out_cols = a.n_out_cols;
  u32 n_words = 0;
  for (u32 c = 0; c < a.n_out_cols; c++) {
    if (a.n_chain) o.out_ref[c] = a.chain_out[c];
    else { const u32 pc = a.proj[c]; o.out_ref[c] = ColRef{a.cols[pc], on_build_side(a, pc) ? 1u : 0u, 0u}; }
    o.out[c] = a.out[c];
    o.out_slot[c] = o.out_ref[c].src == 1 ? (u8)0xFF : (u8)n_words++;
    if (o.out_ref[c].src == 1 && o.out_ref[c].ptr == B.cols[B.sorted_col] && t.sorted_col < 0) { t.sorted_col = (int)c; t.key_min = B.key_min; t.key_max = B.key_max; }
  }
  o.n_rec = n_words > 4 ? 2u : 1u;
  o.out_cap = spec_cap; o.n_out_dev = a.n_out_dev; o.overflow = a.overflow;
  // the consumer is a band join that (last time) found this output sorted by its key and needed nothing else of it: the write
  // pass is held back — that join has it write its row records instead of this table (exec_band_join), anything else flushes it.
  // If that join also read the slice's rows in place last time and no key had two table rows, the count pass waits as well:
  // the in-place records do not need it (OjInPlace); whatever else takes the table runs it first (count_pending_oj)
  const int consumer = size_node.parent;
  const bool held = consumer >= 0 && nodes[consumer].band.takes_records && !pending_oj.active && t.sorted_col >= 0;
  // (NO_BAND_COMPACT switches it off: the in-place records are the 16-byte ones)
  const bool in_place = held && nodes[consumer].band.in_place && nodes[consumer].band.multi_rows == 0 && !opt.on(RDFGPU_OPT_NO_BAND_COMPACT);
  if (held) o.multi_rows = reinterpret_cast<u32*>(new_counter());
  // (.. and with the rows' windows cached on the slice last time, only the table rows' output values travel by key)
  // Such a step takes nothing else from the table, and which column the value is the band join alone knows (take_pending_oj): the probe pass is OWED — nothing is
  // launched here, the band join runs the values-by-key pass in its place, or count_pending_oj the full one when the step takes another form after all
  OjProbeShape probe;
  probe.held = held; probe.in_place = in_place; probe.row_cache = consumer >= 0 && nodes[consumer].band.row_cache; probe.option_off = !opt.on(RDFGPU_OPT_NO_BAND_ROW_CACHE);
  probe.row_static = true;   // (what the flags promise; the step's own form is known where the debt is settled)
  const bool owed = oj_probe_form(probe) != OjProbeForm::FULL;
  if (owed) o.key_val = scratch<u32>(a.direct_n);
  else if (in_place) o.key_rec = scratch<uint4>(a.direct_n);
  if (!owed) probe_ordered_join(o);
  if (!in_place) count_ordered_join(o);
  if (held) {
    pending_oj.active = true; pending_oj.o = o; pending_oj.first_col = a.out[0]; pending_oj.n_build = B.cap;
    pending_oj.counted = !in_place; pending_oj.rows_seen = size_node.last_rows; pending_oj.probe_owed = owed; pending_oj.probe = probe;
  } else timed(KC_OJ_WRITE, 0, B.cap, nullptr, 4, a.n_out_dev, 0, 8ull * a.n_out_cols, [&] { launch_ordered_join_write(o, stream); });
  return true;
}

// Exact mode: the output sized from the table form, the count read back; a second attempt with room for all if it did not fit.
DevTable Plan::run_exact(LdsJoin& j) {
  NodeInfo& nd = j.nd;
  LdsJoinArgs& a = j.a;
  const DevTable& B = j.B; const DevTable& P = j.P;
  DevTable& t = j.t;
  u64 out_cap = P.cap < 1024 ? 1024 : P.cap;   // optimistic: at most one match per probe row on average
  if (a.csr_off) out_cap = std::max<u64>(out_cap, 2 * P.cap * ((B.cap + a.direct_n - 1) / (a.direct_n ? a.direct_n : 1)) + 1024);   // CSR: twice the mean rows per key
  u64 total = 0;
  for (int attempt = 0; attempt < 2; attempt++) {
    a.out_cap = out_cap;
    for (u32 c = 0; c < nd.n_proj; c++) { a.out[c] = scratch<u32>(out_cap + j.tail); t.cols[c] = a.out[c]; }
    if (j.left_join) RDFGPU_HIP(hipMemsetAsync(a.visited, 0, j.L.cap, stream));
    run_join_kernel(j, 0, 4ull * nd.n_proj);
    const u32 i0 = (u32)(a.n_out_dev - counters);
    read_back(ctx->counters_host + i0, counters + i0, 2 * sizeof(u64));
    total = ctx->counters_host[i0];
    const bool ovf = (ctx->counters_host[i0 + 1] & 0xFFFFFFFFull) != 0;
    if (!ovf) break;
    if (attempt == 1) fail(RDFGPU_ERR_DEVICE, "LDS join overflowed its exact-size output");
    out_cap = total;   // the count is exact even when the writes did not fit: run again with room for all
    RDFGPU_HIP(hipMemsetAsync(a.n_out_dev, 0, 2 * sizeof(u64), stream));
  }
  nd.last_rows = total; nd.has_last = true; nd.last_scaled = false;   // history for the next (speculative) execution
  t.cap = total + j.tail;
  if (!j.left_join) { if (total == 0) t.cap = 0; return t; }
  left_join_tail(nd, j.L, j.R, a.out, a.visited, a.n_out_dev, 0);
  t.n_dev = a.n_out_dev;
  return t;
}

// Left join tail: the build (left) rows no probe row visited, nulls on the right, appended at the device count `n_out_dev`.
// `matched_total`: the capacity of the output columns when the count is not known on the host (0 = unchecked).
void Plan::left_join_tail(const NodeInfo& nd, const DevTable& L, const DevTable& R, u32* const* out, u8* visited, u64* n_out_dev, u64 matched_total) {
  JoinArgs ja{};
  for (u32 c = 0; c < L.n_cols; c++) ja.left[c] = L.cols[c];
  ja.n_left_cols = L.n_cols; ja.n_right_cols = R.n_cols; ja.n_out_cols = nd.n_proj;
  for (u32 c = 0; c < nd.n_proj; c++) { ja.proj[c] = nd.proj[c]; ja.out[c] = out[c]; }
  ja.n_left_dev = L.n_dev; ja.n_left_cap = L.cap;
  ja.visited = visited; ja.n_out_dev = n_out_dev; ja.matched_total = matched_total;
  timed(KC_LEFT_TAIL, 0, L.cap, L.n_dev, 1, nullptr, 0, 0, [&] { launch_join_left_unmatched(ja, stream); });
}

// Radix partitioning of both sides of a HashJoinExec by the top bits of the key hash (part_join.hip): per side one pass
// that computes (partition, {row, key0, key1}) per row, one rocPRIM radix sort moving the 12-byte records, one pass that
// finds the partition boundaries.  Rows with a null key (NullEqualsNothing) or beyond the live row count ride in the last
// partition, marked (row = kNil) so that the join skips them.
void Plan::prepare_partitions(const LdsJoinArgs& a, const DevTable& B, const DevTable& P, PartArgs& pa) {
  u32 bits = 0;
  u32 target_rows = kPartTargetRows, part_slots = kPartSlots;
  // a join with a large output is bound by the latency of its gathers (part_join.hip, BIG): a 2048-slot table (24 KB) lets three
  // workgroups share a CU instead of two — 8.25 -> 7.5 ms on the 0.54 G-row candidate join of BSBM Q5 (profiles/tools/nc_variants.py)
  if (pa.two_pass) { part_slots = 2048; target_rows = 512; }
  if (opt.v[RDFGPU_OPT_PARTITION_SLOTS]) {
    const u64 v = opt.v[RDFGPU_OPT_PARTITION_SLOTS];
    if (v < 1024 || v > 8192 || (v & (v - 1))) fail(RDFGPU_ERR_INVALID, "PARTITION_SLOTS = %llu (a power of two from 1024 to 8192)", (unsigned long long)v);
    part_slots = (u32)v; target_rows = part_slots / 4;
  }
  if (opt.v[RDFGPU_OPT_PARTITION_ROWS]) target_rows = (u32)std::min<u64>(opt.v[RDFGPU_OPT_PARTITION_ROWS], part_slots / 2);
  while (bits < 16 && (B.cap >> bits) > target_rows) bits++;   // <= 16 bits = two radix passes; larger partitions are joined chunk by chunk
  const u32 n_parts = 1u << bits;
  pa.n_parts = n_parts; pa.chunk = part_slots / 2; pa.tbl_mask = part_slots - 1;
  // The probe side is a store slice sorted by one of the join keys (and every row of it is live): its partitions are KEY RANGES
  // of that column — contiguous pieces of the slice, found by one binary search per partition and read in place; only the
  // build side goes through the partition sort (LUBM Q9's closing join: 98 M of 327 M rows).
  PartKeyRange kr{-1, 0u, 0u, 0u, 0u, nullptr};
  if (!opt.on(RDFGPU_OPT_NO_RANGE_PARTITION) && P.sorted_col >= 0 && !P.n_dev && P.cap && P.key_min >= 1 && P.key_max >= P.key_min && n_parts >= 4)
    for (u32 k = 0; k < a.n_keys && kr.range < 0; k++)
      if (P.cols[P.sorted_col] == a.probe_key[k]) {
        // id ranges are not row ranges (LUBM: undergraduate and graduate courses share the slice, at different rows per id):
        // a coarse directory over the id range hands every bucket partitions in proportion to the slice rows in it
        const u64 span = (u64)P.key_max - P.key_min + 1;
        const u32 n_coarse = std::min<u32>(4096u, n_parts / 4);
        u32 cshift = 0;
        while (((span - 1) >> cshift) >= n_coarse) cshift++;
        uint2* dir = scratch<uint2>((u64)n_coarse + 1);
        kr = PartKeyRange{(int)k, P.key_min, P.key_max, cshift, n_coarse, dir};
        timed(KC_BAND_BOUNDS, 0, n_coarse, nullptr, 0, nullptr, 0, 0, [&] { launch_part_equalise(a.probe_key[k], P.cap, kr, n_parts, dir, stream); });
      }
  auto side = [&](const DevTable& T, const u32* const* keys, const PartRec*& recs, const u32*& start, PartKeyRange r) {
    const u64 n = T.cap;
    u32* st = scratch<u32>((u64)n_parts + 2);
    if (!opt.on(RDFGPU_OPT_NO_OWN_PARTITION_PASS)) {   // hand-written MSD passes that recompute the partition from the keys (part_pass.hip)
      const PartPassPlan pl = part_pass_plan(n, bits);
      PartPassBuffers w{};
      w.recs = scratch<PartRec>(n); w.recs_a = pl.two ? scratch<PartRec>(n) : nullptr;
      w.pid16 = scratch<unsigned short>(n); w.digit = pl.two ? scratch<unsigned char>(n) : nullptr;
      w.hist_a = scratch<u32>(pl.hist_a);
      w.total = scratch<u32>((u64)std::max<u32>(pl.nb_a, n_parts) + 2); w.base_a = scratch<u32>((u64)pl.nb_a + 2);
      if (pl.two) {
        w.hist_b = scratch<u32>(pl.hist_b);
        w.tiles_b = scratch<unsigned char>(pl.tile_desc_bytes); w.n_tiles_b = scratch<u32>(1);
      }
      w.tb = scratch<u32>((u64)pl.nb_a + 2);
      w.start = st;
      const size_t tb = scan_temp_bytes((u64)n_parts + 2);
      void* temp = scratch<unsigned char>(tb);
      timed(KC_PART_PASS, 0, n, T.n_dev, 0, nullptr, 0, 0, [&] { part_pass_run(w, pl, keys[0], a.n_keys > 1 ? keys[1] : nullptr, a.n_keys, T.n_dev, n, bits, n_parts, r, temp, tb, stream); });
      recs = w.recs; start = st;
      return;
    }
    u32* skey_in = scratch<u32>(n); u32* skey = scratch<u32>(n);
    PartRec* sval_in = scratch<PartRec>(n); PartRec* sval = scratch<PartRec>(n);
    const size_t tb = part_sort_temp_bytes(n, bits ? bits : 1);
    void* temp = scratch<unsigned char>(tb);
    timed(KC_PART_KEYS, 0, n, T.n_dev, 0, nullptr, 0, 0, [&] { launch_part_keys(keys[0], a.n_keys > 1 ? keys[1] : nullptr, a.n_keys, T.n_dev, n, bits, n_parts, r, skey_in, sval_in, stream); });
    timed(KC_RADIX_SORT, 0, n, nullptr, 0, nullptr, 0, 0, [&] { part_sort(skey_in, skey, sval_in, sval, n, bits ? bits : 1, temp, tb, stream); });
    timed(KC_BAND_BOUNDS, 0, n_parts, nullptr, 0, nullptr, 0, 0, [&] { launch_sorted_bounds(skey, n, n_parts, st, stream); });
    recs = sval; start = st;
  };
  side(B, a.build_key, pa.bpart, pa.bstart, kr);
  if (kr.range >= 0) {
    u32* st = scratch<u32>((u64)n_parts + 2);
    timed(KC_BAND_BOUNDS, 0, n_parts, nullptr, 0, nullptr, 0, 0, [&] { launch_part_range_bounds(a.probe_key[kr.range], P.cap, kr, n_parts, st, stream); });
    pa.ppart = nullptr; pa.pstart = st; pa.pcol0 = a.probe_key[0]; pa.pcol1 = a.n_keys > 1 ? a.probe_key[1] : nullptr;
  } else side(P, a.probe_key, pa.ppart, pa.pstart, kr);
}

}  // namespace rdfgpu
