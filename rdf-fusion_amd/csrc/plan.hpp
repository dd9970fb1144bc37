// plan.hpp — compiled operator tree: DataSourceExec / FilterExec / HashJoinExec / CrossJoinExec /
// NestedLoopJoinExec / ProjectionExec over HBM-resident binding tables.
#pragma once
#include <memory>
#include <shared_mutex>
#include <string>
#include <vector>

#include "host_logic.hpp"
#include "kernels.hpp"
#include "store.hpp"

namespace rdfgpu {

struct SourceInfo {               // one DataSourceExec
  u32 node = 0;
  u32 components = RDFGPU_GSPO;   // chosen permutation (IndexPermutations::choose_index)
  ScanInstructions ix;            // instructions in the order of `components`
  PrunePlan prune;
  bool has_residual = false;      // predicates left after pruning => K2 compaction, else zero-copy slice
  u32 n_out = 0;
  u32 out_level[4] = {};          // index level feeding output column k (G,S,P,O order of first binding)
  u64 lo = 0, hi = 0;             // located range of the last execution
  u32 sorted_level = 4, key_min = 0, key_max = 0;   // the level sorted within [lo, hi) and its first / last id (4: none)
  ScanInstructions gspo;          // the pattern's instructions in G,S,P,O order, push-down filters folded in
  std::vector<std::pair<u32, ScanPredicate>> dynamic;   // current dynamic filters: (variable slot, predicate)
  bool dynamic_dirty = false;     // the effective instructions have to be derived again before the next execute
};

// What the band join based on a node keeps from one execution to the next: measurements, written by Plan::record_band_history, and two route flags.
struct BandHistory {
  bool ran = false; u64 slow_rows = 0;   // record_band_history: it ran; probe rows that needed the full typed-value semantics.  exec_band_join: ran and 0 = the full-semantics pass is not launched
  u64 blocks = 0;               // record_band_history: its blocks (counted on the device; in place: known on the host).  exec_band_join sizes the block kernels' launch from it
  u64 run_stats = 0;            // record_band_history: sampled rows << 32 | runs of equal neighbouring probe keys.  exec_band_join: a piecewise sorted probe side takes the counting partition
  u64 multi_rows = 0;           // record_band_history: table rows the ordered slice join that wrote this join's records met behind another of the same key.  run_ordered_join: 0 = it may skip its count pass
  bool takes_records = false;   // exec_band_join: the probe side came presorted from an ordered slice join and no row needed the slow pass.  run_ordered_join / keeps_pending_oj: that join holds its write pass back
  bool in_place = false;        // exec_band_join: the slice's block layout is cached, the in-place route is available.  run_ordered_join reads it with multi_rows
  bool row_cache = false;       // exec_band_join: the rows' decoded windows are cached on the slice too (SliceTable::BandRowWindows).  run_ordered_join: its probe pass prepares the values by key, not the 16-byte records
};

// Where an output column's values come from (RDFGPU_PLAN_AGG_COLUMNS): node < 0 = an object-id column; else the column holds 1-based
// indexes into value array `agg` of `node` (0 = unbound) — aggregate `agg` of an AggregateExec, or expression `agg` of a ProjectionExec
// with expressions (RDFGPU_NODE_EXTEND).  Fixed at compile, carried through every operator above.
// The mark column of a LeftMark join (RDFGPU_JOIN_LEFT_MARK) is value array 0 of the join node: two records, false and true.
struct ValueOrigin { int node = -1; u32 agg = 0; bool extend = false; bool mark = false; };   // extend / mark: `node` is an EXTEND / a LeftMark join (for the refusals' texts)

struct NodeInfo {
  rdfgpu_plan_node d;
  u32 width = 0;                  // output columns
  ValueOrigin origin[kMaxCols];   // per output column: the aggregate whose values it indexes, if it is a value column
  u32 n_proj = 0; u32 proj[kMaxCols] = {};
  ExprProgram prog{};             // filter / join filter
  int shape = 0;                  // filter kernel specialisation
  bool lex = false;               // a program of the node holds an op with kOpExtended (a lexical cast of a literal, a date part, IF, COALESCE, a term test): its host runs the instantiation with those cases compiled in
  u32 n_enc_tv = 0;               // ENC_TV gathers per row (algorithmic bytes)
  u32 n_cols_read = 0;            // distinct input columns the kernel has to read
  int source = -1;                // index into Plan::sources
  u32 refs = 0;                   // how many operators consume this node
  u64 last_rows = 0; bool has_last = false;   // output cardinality of the previous execution (speculative sizing)
  bool last_scaled = false;                    // .. extrapolated from a priming run over a prefix of the bound tables (Plan::prime), not measured
  bool transient_direct_failed = false;        // a build side that is not cached turned out not to be unique and dense: do not try the direct-address form again
  int parent = -1;                             // the one operator consuming this node (-1: the root, or several)
  u32 n_aggs = 0; u32 agg_fn[RDFGPU_MAX_AGGREGATES] = {}, agg_col[RDFGPU_MAX_AGGREGATES] = {};   // AggregateExec: (RDFGPU_AGG_*, input column)
  int agg_prog[RDFGPU_MAX_AGGREGATES] = {-1, -1, -1, -1, -1, -1, -1, -1};                           // .. or the index in agg_progs of its input expression (RDFGPU_AGG_INPUT_EXPR)
  std::vector<ExprProgram> agg_progs;             // .. and, of a ProjectionExec with expressions (RDFGPU_NODE_EXTEND), the program of every computed column
  rdfgpu_agg_value* values[RDFGPU_MAX_AGGREGATES] = {}; u64 n_values = 0, values_run = 0;   // AggregateExec / EXTEND: the value arrays (scratch) of execution `values_run` (Plan::run) and their length = its groups / rows
  const u64* n_values_dev = nullptr;              // EXTEND over an input counted on the device only: n_values is the capacity while the plan runs (no entry exceeds the rows written) and becomes this count when it has come back
  BandHistory band;                            // the band join based on this node, if there was one
  u32 sort_words = 0;                          // SortExec: 64-bit words of its key record, the row index included (compile_sort)
};
struct SpecCheck { NodeInfo* node; u32 counter; bool left_join; };   // counter = n_out slot, counter+1 = overflow flag

// A run of inner single-key joins above a base join whose other inputs are store slices with cached direct-address
// tables: handed to the base join, which runs them inside its resolve phase (kernels.hpp ChainStage).
struct ChainLink { NodeInfo* node; bool slice_is_left; DevTable slice; const SliceTable* table; };
struct ChainRequest { NodeInfo* top = nullptr; NodeInfo* base = nullptr; std::vector<ChainLink> links /* bottom-up */; bool consumed = false; };

// An ordered slice join whose write pass is held back: its consumer, a band join, may have it write the band join's row
// records instead of the output table (OjBandFuse); anything else flushes it (Plan::flush_pending_oj) first.
// counted = false: its count pass has not run either (the band join may read the slice's rows in place, OjInPlace); whatever
// else takes the table runs it first (Plan::count_pending_oj) and registers `check`, the check of the count it writes.
// rows_seen: that join's last measured output rows (how much of the slice the band join's in-place form would leave idle).
// probe_owed: its probe pass has not run either, and o holds none of head, next, trec and the stage rows (host_logic.hpp, oj_probe_form, asked with `probe`): the band
// join runs the values-by-key pass in its place (band_row_records), or count_pending_oj the full one.  An owed probe implies !counted.
struct PendingOj {
  bool active = false; OrderedJoinArgs o{}; const u32* first_col = nullptr; u64 n_build = 0; bool counted = true; SpecCheck check{}; u64 rows_seen = 0;
  bool probe_owed = false; OjProbeShape probe{};
};

struct BoundTable { std::vector<const u32*> cols; u64 n_rows = 0; bool bound = false; };

// The table an LDS join probes (Plan::choose_join_table).
enum class JoinTable {
  Lds,                                 // built by every workgroup in its own LDS
  SliceCsr, SliceDirect, SliceHash,    // a store slice's table, built once per store version and kept on the store
  Partitioned,                         // both sides radix-partitioned, every partition's table built in LDS (part_join.hip)
  TransientDirect, ScratchHash         // direct-address / hash table in HBM, built inside this execution
};

// One HashJoinExec on the LDS-join path while it is set up and run (Plan::exec_lds_join and its steps).
struct LdsJoin {
  NodeInfo& nd;
  const DevTable& L; const DevTable& R;
  const bool build_left;
  const DevTable& B; const DevTable& P;
  const NodeInfo* probe_filter;        // a FilterExec of the probe side run inside the probe
  const NodeInfo* post_filter;         // a FilterExec of the build side kept as a conjunct of the join filter
  // a LEFT join built on its right input preserves its PROBE side (choose_build_left): for everything below it is an inner join whose
  // kernel adds one null-extended row per unmatched probe row — no visited flags, no tail pass
  const bool probe_outer, left_join;
  LdsJoinArgs a{};
  u32 build_keys[RDFGPU_MAX_KEYS] = {}, probe_keys[RDFGPU_MAX_KEYS] = {};
  u32 probe_cols = 0, build_payload = 0;   // columns the kernel reads on the probe side; build columns besides the keys
  u64 build_bytes = 0;                     // SURVEY §8d hash join, build half: 4(k+p_b)N_b + 8N_b (the 8-byte slot in LDS)
  u32 slots = 64;                          // hash table slots (LDS or HBM)
  bool global_table = false;               // one table in HBM / L2 instead of a copy per workgroup in LDS
  JoinTable table = JoinTable::Lds;
  SliceTable* slice = nullptr;             // the store-level tables of a slice build side
  PartArgs part{};
  u64 tail = 0;                            // left join: output rows reserved for the unmatched build rows
  bool stream_values_tried = false;
  u64 stage_bytes = 0;                     // a fused chain of lookups above this join (Plan::apply_chain): what its stages read (estimate)
  std::vector<ColRef> chain_cols; SliceTable::ValueColumn chain_vc[kMaxChain] = {};   // .. its output columns (bottom-up, while it is resolved into a.chain / a.chain_out); the decoded value table a stage's window reads (a copy; val == nullptr: none)
  BandArgs band{}; bool use_band = false;  // the chain runs as a band join (Plan::exec_band_join), with these arguments
  DevTable t;                              // the output
  const NodeInfo* out_node = nullptr;      // the node the output belongs to: this join's, or the top node's of a fused chain (set by run_speculative)
  LdsJoin(NodeInfo& n, const DevTable& l, const DevTable& r, bool bl, const NodeInfo* pf, const NodeInfo* post)
      : nd(n), L(l), R(r), build_left(bl), B(bl ? l : r), P(bl ? r : l), probe_filter(pf), post_filter(post),
        probe_outer(n.d.join_type == RDFGPU_JOIN_LEFT && !bl), left_join(n.d.join_type == RDFGPU_JOIN_LEFT && bl) {}
};

// One band join while it is set up and run (Plan::exec_band_join and its steps): the fused chain of `j`, its kernel arguments (left by apply_chain) in j.band.
struct BandJoin {
  LdsJoin& j; const u32 kn; const u64 np, nb, cmax;   // keys of the build side's CSR table (key kn = joins nothing); probe rows (capacity), build rows; 64-entry pieces of its largest group
  bool presorted = false;              // route: the probe side arrives sorted by the key (an ordered slice join below): nothing to partition.  Its keys may not lie below the table's range: they would map to "joins nothing" (= kn, the largest) out of order
  bool skip_slow = false;              // route: the previous execution met no row that needed the full-semantics pass: it is not launched
  bool counting = false;               // route: not sorted, but small or piecewise sorted (>= 4 rows per run of equal neighbouring keys last time, the N sorted runs a repartition delivers): counting sort on the key, one atomic per run, instead of the radix sort
  bool fused = false;                  // route: the held-back ordered slice join below writes this join's row records itself (OjBandFuse)
  bool in_place = false;               // route: .. without counting its matches: the rows of key k are the slice's own CSR group k (OjInPlace)
  bool cache_entries = false;          // the build side is a store slice: its decoded entries and block layout are kept on its SliceTable
  OjBandFuse fuse{};                   // fused: where the ordered join's packed record holds what this join reads of a row
  std::string ekey; SliceTable::BandEntries lay{};   // what the decoded entries depend on, spelt out (SliceTable::BandEntries::key); a copy of the slice's in-place block layout (boff == nullptr: there is none, the route is closed)
  SliceTable::BandRowWindows rw{};     // what the slice keeps of the row side for this chain and this plan's options accept (band_row_windows; a copy without the key, as `lay` is of the
                                       // layout): row_win (null: not eligible, declined, or the route is closed), and behind it pair_bits, and behind them the list with its counts
  BandForm form = BandForm::RECORDS;   // route: which way the block passes run and what they read (host_logic.hpp, band_step_form; the table: band_join.hip).  Every form but RECORDS is in_place
  bool row_static() const { return form != BandForm::RECORDS; }   // .. the rows come as the slice's cached windows and this execution's values by key, not as 16-byte records
  u64 nrows = 0, max_blocks = 0;       // probe rows of the block kernels (in place: the slice's own rows); upper bound of the blocks (in place: exact)
  u32* skey = nullptr; u32* perm = nullptr; u32 sort_bits = 1; void* sort_temp = nullptr; size_t sort_temp_bytes = 0;   // the radix sort of the probe keys (its output pairs, key bits, temp): allocated by band_probe_side, run by band_blocks_and_emit
  BandJoin(LdsJoin& join) : j(join), kn(join.a.direct_n), np(join.P.cap), nb(join.B.cap), cmax((join.slice->csr_max_group + 63) / 64) {}
};

// The tiers of a slice's BandRowWindows entry as one step meets them (Plan::band_row_windows): use_* = this plan's options accept the tier (the windows are used wherever
// the entry has them); build_* = accepted and missing — launched behind one another before the step's one wait.
struct BandRowTiers { bool build_windows = false, build_verdicts = false, build_list = false, use_verdicts = false, use_list = false; };

// Kernel classes for per-kernel timing; names are what rocprofv3 --kernel-trace prints.
enum KernelClass {
  KC_LOCATE, KC_SCAN_COUNT, KC_SCAN_WRITE, KC_FILTER_ID, KC_FILTER_TV, KC_FILTER_VM, KC_CROSS, KC_JOIN_BUILD,
  KC_JOIN_COUNT, KC_JOIN_WRITE, KC_LEFT_TAIL, KC_NLJ_COUNT, KC_NLJ_WRITE, KC_DEVICE_SCAN,
  KC_GJOIN_BUILD,
  KC_GDIRECT_BUILD, KC_MINMAX, KC_CSR_HIST, KC_CSR_SCATTER,
  KC_TOPK_MAX, KC_TOPK_HIST, KC_TOPK_SCATTER, KC_TOPK_SELECT, KC_TOPK_WRITE,
  KC_FILTER_VERDICT, KC_REGEX_VERDICTS, KC_UNION,
  KC_BAND_SLOW, KC_RADIX_SORT, KC_BAND_BOUNDS, KC_BAND_BLOCKS, KC_BAND_DECODE, KC_BAND_MASK, KC_BAND_EMIT, KC_BAND_ENTRIES, KC_BAND_DESC, KC_BAND_PT, KC_BAND_ROWS,
  KC_FILTER_BITS_ID, KC_FILTER_BITS_TV, KC_FILTER_BITS_VERDICT, KC_FILTER_BITS_VALUE, KC_VALUE_VERDICTS, KC_VALUE_RUNS, KC_RUN_SCAN, KC_RUN_COPY, KC_OJ_PROBE, KC_OJ_COUNT, KC_OJ_WRITE, KC_FILTER_WRITE,
  KC_PART_KEYS, KC_PART_JOIN, KC_OJ_BAND_RECORDS, KC_OJ_WRITE_BAND, KC_SMALL_SCAN, KC_PART_PASS, KC_STREAM_JOIN, KC_OJ_WRITE_BAND_IN_PLACE,
  KC_SEMI_BUILD, KC_SEMI_JOIN0,      // 6 names: semi_join_kernel<form 0 / 1, anti>, semi_nested_kernel<anti> (semi_join_class)
  KC_SEMI_JOIN_END = KC_SEMI_JOIN0 + 6,
  KC_AGG_GROUPS = KC_SEMI_JOIN_END, KC_AGG_ACCUM_HBM, KC_AGG_ACCUM_LDS, KC_AGG_FINAL,
  KC_AGG_ACCUM_EXPR_HBM, KC_AGG_ACCUM_EXPR_LDS,   // agg_accum_expr_kernel<LDS>: some SUM / AVG reads an expression
  KC_BAND_ROW_WIN_KEYS, KC_BAND_ROW_WIN_ROWS,     // the build of a slice's cached row windows (band_join.hip)
  KC_BAND_PAIR_BITS,                              // .. and of its cached pair verdicts
  KC_BAND_PAIR_LIST_COUNT, KC_BAND_PAIR_LIST_WRITE,   // .. and of the list of their set bits
  KC_AGG_VALUE_COLS,                              // agg_value_cols_kernel: an AggregateExec's value columns (RDFGPU_PLAN_AGG_COLUMNS)
  KC_EXTEND,                                      // extend_kernel: the computed columns of a ProjectionExec with expressions (RDFGPU_NODE_EXTEND)
  KC_SORT_KEYS, KC_SORT_TILE, KC_SORT_MERGE, KC_SORT_GATHER,   // SortExec (sort.hip, RDFGPU_NODE_SORT): records, tile sort, one launch per merge pass, gather
  KC_AGG_ACCUM_MINMAX_HBM, KC_AGG_ACCUM_MINMAX_LDS,             // agg_accum_minmax_kernel<LDS>: some aggregate of the node is a MIN / MAX
  KC_AGG_ACCUM_MINMAX_EXPR_HBM, KC_AGG_ACCUM_MINMAX_EXPR_LDS,   // .. and some SUM / AVG / MIN / MAX reads an expression or a value column
  KC_AGG_MINMAX_REFINE,                                         // agg_minmax_refine_kernel: the low word of the decimal candidates
  KC_OJ_PROBE_VALUES,                                           // oj_probe_kernel(.., OjKeyValues): the probe pass of a step that reads the slice's rows through their cached windows
  KC_AGG_GROUPS_WIDE, KC_AGG_WIDE_KEYS,                         // agg_groups_wide_kernel / agg_wide_keys_kernel: the group pass over value keys or more than 4 keys (RDFGPU_PLAN_VALUE_KEYS), its key copy
  KC_MARK_JOIN0, KC_MARK_JOIN_END = KC_MARK_JOIN0 + 3,          // 3 names: mark_join_kernel<form 0 / 1>, mark_nested_kernel (mark_join_class): LeftMark joins (RDFGPU_JOIN_LEFT_MARK)
  KC_LDS_JOIN0 = KC_MARK_JOIN_END,   // 192 names: lds_join_kernel<FS in {0..3}, PFS in {0,1,2}, ITEMS in {4,1}, MODE in {0,1,2,3}, CHAIN>
  KC__N = KC_LDS_JOIN0 + 192
};
const char* kernel_class_name(int kc);
inline int lds_join_class(u32 fs, u32 pfs, int items, int mode, bool chain = false) {
  return KC_LDS_JOIN0 + (int)((((fs * 3 + pfs) * 2 + (items == 4 ? 0 : 1)) * 4 + mode) * 2) + (chain ? 1 : 0);
}

// Group column k of an AggregateExec: columns 0..3 in left_keys[], 4..7 in right_keys[] (RDFGPU_PLAN_VALUE_KEYS).
inline u32 agg_key_col(const rdfgpu_plan_node& d, u32 k) { return k < RDFGPU_MAX_KEYS ? d.left_keys[k] : d.right_keys[k - RDFGPU_MAX_KEYS]; }

inline int semi_join_class(int form, bool anti) { return KC_SEMI_JOIN0 + form * 2 + (anti ? 1 : 0); }
inline int mark_join_class(int form) { return KC_MARK_JOIN0 + form; }

// The class of the accumulate pass that launch_agg_accum (aggregate.hip) launches for these arguments: the one place that maps
// (minmax, exprs, lds) to a KernelClass.  The LEX kernels (a.exprs == 2: agg_accum_lex_kernel, agg_accum_minmax_lex_kernel) have no
// class of their own: they are reported under the EXPR classes, as they always were.
inline int agg_accum_class(const AggArgs& a) {
  static const int kc[2][2][2] = {{{KC_AGG_ACCUM_HBM, KC_AGG_ACCUM_LDS}, {KC_AGG_ACCUM_EXPR_HBM, KC_AGG_ACCUM_EXPR_LDS}},
                                  {{KC_AGG_ACCUM_MINMAX_HBM, KC_AGG_ACCUM_MINMAX_LDS}, {KC_AGG_ACCUM_MINMAX_EXPR_HBM, KC_AGG_ACCUM_MINMAX_EXPR_LDS}}};
  return kc[a.minmax ? 1 : 0][a.exprs ? 1 : 0][a.lds ? 1 : 0];
}

struct KernelStat { u32 launches = 0; double ms = 0; u64 bytes = 0; u64 rows = 0; };

// One timed launch whose byte count may depend on device-side row counts, resolved after the run.
struct PendingLaunch {
  int kc;
  hipEvent_t start, stop;
  u64 fixed_bytes;      // bytes known on the host
  u64 rows_cap;         // rows streamed if no device count
  const u64* rows_dev;  // device count of streamed rows (or null)
  u64 bytes_per_row;    // multiplied by the live streamed rows
  const u64* out_dev;   // device count of produced rows (or null)
  u64 out_rows;         // produced rows if known on the host
  u64 bytes_per_out;    // multiplied by the produced rows
};

// One AggregateExec while it is set up and run (plan_aggregate.cpp).
struct AggNode {
  NodeInfo& nd; const DevTable& in;
  AggArgs a{};
  bool wide = false; AggWideArgs w{};   // a value key or more than RDFGPU_MAX_KEYS keys (RDFGPU_PLAN_VALUE_KEYS): the group pass is agg_groups_wide_kernel over `w`
  u64 slots = 64;             // slots of the group table, and of every COUNT DISTINCT set: a power of two, at least twice the input's capacity
  u64 G = 1;                  // groups = output rows
  u64 accum_row_bytes = 0, refine_row_bytes = 0;   // what the accumulate pass / the refinement reads per input row
  u64 group_row_bytes = 0;                         // .. and the group pass: 4 per key column, 24 more per value key (its record)
  AggNode(NodeInfo& n, const DevTable& t) : nd(n), in(t) {}
};

struct Plan {
  Store* store = nullptr;
  EngineOptions opt;              // copied from the store at compile time (rdfgpu_plan_set_option changes this copy)
  std::vector<NodeInfo> nodes;
  std::vector<SourceInfo> sources;
  std::vector<u32> pool;          // IN-set ids of residual predicates (host copy)
  u32* pool_dev = nullptr;        // same, on device
  RegexProg* regex_dev = nullptr; // compiled REGEX patterns of the plan (device)
  unsigned char* str_consts_dev = nullptr;   // bytes of the plan's string constants (RDFGPU_EX_LIT_STR)
  rdfgpu_agg_value* mark_values_dev = nullptr;   // {boolean false, boolean true}: the value array of every LeftMark join's mark column (allocated by the first one that runs)
  std::vector<std::string> regex_strings; std::vector<rdfgpu_regex> regex_text;   // their texts (pattern, flags per entry)
  u32 root = 0;
  u64 run = 0;                    // counts the executions (a value array belongs to the one that wrote it)
  bool agg_columns = false;       // RDFGPU_PLAN_AGG_COLUMNS: aggregate values are u32 columns that flow into the operators above
  bool value_keys = false;        // RDFGPU_PLAN_VALUE_KEYS: an AggregateExec takes value columns as group columns, and up to RDFGPU_MAX_GROUP_KEYS of them
  ExecContext* ctx = nullptr;     // stream, events, counters (pooled per store)
  hipStream_t stream = nullptr;
  std::vector<BoundTable> tables;

  // per-execution state
  std::vector<void*> allocs;      // pool blocks owned by the current result / intermediates
  // The early result count (host_logic.hpp, early_count_eligible): execute returns at the band join's count point, in front of its emit pass — the
  // execution's TAIL, which then runs on `stream` while the host goes on.  tail_pending: the last execute left such a tail and no call has completed it
  // (complete()); the plan is then entered in store->tails.  The next execute does not wait for it — the stream orders its work behind the tail — and does not
  // hand the predecessor's blocks back to the pool, which another plan on another stream could be given: it retires them (`retired`; tail_lifetime.hpp),
  // takes from them what it needs itself and gives the rest back at its own first wait behind the tail.  retired_held: the predecessor's store generation.
  struct CountPoint { bool armed = false; const u64* n_out_dev = nullptr; u32 n_out = 0, overflow = 0; u64 out_cap = 0; };
  CountPoint count_point;         // set by Plan::band_blocks_and_emit when this execution's counters and total travel to the host in front of emit
  bool tail_pending = false;
  RetiredBlocks retired; std::shared_ptr<IndexGeneration> retired_held;
  void complete();                // waits for the stream once and finishes what execute left (elapsed time, retired memory, the registry entry); idempotent
  void tail_waited();             // a host wait that was stream-ordered behind the predecessor's tail has returned: what that tail kept alive goes
  u64* counters = nullptr;        // device u64 slots for operator output counts
  u32 counters_used = 0;
  u32 progs_used = 0;
  u32 arg_slots_used = 0;
  DevTable result; u64 result_rows = 0; bool executed = false;
  std::shared_ptr<IndexGeneration> held;   // the store generation the last execute ran against: zero-copy result slices point into it
  rdfgpu_metrics metrics{};
  bool timing = false;
  int timing_focus = -1;    // >= 0: only launches of this kernel class are bracketed with events (the longest class of the last fully timed execution)
  int last_top_kc = -1;
  u64 located_version = ~0ull;    // store version the cached scan ranges belong to
  bool allow_speculation = true, speculative = false;
  u64 scratch_hist[2] = {0, 0};           // intermediates of the last two completed executions (bounds what the pool keeps cached)
  bool priming = false, primed = false;   // the first execution over big bound tables is preceded by one over their first rows (Plan::prime)
  void prime();
  std::vector<SpecCheck> spec_checks;
  // The counter slots a band join of this execution leaves its measurements in -> NodeInfo::band (known_blocks != 0: counted on the host; multi_rows < 0: not fused, no such count)
  struct BandFeedback { NodeInfo* node; u32 blocks, slow_rows, run_stats; int multi_rows; bool slow_skipped, in_place; u64 known_blocks; };
  std::vector<BandFeedback> band_feedback;
  bool record_band_history();     // after the counters came back; true: a band join speculated wrongly (exact re-run)
  std::vector<PendingLaunch> pending;
  std::vector<DevTable> memo; std::vector<char> memo_valid;   // node results of the current execution
  ChainRequest* pending_chain = nullptr;                        // set while the base join of a fusable chain executes
  PendingOj pending_oj;
  void flush_pending_oj();
  void count_pending_oj();
  void count_ordered_join(OrderedJoinArgs& o);
  void probe_ordered_join(OrderedJoinArgs& o);
  u32 events_used = 0;
  KernelStat kstats[KC__N];
  // Arrow batch stream over a host copy of the result
  std::vector<std::vector<u32>> host_cols; bool host_valid = false; u64 cursor = 0;
  // aggregate values of an AggregateExec root (result_rows each), on the device and their host copy
  std::vector<rdfgpu_agg_value*> agg_out; std::vector<std::vector<rdfgpu_agg_value>> host_aggs;
  // .. and, per result column that is a value column, the value of every result row (gathered on the host; empty for an id column)
  std::vector<std::vector<rdfgpu_agg_value>> host_values;
  // the value array result column `col` indexes, of this execution (null / 0: an id column)
  const rdfgpu_agg_value* result_values(u32 col, u64* n) const;

  ~Plan();
  // the store's typed-value table with this execution's run-time error word attached (the last counter slot)
  TypedTable typed_table() const { TypedTable t = store->typed_table(); t.rt_error = reinterpret_cast<u32*>(counters + 255); return t; }
  void execute();
  void pushdown_filters(u32 node, const rdfgpu_pushdown_filter* filters, u32 n, u8* pushed);
  void set_dynamic_filters(u32 node, const rdfgpu_pushdown_filter* filters, u32 n);
  void derive_source(SourceInfo& src, const ScanInstructions& gspo);
  void upload_pool();
  void ensure_host_copy();

 private:
  void refresh_dynamic_sources(std::shared_lock<std::shared_mutex>& lock); void locate_sources();   // steps of execute
  DevTable exec_node(u32 idx);
  DevTable exec_sub_plan(u32 idx);
  DevTable exec_source(NodeInfo& nd);
  DevTable exec_projection(NodeInfo& nd);
  DevTable exec_closure(NodeInfo& nd);
  DevTable exec_union(NodeInfo& nd);
  DevTable exec_table(NodeInfo& nd);
  DevTable exec_filter(NodeInfo& nd);
  DevTable exec_join(NodeInfo& nd);
  DevTable exec_topk(NodeInfo& nd);
  DevTable exec_semi_join(NodeInfo& nd);
  DevTable exec_mark_join(NodeInfo& nd);
  DevTable exec_aggregate(NodeInfo& nd);   // its steps, in order (plan_aggregate.cpp):
  void agg_bind_inputs(AggNode& n); void agg_group_pass(AggNode& n); DevTable agg_outputs(AggNode& n); void agg_accumulate(AggNode& n); void agg_finish(AggNode& n);
  DevTable exec_extend(NodeInfo& nd);
  DevTable exec_sort(NodeInfo& nd);
  DevTable apply_filter(NodeInfo& nd, const DevTable& in);   // its routes:
  bool filter_string_verdicts(const NodeInfo& nd, const DevTable& in, FilterArgs& a); bool filter_run_copy(const NodeInfo& nd, const DevTable& in, FilterArgs& a, int shape);
  void filter_streamed(const NodeInfo& nd, const DevTable& in, FilterArgs& a, int shape); void filter_single_pass(const NodeInfo& nd, const DevTable& in, FilterArgs& a, int shape);
  // The inputs of a join as exec_join hands them to the join proper: lf / rf = the FilterExec above that input runs inside the probe; post = a build-side FilterExec kept as a conjunct of the join filter.
  struct JoinInputs { DevTable L, R; bool lf = false, rf = false; const NodeInfo* post = nullptr; };
  bool try_fused_chain(NodeInfo& nd, DevTable& fused); JoinInputs join_inputs(NodeInfo& nd);   // steps of exec_join
  DevTable exec_cross_join(const NodeInfo& nd, const DevTable& L, const DevTable& R);
  DevTable exec_generic_join(const NodeInfo& nd, const DevTable& L, const DevTable& R);
  bool keeps_pending_oj(const NodeInfo& nd, const DevTable& L, const DevTable& R, bool left_join, bool lf, bool rf) const;
  DevTable exec_lds_join(NodeInfo& nd, const DevTable& L, const DevTable& R, bool build_left, const NodeInfo* probe_filter, const NodeInfo* post_filter = nullptr);
  void lds_join_args(LdsJoin& j);
  JoinTable choose_join_table(LdsJoin& j);
  void size_wave_queue(LdsJoin& j);
  void run_join_kernel(LdsJoin& j, u64 stage_bytes, u64 out_bytes_per_row);
  DevTable run_speculative(LdsJoin& j, u64 first_guess, NodeInfo& size_node);
  bool run_ordered_join(LdsJoin& j, const NodeInfo& size_node, u64 spec_cap);
  DevTable run_exact(LdsJoin& j);
  void left_join_tail(const NodeInfo& nd, const DevTable& L, const DevTable& R, u32* const* out, u8* visited, u64* n_out_dev, u64 matched_total);
  bool plan_chain(NodeInfo& top, ChainRequest& req);
  struct DirectTable { bool dense = false; u32 kmin = 0, kn = 0; u32* direct = nullptr; u32* flags = nullptr; };
  DirectTable build_direct(const u32* key, u64 n, u64 max_range, bool cached);
  void build_dense_table(SliceTable* st, const u32* key, u64 n);
  bool apply_chain(const ChainRequest& req, LdsJoin& j);   // its steps:
  bool resolve_chain(const ChainRequest& req, LdsJoin& j); SliceTable::ValueColumn slice_value_column(const ChainLink& ln, const u32* col);
  bool chain_band_args(const ChainRequest& req, LdsJoin& j); u32 csr_max_group(SliceTable* tab, const LdsJoinArgs& a);
  void chain_range_index(LdsJoin& j, const ChainStage& s0); template <class F> void device_minmax_i64(long long (&got)[2], F&& launch);
  void prepare_partitions(const LdsJoinArgs& a, const DevTable& B, const DevTable& P, PartArgs& pa);
  void exec_band_join(LdsJoin& j);   // its steps, in order:
  bool take_pending_oj(BandJoin& bj); void band_probe_side(BandJoin& bj); void band_row_records(BandJoin& bj); void band_blocks_and_emit(BandJoin& bj);
  void band_slice_tables(BandJoin& bj); void band_entries(BandJoin& bj); SliceTable::BandEntries* band_layout(BandJoin& bj); void band_row_windows(BandJoin& bj);   // .. and its steps:
  bool band_row_operands(const BandJoin& bj, BandRowWinArgs& w); std::string band_row_win_key(const BandJoin& bj, const BandRowWinArgs& w); BandRowTiers band_row_tiers(const BandJoin& bj, const SliceTable::BandRowWindows& e, bool fresh);
  uint2* build_row_win(const BandJoin& bj, BandRowWinArgs& w, u32* declined); u64* build_pair_bits(const BandJoin& bj, const uint2* row_win); BandPairListArgs build_pair_list(const BandJoin& bj, const u64* bits, u32* total_out);
  void band_form_args(BandJoin& bj);
  bool choose_build_left(const NodeInfo& nd, const DevTable& L, const DevTable& R, bool left_join, bool lf, bool rf, bool lpost = false, bool rpost = false) const;
  void release_intermediates();
  template <class T> T* scratch(u64 n);
  u64* new_counter();
  const ExprProgram* upload_program(const ExprProgram& p);
  void bind_values(ExprProgram& p) const;   // a program's value loads (kExAggValue) get this execution's arrays
  // one host round trip: `bytes` of device memory copied to `host`, then the stream waited for
  void read_back(void* host, const void* dev, size_t bytes);
  template <class T> T read_back(const void* dev) { T v{}; read_back(&v, dev, sizeof v); return v; }
  // brackets one launch with HIP events when timing is on
  template <class F>
  void timed(int kc, u64 fixed_bytes, u64 rows_cap, const u64* rows_dev, u64 bytes_per_row,
             const u64* out_dev, u64 out_rows, u64 bytes_per_out, F&& launch);
  void resolve_timing();
};

Plan* plan_compile(Store* store, const rdfgpu_plan_desc* desc);

}  // namespace rdfgpu
