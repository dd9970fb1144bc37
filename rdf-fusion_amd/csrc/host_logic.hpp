// host_logic.hpp — scan planning on the host: predicate algebra, index choice, pruning levels.
// Mirrors lib/storage/src/memory/storage/{scan_instructions,quad_index}.rs and
// lib/storage/src/index/permutations.rs.  Never touches the device.
#pragma once
#include <vector>

#include "common.hpp"

namespace rdfgpu {

// MemIndexScanPredicate (scan_instructions.rs:157-166)
struct ScanPredicate {
  u32 kind = RDFGPU_PRED_NONE;
  std::vector<u32> ids;   // IN (sorted, unique)
  u32 from = 0, to = 0;   // BETWEEN (inclusive)
  u32 equal_to = 0;       // EQUAL_TO variable slot
};
// MemIndexScanInstruction (scan_instructions.rs:247-252)
struct ScanInstruction {
  u32 kind = RDFGPU_TRAVERSE;
  u32 var = 0;
  ScanPredicate pred;
};
// MemIndexScanInstructions (scan_instructions.rs:13): components + 4 instructions in that order
struct ScanInstructions {
  u32 components = RDFGPU_GSPO;
  ScanInstruction in[4];
};

ScanInstruction decode_instruction(const rdfgpu_scan_instruction& raw, const u32* pool, u32 n_pool);
// MemIndexScanInstructions::new (scan_instructions.rs:19-46): a variable bound twice becomes EqualTo
ScanInstructions make_gspo(const rdfgpu_scan_instruction raw[4], const u32* pool, u32 n_pool);
// ScanInstructions::reorder (scan_instructions.rs:137-152)
ScanInstructions reorder(const ScanInstructions& gspo, u32 components);
// compute_scan_score (quad_index.rs:100-130)
u64 scan_score(const ScanInstruction in[4]);
// choose_index (permutations.rs:81-96)
u32 choose_index(const ScanInstructions& gspo, u32 available_mask);
// try_and_with (scan_instructions.rs:170-210); false = not combinable
bool predicate_and(const ScanPredicate& a, const ScanPredicate& b, ScanPredicate* out);
// to_scan_predicate (predicate_pushdown.rs:120-157)
ScanPredicate pushdown_to_scan_predicate(u32 op, u32 value);

// What prune_relevant_row_groups (quad_index_data.rs:155-284) decides without looking at data:
// the leading levels that narrow the range, and which predicates the narrowing makes redundant.
struct PrunePlan {
  u32 n_levels = 0;
  u32 from[4] = {}, to[4] = {};
  u32 dropped_mask = 0;
};
PrunePlan plan_pruning(const ScanInstructions& ix);

// Band join reading a store slice's rows in place (plan_band.cpp, exec_band_join): may the rows' decoded windows be kept on the slice
// (SliceTable::BandRowWindows) instead of travelling by key every step?  Yes when the route is the in-place one with compact, packed
// records, the option is off, and every window operand is a column the ordered slice join below reaches through a stage (src >= 2)
// whose key column is that join's own key: the operand is then a function of the key alone, not of the batch.
struct BandRowOperandShape { u32 src = 0; bool stage_keyed_by_join_key = false; };   // src: ColRef::src of the ordered join's output column holding the operand
struct BandRowCacheShape {
  bool in_place = false, compact = false, pack16 = false, option_off = false;
  u32 n_win = 0; BandRowOperandShape y0[2], y1[2];
};
bool band_row_cache_eligible(const BandRowCacheShape& s);
// .. and may the pair test's verdicts be kept beside them (SliceTable::BandRowWindows::pair_bits: 512 bytes per block of the in-place layout)?  Yes when the
// rows' windows are kept (eligible, and accepted for this store), the pair test is the packed form whose `!=` is by entry index (BandArgs::neq_self, pack16),
// the option is off and the layout has at most `cap` blocks (RDFGPU_OPT_BAND_PAIR_CACHE_BLOCKS, inclusive; 0 = kBandPairCacheBlocks).
constexpr u64 kBandPairCacheBlocks = 1ull << 21;   // 1 GiB of verdicts: ten times what BSBM Q5 at 285 k products needs, small against the device's memory
struct BandPairCacheShape { bool row_windows = false, neq_self = false, pack16 = false, option_off = false; u64 n_blocks = 0, cap = 0; };
bool band_pair_cache_eligible(const BandPairCacheShape& s);
// .. and is a list of the surviving pairs kept beside the verdicts (SliceTable::BandRowWindows::pair_list: 2 bytes per set bit, in the order the emit pass writes the
// rows)?  A condition, not a measurement: yes when the step streams the cached verdicts, the option is off, the list is no larger than the bits it stands in for
// (2 * survivors <= 512 * n_blocks: at most 256 survivors per block on average) and the layout has fewer than kBandPairListBlocks blocks (4096 pairs per block:
// the list's 32-bit offsets cannot wrap).  survivors = 0 asks before the build, when only the layout is known.
constexpr u64 kBandPairListBlocks = 1ull << 20;
struct BandPairListShape { bool pair_cached = false, option_off = false; u64 survivors = 0, n_blocks = 0; };
bool band_pair_list_eligible(const BandPairListShape& s);
// .. and does a step that emits from the list count its blocks' rows from the per-row counts kept with it (SliceTable::BandRowWindows::pair_cnt: 64 bytes per
// block, band_mask_kernel's COUNTS form) instead of streaming the 512 bytes of bits?  A condition, not a measurement: yes when the step emits from the list (nothing
// else in it reads the bits), the option is off and the layout has at least `min_blocks` blocks (RDFGPU_OPT_BAND_PAIR_COUNT_BLOCKS, inclusive; 0 =
// kBandPairCountBlocks: 32 MiB of verdicts, the size of the L2 — below it the bits stay in cache from step to step and the pass is bound by its launch either way).
constexpr u64 kBandPairCountBlocks = 1ull << 16;
struct BandPairCountShape { bool has_list = false, option_off = false; u64 n_blocks = 0, min_blocks = 0; };
bool band_pair_count_eligible(const BandPairCountShape& s);

// The way one band-join step runs (band_join.hip's header has the table: what the mask pass and the emit pass do in each form, and what the step reads).  Decided
// here, once per step; Plan sets the kernel arguments from it and the launchers pick their kernels by it.
enum class BandForm : u32 { RECORDS, ROW_WINDOWS, VERDICTS, VERDICTS_LIST, COUNTS_LIST };
constexpr const char* band_form_name(BandForm f) {
  return f == BandForm::RECORDS ? "RECORDS" : f == BandForm::ROW_WINDOWS ? "ROW_WINDOWS" : f == BandForm::VERDICTS ? "VERDICTS" : f == BandForm::VERDICTS_LIST ? "VERDICTS_LIST" : "COUNTS_LIST";
}
// row_static: the step reads the slice's rows in place, through their cached windows and this execution's values by key (else: RECORDS, whatever the slice keeps).
// has_verdicts / has_list: the slice keeps the pair test's verdicts / their list and per-row counts for this chain, built under options like this plan's.  The list
// serves a step that streams the verdicts, has at most one row column (the list form of the emit pass knows one) and whose RDFGPU_OPT_NO_BAND_PAIR_LIST is off;
// such a step counts from the per-row counts when band_pair_count_eligible says so for the layout's n_blocks.
struct BandStepShape {
  bool row_static = false, has_verdicts = false, has_list = false, list_option_off = false, counts_option_off = false;
  u32 n_row_cols = 0; u64 n_blocks = 0, min_blocks = 0;
};
BandForm band_step_form(const BandStepShape& s);

// The probe pass of the ordered slice join below such a band join (ordered_join.hip): which of its two forms runs, and when.  A step of a row_static form takes from the
// table only the rows' values by key, and which output column that is the band join alone knows: so when the last execution's flags promise such a step — the write pass
// held back for the band join (held), that join read the slice's rows in place and no key had two table rows (in_place), the rows' windows were cached on the slice
// (row_cache), RDFGPU_OPT_NO_BAND_ROW_CACHE off — the ordered join launches nothing and OWES its probe.  It is asked twice with the same four flags: by the ordered join,
// with row_static = true (anything but FULL: the probe is owed), and where the debt is settled, with what the step turned out to be —
//   FULL      nothing is owed: the full pass (multimap, stage rows, packed records) ran where the ordered join ran, as on every other route;
//   LEAN      the band join took a row_static form: it runs the values-by-key pass (OjKeyValues) in the place of its records pass;
//   FULL_NOW  it did not, or something else takes the table: the full pass runs now, in front of the count pass.
enum class OjProbeForm : u32 { FULL, LEAN, FULL_NOW };
constexpr const char* oj_probe_form_name(OjProbeForm f) { return f == OjProbeForm::FULL ? "FULL" : f == OjProbeForm::LEAN ? "LEAN" : "FULL_NOW"; }
struct OjProbeShape { bool held = false, in_place = false, row_cache = false, option_off = false, row_static = false; };
OjProbeForm oj_probe_form(const OjProbeShape& s);

// May Plan::execute learn its result's row count in front of the band join's emit pass and return while that pass runs (Plan::band_blocks_and_emit, the count
// point)?  Nothing the host waits for is produced by emit: the total is the last entry of the blocks' scan, every counter the host reads afterwards is written by
// the passes before.  Yes only when the band join is the plan's root (is_root), its output is the plan's result and nothing is launched behind emit
// (result_is_output: no left-join tail, no held-back write pass), the step's form is one of the two list forms with the full-semantics pass skipped (a
// band_slow_kernel would run between the count and emit and may change the blocks' counts), the execution is speculative and not the priming run, kernel timing
// is off (the events of `timed` and elapsed_compute_ms need the finished stream) and RDFGPU_OPT_NO_EARLY_RESULT_COUNT is off.
// What runs behind the count point may READ only this execution's scratch, the slice's tables (eo, bdesc, pair_list, pair_list_off) and arguments passed by
// value, and WRITE only the result columns and its two counter words: never a caller-bound table (the caller may rebind or free it once execute has returned)
// and never a pinned staging slot of the context (the next execute fills those while the tail runs).  band_emit_list keeps to that; a form added to this
// function has to as well.
struct EarlyCountShape { bool is_root = false, result_is_output = false, skip_slow = false, speculative = false, priming = false, timing = false, option_off = false; BandForm form = BandForm::RECORDS; };
bool early_count_eligible(const EarlyCountShape& s);

}  // namespace rdfgpu
