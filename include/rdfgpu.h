/*
 * rdfgpu.h — C ABI of the MI355X-native BGP-scan + hash-join + FILTER path.
 *
 * This is the drop-in boundary for the one hot path of tobixdev/rdf-fusion that this
 * repository accelerates: triple-pattern scan over sorted u32 quad
 * indexes -> cross/hash join of binding tables -> SPARQL FILTER.  Everything in here is
 * plain C: pointers, sizes, PODs.  No C++/torch/Arrow-library types cross the boundary;
 * result batches leave through the Arrow C Data Interface structs declared below.
 *
 * Every entry point names the reference interface (file:line, relative to the
 * rdf-fusion tree) that it replaces.  INTEGRATION.md shows the Rust-side binding.
 *
 * Conventions
 *   - All functions return an rdfgpu_status (0 ok, >0 informational, <0 error) unless
 *     stated otherwise.  On error, rdfgpu_last_error() returns a thread-local message.
 *   - Object ids are u32.  Id 0 is the default graph AND the null / unbound marker,
 *     exactly as in the reference (lib/storage/src/memory/object_id.rs:21,80;
 *     quad_index_data.rs:438-440 stores 0 as an Arrow null).
 *   - The caller owns every input buffer; the library copies what it keeps.
 *   - A handle may be used from any thread, one in-flight call per handle.
 *   - There is NO CPU fallback: entry points that touch data fail with
 *     RDFGPU_ERR_NO_DEVICE when no gfx950 device is usable.  The host-logic entry
 *     points (section 5) never touch the device.
 */
#ifndef RDFGPU_H
#define RDFGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RDFGPU_ABI_VERSION 4u

/* ------------------------------------------------------------------------------------ */
/* 0. Status codes                                                                       */
/* ------------------------------------------------------------------------------------ */
typedef enum rdfgpu_status {
  RDFGPU_OK = 0,
  RDFGPU_END = 1,              /* rdfgpu_plan_next: stream exhausted                      */
  RDFGPU_ERR_INVALID = -1,     /* malformed argument / plan (DataFusionError::Plan)       */
  RDFGPU_ERR_DEVICE = -2,      /* HIP runtime error (DataFusionError::External)           */
  RDFGPU_ERR_UNSUPPORTED = -3, /* valid but not implemented on device                     */
  RDFGPU_ERR_OOM = -4,         /* device allocation failed                                */
  RDFGPU_ERR_NO_DEVICE = -5    /* no usable gfx950 device; there is no CPU fallback       */
} rdfgpu_status;

/* Thread-local text of the last error raised on the calling thread ("" if none). */
const char* rdfgpu_last_error(void);
uint32_t rdfgpu_abi_version(void);

/* ------------------------------------------------------------------------------------ */
/* 1. Arrow C Data Interface (verbatim ABI structs, https://arrow.apache.org/docs/format/CDataInterface.html) */
/* ------------------------------------------------------------------------------------ */
#ifndef ARROW_C_DATA_INTERFACE
#define ARROW_C_DATA_INTERFACE
struct ArrowSchema {
  const char* format;
  const char* name;
  const char* metadata;
  int64_t flags;
  int64_t n_children;
  struct ArrowSchema** children;
  struct ArrowSchema* dictionary;
  void (*release)(struct ArrowSchema*);
  void* private_data;
};
struct ArrowArray {
  int64_t length;
  int64_t null_count;
  int64_t offset;
  int64_t n_buffers;
  int64_t n_children;
  const void** buffers;
  struct ArrowArray** children;
  struct ArrowArray* dictionary;
  void (*release)(struct ArrowArray*);
  void* private_data;
};
#endif

/* ------------------------------------------------------------------------------------ */
/* 2. Store: three sorted u32 quad permutations + typed-value table, resident in HBM     */
/*    replaces MemQuadStorage (lib/storage/src/memory/storage/mem_storage.rs:22-102)     */
/*    and the MemIndexData layout (quad_index_data.rs:57-64)                             */
/* ------------------------------------------------------------------------------------ */
typedef struct rdfgpu_store rdfgpu_store;

typedef struct rdfgpu_config {
  int32_t device;        /* HIP device ordinal; -1 = current device                       */
  uint32_t batch_size;   /* rows per exported batch; 0 = 8192 (store.rs:102)              */
  uint32_t flags;        /* reserved, 0                                                   */
  uint32_t reserved;
} rdfgpu_config;

/* Index permutations, in the reference's listing order (mem_storage.rs:41-45).          */
enum { RDFGPU_GSPO = 0, RDFGPU_GPOS = 1, RDFGPU_GOSP = 2, RDFGPU_N_INDEXES = 3 };

/*
 * Device-side typed value of one object id: the FILTER side table.
 * Mirrors TypedValueEncodingField type ids (lib/encoding/src/typed_value/encoding.rs:248-268)
 * and the id -> typed value decode of object_id_mapping.rs:376-399.
 *   tag 0 null/invalid (parse failure => null, typed_value.rs:349-411)
 *   tag 1 named node, 2 blank node: lo = rank of the IRI / label in str order
 *   tag 3 string: lo = rank of the lexical value in str order; aux = language id
 *                 (0 = simple literal); flags bit0 = value is the empty string
 *   tag 4 boolean: lo = 0/1
 *   tag 5 float:   lo = IEEE-754 binary32 bits (zero-extended)
 *   tag 6 double:  lo = IEEE-754 binary64 bits
 *   tag 7 decimal: lo = index into the i128 side table (value * 10^18, decimal.rs:9-21)
 *   tag 8 int (i32, sign-extended), tag 9 integer (i64)
 *   tag 10 dateTime, 11 time, 12 date: a Timestamp (lib/model/src/xsd/date_time.rs:1599-1603; the host reads it with
 *              DateTime::timestamp() / Time::timestamp() / Date::timestamp()): lo = index into the i128 side table
 *              holding Timestamp.value (seconds on the XSD time line * 10^18, already shifted to UTC when a timezone
 *              is present), aux bit0 = timezone_offset.is_some().  Compared as PartialOrd for Timestamp does
 *              (date_time.rs:1617-1654): same presence => the values; otherwise the value without a timezone may lie
 *              14 h either way and the order must hold for both, else the comparison is an error.  Same kind only.
 *   tag 13 duration, 14 other literal: opaque on device (other literals: equal iff same datatype (aux) and same
 *              lexical value (lo), typed_value.rs:253-258); an operator that would need their value yields the
 *              SPARQL error value, i.e. the row is dropped by a FILTER — durations order by calendar arithmetic
 *              (duration.rs:271-310), not restated here.
 */
typedef struct rdfgpu_typed_value {
  int64_t lo;
  uint32_t aux;
  uint8_t tag;
  uint8_t flags;
  int16_t tz_minutes;  /* tags 10 / 11 / 12 with aux bit0 set: the TimezoneOffset in minutes (-840 .. 840); 0 otherwise.  Read by
                          RDFGPU_EX_YEAR .. RDFGPU_EX_MINUTES only (ordering and equality never look at it: two dateTimes are equal by
                          value and presence of a timezone, date_time.rs:1605-1613).  The field was `reserved` (0): a host that leaves
                          it 0 gets the parts of the UTC instant. */
} rdfgpu_typed_value; /* 16 bytes, one aligned dwordx4 gather per row */

enum {
  RDFGPU_TV_NULL = 0, RDFGPU_TV_NAMED_NODE = 1, RDFGPU_TV_BLANK_NODE = 2, RDFGPU_TV_STRING = 3,
  RDFGPU_TV_BOOLEAN = 4, RDFGPU_TV_FLOAT = 5, RDFGPU_TV_DOUBLE = 6, RDFGPU_TV_DECIMAL = 7,
  RDFGPU_TV_INT = 8, RDFGPU_TV_INTEGER = 9, RDFGPU_TV_DATE_TIME = 10, RDFGPU_TV_TIME = 11,
  RDFGPU_TV_DATE = 12, RDFGPU_TV_DURATION = 13, RDFGPU_TV_OTHER = 14
};
#define RDFGPU_TVF_EMPTY_STRING 1u
#define RDFGPU_TVF_NEEDS_HOST 0x80u   /* rdfgpu_ntriples_decoded only: the literal's value is left to the host's parser (see there) */

/* MemQuadStorage::new (mem_storage.rs:31-65): creates the store on `cfg->device`.  The first store a process creates also has the HIP
   runtime load every code object of this library (it would otherwise do so at the first launch from each translation unit: some
   tens of milliseconds that the first query would pay). */
int rdfgpu_store_create(const rdfgpu_config* cfg, rdfgpu_store** out);
void rdfgpu_store_destroy(rdfgpu_store* store);

/*
 * QuadStorage::extend (lib/extensions/src/storage/quad_storage.rs:35; mem_storage.rs:95-102;
 * IndexPermutations::insert permutations.rs:102-118): merges `n` encoded quads (host
 * buffers, ids assigned by the host dictionary) into all three permutations; duplicates
 * are ignored.  `*inserted` receives the number of quads that were new.
 */
int rdfgpu_store_extend(rdfgpu_store* store, const uint32_t* g, const uint32_t* s,
                        const uint32_t* p, const uint32_t* o, uint64_t n, uint64_t* inserted);
/* Same, with the four columns already resident in this device's HBM. */
int rdfgpu_store_extend_device(rdfgpu_store* store, const uint32_t* g, const uint32_t* s,
                               const uint32_t* p, const uint32_t* o, uint64_t n,
                               uint64_t* inserted);
/* QuadStorage::remove (quad_storage.rs:38; permutations.rs:120-128). */
int rdfgpu_store_remove(rdfgpu_store* store, const uint32_t* g, const uint32_t* s,
                        const uint32_t* p, const uint32_t* o, uint64_t n, uint64_t* removed);
/* QuadStorage::clear (quad_storage.rs:56). */
int rdfgpu_store_clear(rdfgpu_store* store);
/* QuadStorage::clear_graph (quad_storage.rs:59-62) and the quads of QuadStorage::drop_named_graph (:65-68): removes every quad
   whose graph is `graph` (0 = the default graph; the registry of named graphs is the host dictionary's). */
int rdfgpu_store_remove_graph(rdfgpu_store* store, uint32_t graph, uint64_t* removed);
/* QuadStorage::len (quad_storage.rs:71). */
int rdfgpu_store_len(const rdfgpu_store* store, uint64_t* out);
/* Cache control (no counterpart in the reference, whose HashJoinExec builds its table per query): forgets every join table
   cached on the store (direct-address / CSR / hash tables of predicate slices, decoded value tables, band-join entries) and
   bumps the store version — exactly what every extend / remove / clear does to the caches, without touching the quads.  The
   next execution of any plan locates its ranges and builds the tables it needs again, inside that execution.  Used to
   measure the "tables rebuilt in the step" figure (bench.py: config.cold_start.fused_rebuild). */
int rdfgpu_store_drop_tables(rdfgpu_store* store);

/*
 * Installs the id -> typed value table (MemObjectIdMapping::decode_array_to_typed_value,
 * object_id_mapping.rs:376-399).  values[i] describes object id i (values[0] is ignored:
 * id 0 is null).  `decimals` holds n_decimals little-endian i128 as (lo,hi) int64 pairs: the
 * values of xsd:decimal literals (tag 7) and the timestamps of tags 10..12.
 */
int rdfgpu_store_set_typed_values(rdfgpu_store* store, const rdfgpu_typed_value* values,
                                  uint64_t n_ids, const int64_t* decimals, uint64_t n_decimals);

/*
 * Installs the lexical forms of the string-valued object ids in HBM (the part of the reference's
 * MemObjectIdMapping dictionary that string builtins read: object_id_mapping.rs:48-59, 262-276).
 * The UTF-8 lexical form of object id i is heap[offsets[i] .. offsets[i + 1]); offsets has
 * n_ids + 1 entries; only ids whose typed value has tag RDFGPU_TV_STRING are ever read.
 * Needed by RDFGPU_EX_REGEX; a plan using it on a store without strings fails to compile.
 */
int rdfgpu_store_set_strings(rdfgpu_store* store, const uint64_t* offsets, uint64_t n_ids,
                             const uint8_t* heap, uint64_t heap_bytes);

/*
 * Test / debug access to a sorted permutation (MemIndexData, quad_index_data.rs:57-64):
 * copies up to `cap` rows of index `components` (RDFGPU_GSPO..) into four host columns,
 * in index order (e.g. g,p,o,s for GPOS).  `*n` receives the index length.
 */
int rdfgpu_store_read_index(const rdfgpu_store* store, uint32_t components, uint32_t* c0,
                            uint32_t* c1, uint32_t* c2, uint32_t* c3, uint64_t cap, uint64_t* n);

/* ------------------------------------------------------------------------------------ */
/* 3. Plan description: what DataFusion hands over for this path                         */
/* ------------------------------------------------------------------------------------ */

/*
 * One level of a quad pattern scan = MemIndexScanInstruction + MemIndexScanPredicate
 * (lib/storage/src/memory/storage/scan_instructions.rs:157-166, 247-252).
 */
enum { RDFGPU_TRAVERSE = 0, RDFGPU_SCAN = 1 };
enum { RDFGPU_PRED_NONE = 0, RDFGPU_PRED_FALSE = 1, RDFGPU_PRED_IN = 2, RDFGPU_PRED_BETWEEN = 3,
       RDFGPU_PRED_EQUAL_TO = 4 };

typedef struct rdfgpu_scan_instruction {
  uint8_t kind;      /* RDFGPU_TRAVERSE | RDFGPU_SCAN                                     */
  uint8_t pred;      /* RDFGPU_PRED_*                                                     */
  uint16_t reserved;
  uint32_t var;      /* SCAN: variable slot this level binds                              */
  uint32_t a;        /* IN: offset into the plan's u32 pool (sorted ascending, unique);
                        BETWEEN: from;  EQUAL_TO: variable slot it must equal             */
  uint32_t b;        /* IN: number of ids;  BETWEEN: to (inclusive)                       */
} rdfgpu_scan_instruction;

/*
 * Expression programs (postfix) = the PhysicalExpr trees DataFusion evaluates in
 * FilterExec / JoinFilter for this path, with the reference's UDF names
 * (lib/extensions/src/functions/builtin.rs:101-186).  Three value kinds live on the
 * evaluation stack: ID (u32 object id, 0 = null), TV (typed value, tag 0 = null/error),
 * BOOL (native nullable boolean).
 */
enum {
  RDFGPU_EX_COLUMN = 1,       /* -> ID      push input column `u` (join filters: left columns first, then right) */
  RDFGPU_EX_LIT_ID = 2,       /* -> ID      push object id literal `u`                                         */
  RDFGPU_EX_LIT_TV = 3,       /* -> TV      push typed literal (tag, lo, aux, flags), plan text "9:120"       */
  RDFGPU_EX_ENC_TV = 4,       /* ID -> TV   ENC_TV: with_typed_value_encoding.rs:71-79                         */
  RDFGPU_EX_GT = 5,           /* TV TV -> TV(boolean|null)  greater_than.rs:41-64                              */
  RDFGPU_EX_LT = 6,           /*            less_than.rs                                                        */
  RDFGPU_EX_GEQ = 7,
  RDFGPU_EX_LEQ = 8,
  RDFGPU_EX_EQ = 9,           /*            equal.rs (typed `=`)                                                */
  RDFGPU_EX_ADD = 10,         /* TV TV -> TV  add.rs:40-86                                                      */
  RDFGPU_EX_SUB = 11,         /*              sub.rs                                                            */
  RDFGPU_EX_EBV = 12,         /* TV -> BOOL   effective_boolean_value.rs:99-119                                 */
  RDFGPU_EX_ID_EQ = 13,       /* ID ID -> BOOL  native UInt32 `=`  (expression_simplifier.rs:162-257)          */
  RDFGPU_EX_ID_NEQ = 14,      /* ID ID -> BOOL  native `!=` (the `product != <object id>` FilterExec)          */
  RDFGPU_EX_AND = 15,         /* BOOL BOOL -> BOOL  SQL three-valued (expr_builder_context.rs:393-434)         */
  RDFGPU_EX_OR = 16,
  RDFGPU_EX_NOT = 17,         /* BOOL -> BOOL                                                                   */
  RDFGPU_EX_IS_COMPATIBLE = 18, /* ID ID -> BOOL  is_compatible.rs:97-136                                      */
  RDFGPU_EX_BOUND = 19,       /* ID -> BOOL   functional_form/bound.rs:21                                       */
  RDFGPU_EX_BOOL_AS_TV = 20,  /* BOOL -> TV   BOOLEAN_AS_TERM (expr_builder.rs:694-698)                        */
  RDFGPU_EX_LIT_BOOL = 21,    /* -> BOOL      literal true (u=1) / false (u=0) / null (u=2)                    */
  RDFGPU_EX_NEQ = 22,         /* TV TV -> TV  NOT(EQ) kept as one op for convenience                            */
  RDFGPU_EX_REGEX = 23,       /* TV -> TV(boolean|null)  REGEX(value, <constant pattern>[, <constant flags>]),
                                 scalar/strings/regex.rs:47-141; `u` indexes rdfgpu_plan_desc.regexes.  The value
                                 must come from ENC_TV of a column; simple / language strings match, anything else is
                                 the error value.  Syntax outside csrc/regex_compile.hpp's subset is RDFGPU_ERR_UNSUPPORTED at
                                 compile time; `\d \w \s \b` are compiled with their ASCII members and a row whose subject
                                 has a non-ASCII byte fails the execute with RDFGPU_ERR_UNSUPPORTED (the crate's Unicode tables
                                 are not restated).  Per-row patterns: RDFGPU_EX_REGEX_VAR.                        */
  RDFGPU_EX_CONTAINS = 24,    /* TV -> TV(boolean|null)  CONTAINS(value, <constant string>), scalar/strings/contains.rs;
                                 `u` indexes rdfgpu_plan_desc.regexes (the entry's pattern is the needle, taken literally; its
                                 flags are ignored), `lo` = language id of the constant (0 = simple literal).  Argument
                                 compatibility (string_literal.rs:80-95): the value must be a string and the constant must
                                 have no language or the value's, else the error value.                                  */
  RDFGPU_EX_STRSTARTS = 25,   /* same shape: STRSTARTS, scalar/strings/str_starts.rs                                     */
  RDFGPU_EX_STRENDS = 26,     /* same shape: STRENDS, scalar/strings/str_ends.rs                                         */
  RDFGPU_EX_LANG_IN = 27,     /* TV -> TV(boolean|null)  LANGMATCHES(LANG(value), <constant range>) — scalar/terms/lang.rs:45-58,
                                 scalar/strings/lang_matches.rs:52-69, as planned for BSBM explore Q8 (`EBV(LANGMATCHES(LANG(ENC_TV(text)),
                                 3:{value:EN,language:}))`, Q8 (Execution Plan).snap:18).  The range is resolved by the host against its
                                 (small) language dictionary: regexes[u].pattern holds ONE BYTE PER LANGUAGE ID (the `aux` numbering of
                                 string values; byte 0 = the empty tag, i.e. every literal without a language), 1 = the tag matches
                                 the range.  Named / blank nodes and null => error (lang.rs:50-52); a language id beyond the table
                                 => error.  At most 16384 language ids.                                                       */
  RDFGPU_EX_REGEX_VAR = 28,   /* TV TV -> TV(boolean|null)  REGEX(value, ?pattern[, <constant flags>]) with a PER-ROW pattern
                                 (regex.rs:59-76 compiles the pattern of every row; testsuite/oxigraph-tests/sparql/regex_variable.rq).
                                 The second operand is the pattern's typed value (ENC_TV of its column): a simple literal, else the
                                 error value.  The host announces the DISTINCT patterns that can occur: rdfgpu_plan_desc.regexes
                                 [u .. u + lo), each with its object id (rdfgpu_regex.pattern_id) and the constant flags; they are
                                 compiled at plan time and a row picks its program by the pattern's id.  A row whose pattern was not
                                 announced fails the execute (RDFGPU_ERR_UNSUPPORTED), it is never answered as "no match".            */
  /* ---- ABI 3: string-valued expressions.  A string value on the device is a VIEW: the lexical form of an object
     id in the store's string heap (rdfgpu_store_set_strings) or a constant of the plan, with a byte window (SUBSTR) and an ASCII
     case mapping (UCASE / LCASE) applied on the fly; nothing is materialised per row.  Views are consumed by REGEX / CONTAINS /
     STRSTARTS / STRENDS (whose operand may now be any string value, not only ENC_TV of a column), STRLEN, EBV and the
     comparisons (two strings of which at least one is a view compare byte-wise — `str` order — when their languages agree). */
  RDFGPU_EX_STR = 29,         /* ID -> TV(simple literal)  STR(term), scalar/terms/str.rs:42: over an object-id column the reference
                                 plans STR in the plain-term encoding (decide_input_encoding, expr_builder_context.rs:557-582:
                                 ObjectId is not supported, PlainTerm is the first that is), i.e. the lexical form AS WRITTEN of IRIs,
                                 blank nodes and every literal ("010"^^xsd:int -> "010", lib/functions/tests/snapshots/
                                 unary__STR(PLAIN_TERM).snap).  Null / an id without a lexical form in the heap => the error value. */
  RDFGPU_EX_LIT_STR = 30,     /* -> TV(string)  a string constant WITH its bytes: `u` indexes rdfgpu_plan_desc.regexes (the entry's
                                 pattern is the text), `lo` = its language id (0 = simple literal).  What a view is compared with:
                                 an RDFGPU_EX_LIT_TV string carries only its rank in the dictionary's order.                     */
  RDFGPU_EX_STRLEN = 31,      /* TV -> TV(integer)  STRLEN, scalar/strings/strlen.rs: characters (code points) of a simple or
                                 language-tagged string; anything else => error.                                                  */
  RDFGPU_EX_SUBSTR = 32,      /* TV TV [TV] -> TV(string)  SUBSTR(str, start[, length]), scalar/strings/sub_str.rs:83-121: `u` = 2 or 3
                                 operands; 1-based character positions; start < 1 or a negative length => error; a start beyond the
                                 end => ""; the language of the source is kept.  start / length must be xsd:int / xsd:integer values
                                 (a float / double / decimal argument fails the execute with RDFGPU_ERR_UNSUPPORTED).             */
  RDFGPU_EX_UCASE = 33,       /* TV -> TV(string)  UCASE, scalar/strings/ucase.rs (str::to_uppercase), language kept.  ASCII letters are
                                 mapped on the device; a string with a non-ASCII byte under a case mapping fails the execute with
                                 RDFGPU_ERR_UNSUPPORTED (Unicode case tables are not restated; never answered differently).      */
  RDFGPU_EX_LCASE = 34,       /* same: LCASE, scalar/strings/lcase.rs (str::to_lowercase)                                        */
  RDFGPU_EX_STRBEFORE = 35,   /* TV TV -> TV(string)  STRBEFORE(a, b), scalar/strings/str_before.rs: both string literals, b without a
                                 language or with a's (string_literal.rs:80-95, else error); the part of a before the first occurrence
                                 of b with a's language — a VIEW of a, nothing is copied; b does not occur => the simple literal "".    */
  RDFGPU_EX_STRAFTER = 36,    /* same: STRAFTER, scalar/strings/str_after.rs — the part of a behind the first occurrence of b             */
  /* ---- ABI 4 addendum: numeric expressions (new enum values only).  Every op is a pure per-row function of its operands and restates
     the reference bit for bit: exact integer / i128 arithmetic or single correctly rounded IEEE operations, nothing fused.  They run in
     the generic VM (FilterExec, join filters, and the input of SUM / AVG: RDFGPU_AGG_INPUT_EXPR). */
  RDFGPU_EX_MUL = 37,         /* TV TV -> TV  scalar/numeric/mul.rs:50-76: both numeric, else error; kinds promote as for ADD.  int: i32 checked,
                                 integer: i64 checked, float / double: one multiply; decimal: Decimal::checked_mul (lib/model/src/xsd/
                                 decimal.rs:93-125) — both values lose their trailing decimal zeros, the zeros must make up the 18 fraction
                                 digits (fewer => error: the product would need more precision, and so does 0 x 2.5 as written there), then a
                                 checked i128 product and a checked multiply by 10^(zeros - 18).                                     */
  RDFGPU_EX_DIV = 38,         /* TV TV -> TV  div.rs:51-80: int and integer pairs divide AS DECIMALS and yield a decimal; float / double: one
                                 divide (x / 0 is inf or NaN, not an error); decimal: Decimal::checked_div (decimal.rs:131-163) — the dividend
                                 is scaled by 10 while it stays inside i128, the divisor loses its trailing zeros, two truncating divisions; a
                                 zero divisor, MIN / -1 and a scale beyond 10^38 => error.  The same code finishes a decimal AVG.       */
  RDFGPU_EX_NEG = 39,         /* TV -> TV  unary_minus.rs (Numeric::neg, lib/model/src/xsd/numeric.rs:30-38): checked for int / integer / decimal
                                 (-MIN => error), the sign bit flipped for float / double; not numeric => error.  Plan text: MINUS.     */
  RDFGPU_EX_PLUS = 40,        /* TV -> TV  unary_plus.rs: a numeric value unchanged, anything else => error                                  */
  RDFGPU_EX_ABS = 41,         /* TV -> TV  abs.rs (Numeric::abs, numeric.rs:20-28): checked like NEG, the sign bit cleared for float / double   */
  RDFGPU_EX_ROUND = 42,       /* TV -> TV  round.rs:48-60: int / integer unchanged; float / double: Rust's `round`, half away from zero, the sign
                                 of a zero result kept; decimal: Decimal::checked_round (decimal.rs:211-222), whose negative branch is
                                 `-value % 10 > 5`: 2.5 rounds to 3 and -2.5 to -2, restated as written.                                */
  RDFGPU_EX_CEIL = 43,        /* TV -> TV  ceil.rs:48-60: like ROUND with `ceil` / Decimal::checked_ceil (decimal.rs:228-238); CEIL(-0.5) = -0.0  */
  RDFGPU_EX_FLOOR = 44,       /* TV -> TV  floor.rs: `floor` / Decimal::checked_floor (decimal.rs:244-254)                                  */
  RDFGPU_EX_CAST = 45,        /* TV -> TV  the XSD constructor functions, scalar/conversion/cast_{boolean,int,integer,decimal,float,double}.rs:
                                 48-62; `u` = the target tag: RDFGPU_TV_BOOLEAN, _INT, _INTEGER, _DECIMAL, _FLOAT or _DOUBLE (any other target:
                                 RDFGPU_ERR_UNSUPPORTED at compile — xsd:string and xsd:dateTime casts are not on the device).  A boolean casts
                                 to 0 / 1 of the target.  A numeric: to decimal from float / double by Decimal::try_from(Double) (decimal.rs:
                                 420-435: v * 10^18 in f64 must lie in [-2^127, 2^127], then a truncating, SATURATING conversion; a float is
                                 widened first); to integer / int through that decimal, a truncating division by 10^18 and a range check
                                 (decimal.rs:464-494, integer.rs:267-287, int.rs:238-267); to double / float as the comparisons promote
                                 (Decimal -> Double decimal.rs:445-462, Double -> Float `as f32`); to boolean `!= 0 && !NaN` (boolean.rs:51-84).
                                 Named / blank nodes, language-tagged strings, dateTime / date / time, durations, other literals and null =>
                                 error.  A SIMPLE LITERAL would have to be parsed: such a row fails the execute with RDFGPU_ERR_UNSUPPORTED
                                 (the lexical parsers are not restated; never answered differently).                                  */
  RDFGPU_EX_CAST_STRING = 46, /* ID -> TV(simple literal)  xsd:string(ENC_TV(id)), scalar/conversion/cast_string.rs:51-76.  Takes the object id,
                                 as STR does (ENC_TV keeps the id for strings only); the host lowers xsd:string(ENC_TV(col)) to it.  A named
                                 node, a simple literal, a language-tagged string and an other literal (`"12.5"^^bsbm:USD`) give their lexical
                                 form without a language: a view of the store's heap, nothing is copied.  A blank node, null, id 0 and an id
                                 beyond the table => error.  Booleans, numbers, dateTime / date / time and durations are FORMATTED by the
                                 reference (format_value / to_string): such a row fails the execute with RDFGPU_ERR_UNSUPPORTED.  Needs
                                 rdfgpu_store_set_strings; a value column or a computed typed value is a kind error.                      */
  RDFGPU_EX_CAST_LEX = 47,    /* TV -> TV  RDFGPU_EX_CAST (same `u`, same targets) that PARSES a simple literal — a dictionary string, a window,
                                 a case-mapped view or an RDFGPU_EX_LIT_STR constant, without a language — as the reference's FromStr impls do:
                                 boolean exactly true / 1 / false / 0 (boolean.rs:108-115); int / integer i32::from_str / i64::from_str (an
                                 optional sign, digits, checked range); decimal Decimal::from_str (decimal.rs:496-568); float / double
                                 f32::from_str / f64::from_str: Rust's grammar (no whitespace; inf / infinity / nan in any case), correctly
                                 rounded with ONE rounding to the target — Clinger's exact case, else Eisel-Lemire over the first 19
                                 significant digits (w and w + 1 must agree when digits were dropped).  What does not parse => error.  A
                                 literal Eisel-Lemire cannot decide (a half-way neighbourhood) and a signed NaN fail the execute with
                                 RDFGPU_ERR_UNSUPPORTED; never answered differently.  Every other operand: exactly RDFGPU_EX_CAST.        */
  /* ---- ABI 4 addendum: the parts of an xsd:dateTime (new enum values only) — what the Wind Farm plans group their time series by
     (bench/tests/plans/snapshots/..Wind Farm - GroupedProduction1..4: `YEAR(tv) as year, MONTH(tv) as month, DAY(tv), HOURS(tv),
     MUL(9:10, FLOOR(DIV(MINUTES(tv), 10.0)))`).  All six are unary, TV -> TV, and restate scalar/dates_and_times/{year,month,day,hours,
     minutes,seconds}.rs over Timestamp::{year_month_day, hour, minute, second} (lib/model/src/xsd/date_time.rs:1731-1839) statement by
     statement (csrc/date_parts.hpp).  Only an RDFGPU_TV_DATE_TIME operand yields a value; every other kind — date, time, null, a number
     — is the error value (`ThinError::expected()`).  t = value / 10^18 truncated toward zero, plus tz_minutes * 60 (no timezone: 0, i.e.
     UTC); days = div_euclid(t, 86400) + 366 and the reference's 400 / 100 / 4 / 1-year descent; hour = rem_euclid(t, 86400) / 3600;
     minute = rem_euclid(t, 3600) / 60.  The offset comes from rdfgpu_typed_value.tz_minutes (ENC_TV) or bits 16..31 of a literal's `u`.
     Allowed wherever MUL is: FILTER, join filters, SUM / AVG / MIN / MAX inputs, RDFGPU_NODE_EXTEND programs; a predicate with one runs in
     the generic VM.  TZ / TIMEZONE and the parts of xsd:date / xsd:time are not on the device. */
  RDFGPU_EX_YEAR = 48,        /* TV(dateTime) -> TV(integer)  year.rs; years before 1 are 0, -1, .. as year_month_day counts them      */
  RDFGPU_EX_MONTH = 49,       /* TV(dateTime) -> TV(integer)  month.rs: 1..12                                                          */
  RDFGPU_EX_DAY = 50,         /* TV(dateTime) -> TV(integer)  day.rs: 1..31                                                            */
  RDFGPU_EX_HOURS = 51,       /* TV(dateTime) -> TV(integer)  hours.rs: 0..23                                                          */
  RDFGPU_EX_MINUTES = 52,     /* TV(dateTime) -> TV(integer)  minutes.rs: 0..59                                                        */
  RDFGPU_EX_SECONDS = 53,     /* TV(dateTime) -> TV(decimal)  seconds.rs: rem_euclid(value, 60 * 10^18) on the scaled i128, in [0, 60);
                                 no offset is applied (offsets are whole minutes)                                                      */
  /* ---- ABI 4 addendum: functional forms (SPARQL 1.1 §17.4.1) and term tests (§17.4.2), new enum values only.  Evaluation is EAGER, as in
     the reference (dispatch_ternary_typed_value computes all three argument arrays of IF; DataFusion's `coalesce` gets evaluated arrays):
     every operand is computed for every row and errors are values.  A RUN-TIME REFUSAL of the device is not a value: an operand that
     raises one (a CAST of a simple literal, a CAST_LEX the device cannot decide, ..) fails the execute with RDFGPU_ERR_UNSUPPORTED even
     when it sits in the branch IF does not choose or behind the operand COALESCE returns — louder than the reference, never a different
     answer.  Allowed wherever MUL is: FILTER, the filter of every join kind, SUM / AVG / MIN / MAX inputs, RDFGPU_NODE_EXTEND programs,
     HAVING over value columns; a predicate with one runs in the generic VM.
     IN / NOT IN need no op: expression_rewriter.rs:302-322 (rewrite_in) is BOOL_AS_TV(OR(EBV(EQ(lhs, e_1)), EBV(EQ(lhs, e_2)), ..)),
     BOOL_AS_TV(LIT_BOOL false) for an empty list, and NOT IN is BOOL_AS_TV(NOT(EBV(IN(..)))).  sameTerm over ids stays ID_EQ.
     LANG(v) = "tag" is an RDFGPU_EX_LANG_IN whose table is 1 exactly for the language ids with that tag (a literal without a language
     gives "": id 0; IRIs, blank nodes and null the error value, lang.rs:49-55).  LANG and DATATYPE as VALUES are not on the device.
     The value 54 is not assigned: a description that holds it is refused as an unknown op, as before. */
  RDFGPU_EX_IF = 55,          /* TV TV TV -> TV  functional_form/sparql_if.rs:38-61: operands test, then, else.  The test must be a typed
                                 value of tag RDFGPU_TV_BOOLEAN (Boolean::try_from, lib/model/src/xsd/boolean.rs:93-102 — NOT the EBV):
                                 the null value, a number, a string, an IRI => the error value.  Otherwise the chosen branch comes out
                                 unchanged, also when the other branch is the error value.  EBV semantics: BOOL_AS_TV(EBV(test)).        */
  RDFGPU_EX_COALESCE = 56,    /* u x TV -> TV  or  u x ID -> ID   DataFusion's `coalesce` (lib/functions/src/registry.rs:264-270): `u` = the
                                 number of operands, 1 .. 8, all of one kind (mixed kinds, u = 0 or u > 8: RDFGPU_ERR_INVALID).  TV form: the
                                 first operand that is not the error value (tag RDFGPU_TV_NULL), else the error value.  ID form: the first
                                 non-zero object id, else 0.  A value column is read through ENC_TV (unwrapped it is refused: its entries
                                 are not object ids).                                                                                    */
  RDFGPU_EX_IS_IRI = 57,      /* TV -> TV(boolean|null)  scalar/terms/is_iri.rs: tag NAMED_NODE; the null value => error (all four)       */
  RDFGPU_EX_IS_BLANK = 58,    /* TV -> TV(boolean|null)  is_blank.rs: tag BLANK_NODE                                                      */
  RDFGPU_EX_IS_LITERAL = 59,  /* TV -> TV(boolean|null)  is_literal.rs: every non-null tag but NAMED_NODE / BLANK_NODE; a computed string
                                 (a view) is a literal                                                                                   */
  RDFGPU_EX_IS_NUMERIC = 60,  /* TV -> TV(boolean|null)  is_numeric.rs: INT, INTEGER, DECIMAL, FLOAT or DOUBLE                            */
  RDFGPU_EX__COUNT
};

typedef struct rdfgpu_expr_node {
  uint8_t op;       /* RDFGPU_EX_*                                                        */
  uint8_t tag;      /* LIT_TV: typed value tag                                            */
  uint8_t flags;    /* LIT_TV: rdfgpu_typed_value.flags                                   */
  uint8_t reserved;
  uint32_t u;       /* COLUMN: column index; LIT_ID: id; LIT_TV: aux; LIT_BOOL: 0/1/2     */
                    /* LIT_TV timestamps: bit 0 = has a timezone, bits 16..31 = the offset in minutes as int16 (rdfgpu_typed_value.tz_minutes;
                       read by the date parts only, every comparison masks to bit 0) */
  int64_t lo;       /* LIT_TV payload (decimal / dateTime / time / date literals: low 64 bits of the i128) */
  int64_t hi;       /* LIT_TV decimal / timestamp literal: high 64 bits; timestamps: u bit0 = has timezone */
} rdfgpu_expr_node; /* 24 bytes */

/* Physical operators of the path, named as in the reference's execution plans
   (bench/tests/plans/snapshots/..Q5 (Execution Plan).snap:10-30). */
enum {
  RDFGPU_NODE_DATA_SOURCE = 1, /* DataSourceExec(MemQuadPatternDataSource), pattern_data_source.rs:21-58  */
  RDFGPU_NODE_FILTER = 2,      /* FilterExec: keep rows whose predicate is true; optional projection       */
  RDFGPU_NODE_HASH_JOIN = 3,   /* HashJoinExec(CollectLeft), inner | left | left semi | left anti, NullEqualsNothing, filter, projection */
  RDFGPU_NODE_CROSS_JOIN = 4,  /* CrossJoinExec                                                            */
  RDFGPU_NODE_NESTED_LOOP_JOIN = 5, /* NestedLoopJoinExec: inner | left | left semi | left anti, no equi keys */
  RDFGPU_NODE_PROJECTION = 6,  /* ProjectionExec of plain columns                                          */
  RDFGPU_NODE_TABLE = 7,       /* bindings supplied by the caller (device columns), e.g. all-gathered rows */
  RDFGPU_NODE_TOPK = 8,        /* The operators directly above the path in the reference's explore plans (SURVEY §8f-3,
                                  ..Q5 (Execution Plan).snap:5-9): AggregateExec(gby = sort keys, first_value) = DISTINCT,
                                  then SortExec TopK(fetch = k), optionally per group (a batch of queries in one tree).
                                  left = input; n_keys sort keys (<= 4), all ascending, NULLS FIRST: left_keys[i] = column,
                                  right_keys[i] = RDFGPU_SORT_BY_ID (the UInt32 id itself, `product@1 ASC`),
                                  RDFGPU_SORT_BY_TERM (ENC_SORT of the term: defined here for columns of one kind among
                                  strings / IRIs / blank nodes, whose typed value carries the rank) or
                                  RDFGPU_SORT_BY_DOUBLE; table_cols = k; table_slot = 1 + group column (0 = one group).
                                  Rows equal on (group, keys) collapse to one.  The reference's AggregateExec groups by the
                                  sort expressions AND the raw columns (`gby=[ENC_SORT(..), product, productLabel]`), so two
                                  terms that sort alike stay two rows: every output column must be the group column or a key
                                  BY_ID — the host appends the remaining gby columns as trailing BY_ID keys (which also makes
                                  the order among ties of the declared ORDER BY deterministic).                          */
  RDFGPU_NODE_UNION = 9,       /* UnionExec: the rows of `left` followed by the rows of `right` (bag union; both inputs have
                                  the same columns) — SPARQL UNION as planned in BSBM Explore - Q4 / Q11 (Execution Plan).snap;
                                  optional projection */
  RDFGPU_NODE_CLOSURE = 10,    /* KleenePlusClosureExec (lib/physical/src/paths/kleene_plus/physical.rs:94-157, 246-384): `left` yields
                                  the inner paths (graph, start, end) — graph 0 = default graph; the output is the SET of all paths
                                  of one or more inner paths chained end-to-start: within one graph (join_type = 0), or continuing
                                  through the inner paths of any graph while keeping the first path's graph (join_type = 1 =
                                  allow_cross_graph_paths).  A null start / end is an execution error, as in the reference. */
  /* ABI 4 addendum (backward compatible: new enum values and functions, no struct changed) */
  RDFGPU_NODE_AGGREGATE = 11,  /* AggregateExec(mode=Single) over object-id group columns — what the BSBM Business Intelligence plans put
                                  on top of their join trees (bench/tests/plans/snapshots/..Business Intelligence - Q1..Q8 (Execution
                                  Plan).snap).  Encoding: left = input; n_keys (0..RDFGPU_MAX_KEYS) group columns in left_keys[];
                                  table_cols = number of aggregates (0..RDFGPU_MAX_AGGREGATES); table_slot = offset into the u32 pool of
                                  table_cols pairs (RDFGPU_AGG_*, input); n_proj must be RDFGPU_NO_PROJECTION.  The input is a column of
                                  `left`, or — SUM, AVG, MIN and MAX only — RDFGPU_AGG_INPUT_EXPR | the pool offset of two words (expr_off, expr_len)
                                  naming a program in `exprs` over the input's columns that leaves a typed value (`SUM(?price * ?qty)`);
                                  such an input of COUNT / COUNT_DISTINCT, and a program with REGEX / CONTAINS / STRSTARTS / STRENDS /
                                  LANG_IN in it, is RDFGPU_ERR_UNSUPPORTED at compile.  Output columns: the
                                  keys in order, then the aggregates.  Two rows are one group when their key ids are equal; id 0
                                  (unbound) is a key value like any other (SQL GROUP BY puts NULLs in a group of their own).  With 0 keys
                                  there is exactly one output row, even over an empty input; with keys an empty input gives no row.  Row
                                  order unspecified.  A node without aggregates (a DISTINCT over its keys, BI Q4's `AggregateExec:
                                  gby=[feature], aggr=[]`) outputs object ids only and may appear anywhere in a plan; a node WITH
                                  aggregates must be the plan's root (their values are not object ids and cannot flow into another
                                  operator), anywhere else it is RDFGPU_ERR_UNSUPPORTED at compile.  An input of 2^32 rows or more fails
                                  the execute with RDFGPU_ERR_UNSUPPORTED.  The aggregate values leave through rdfgpu_plan_agg_*;
                                  rdfgpu_plan_result_info / _device / _fetch report the key columns only.
                                  With RDFGPU_PLAN_AGG_COLUMNS in rdfgpu_plan_desc.flags (opt-in per plan; without it all of the above holds
                                  unchanged) a node with aggregates may sit ANYWHERE, the root included: its output has n_keys + table_cols
                                  u32 columns, the keys and then one VALUE COLUMN per aggregate.  Row g of the node carries g + 1 in a value
                                  column, or 0 where the aggregate is the error value: an error aggregate is an unbound binding everywhere
                                  (BOUND is false, a LEFT join's padding looks the same, rdfgpu_plan_next exports a null).  The 24-byte
                                  values stay in one device array per aggregate, which the entries index (rdfgpu_plan_result_values).
                                  Value columns are typed at compile and carried through projections, filters and joins.  They may be
                                  read by ENC_TV and BOUND in FILTER predicates and join filters (ENC_TV yields the aggregate's value:
                                  the BI plans' HAVING, `FilterExec: EBV(GT(INT64_AS_TERM(count@1), 9:0))`, where INT64_AS_TERM is the
                                  identity: counts are xsd:integer values already), projected, carried as payload of HASH_JOIN /
                                  CROSS_JOIN / NESTED_LOOP_JOIN of every join type, consumed by two parents, and be the input of COUNT, SUM,
                                  AVG, MIN and MAX (plain or inside an input expression) of a further AggregateExec.  Equal values have different
                                  indexes, so whatever would compare the entries as ids is RDFGPU_ERR_UNSUPPORTED at compile (the text names
                                  node and column): a join key, a group column, a COUNT_DISTINCT input, any TopK key / group / output, a
                                  CLOSURE or UNION input; and so is rdfgpu_plan_decode_terms of a value column.  A value column under
                                  ID_EQ / ID_NEQ / IS_COMPATIBLE / STR is RDFGPU_ERR_INVALID, like every operand of the wrong kind.  A
                                  predicate that reads a value column runs in the generic VM.
                                  With RDFGPU_PLAN_VALUE_KEYS as well (opt-in per plan, valid only together with RDFGPU_PLAN_AGG_COLUMNS; without
                                  it every refusal and every launch above is unchanged) — the tail of the Wind Farm GroupedProduction plans,
                                  `AggregateExec: gby=[site_label, wtur_label, ENC_PT(year), ENC_PT(month), ENC_PT(day), ENC_PT(hour),
                                  ENC_PT(minute_10)], aggr=[AVG(val)]` —: n_keys may be up to RDFGPU_MAX_GROUP_KEYS, keys 0..3 in left_keys[], keys
                                  4..7 in right_keys[] (which an aggregate has no other use for), and any key may be an object-id column or a
                                  value column (an aggregate's or a computed one).  Group equality: id keys compare as ids.  A value key
                                  compares by the plain term its value stands for (the reference groups by ENC_PT of the column): the tag;
                                  `lo`; `hi` for RDFGPU_TV_DECIMAL only (ignored otherwise).  All NaNs of one tag are equal; +0.0 and -0.0
                                  are different terms; INTEGER 5, INT 5 and DECIMAL 5 are different terms; an entry of 0 and a record with tag
                                  RDFGPU_TV_NULL are both "unbound", which is one key value like id 0.  Output: the key columns first, in
                                  order; a value key stays a value column WITH ITS INPUT'S ORIGIN — the entry of the group's representative
                                  row, which indexes the same value array — so FILTERs, SortExec by value, EXTEND and
                                  rdfgpu_plan_result_values above the node work unchanged; then the aggregates' value columns, as above.
                                  The other roles of a value column stay refused, with the texts above: join key, COUNT_DISTINCT input, TopK
                                  key / group / output, CLOSURE / UNION input.  Joins, TopK and SortExec keep RDFGPU_MAX_KEYS keys.  A node
                                  with a value key or more than 4 keys runs a group pass of its own (agg_groups_wide_kernel in
                                  rdfgpu_plan_kernel_stats); a node with at most 4 id keys launches exactly what it launches without the flag.  */
  RDFGPU_NODE_EXTEND = 12,     /* ProjectionExec whose `expr=[..]` holds expressions (SPARQL Extend: BIND, `SELECT (expr AS ?x)`) — what the
                                  BSBM Business Intelligence plans put directly above their aggregates (..Business Intelligence - Q3 / Q4 /
                                  Q8 (Execution Plan).snap: `DIV(xsd:float(monthCount@1), monthBeforeCount@2) as ratio`).  Encoding: left =
                                  input, right = -1; proj_off / n_proj = the input columns kept, in order (RDFGPU_NO_PROJECTION keeps all);
                                  table_cols = number k of computed columns (1..RDFGPU_MAX_AGGREGATES); table_slot = offset into the u32
                                  pool of k pairs (expr_off, expr_len), each naming a program in `exprs`.  Output columns: the kept
                                  columns, then the k computed columns, at most RDFGPU_MAX_COLUMNS together.
                                  The node is accepted only in a plan compiled with RDFGPU_PLAN_AGG_COLUMNS; without the flag it is
                                  RDFGPU_ERR_UNSUPPORTED at compile (its outputs are not object ids).
                                  A program ranges over ALL input columns, not only the kept ones.  It may read id columns through ENC_TV /
                                  BOUND, and value columns of aggregates and of other EXTEND nodes below.  It must leave a typed value: a
                                  program that leaves a boolean verdict is RDFGPU_ERR_INVALID (wrap it in BOOLEAN_AS_TERM), one that leaves
                                  an id is RDFGPU_ERR_INVALID (a plain column is a projection), and one with REGEX / CONTAINS / STRSTARTS /
                                  STRENDS / LANG_IN or a string-view op (STR, LIT_STR, STRLEN, SUBSTR, UCASE, LCASE, STRBEFORE, STRAFTER)
                                  in it is RDFGPU_ERR_UNSUPPORTED — the rule of an aggregate's input expression.
                                  Row r of the node carries r + 1 in a computed column; its value is entry r of that column's
                                  rdfgpu_agg_value array.  A row whose program yields the error value (DIV by an integer zero, an overflow,
                                  an unbound or non-numeric operand) carries 0 and tag RDFGPU_TV_NULL: an unbound binding everywhere,
                                  exactly like an error aggregate.  The 24-byte record carries INT, INTEGER, DECIMAL, FLOAT, DOUBLE and
                                  BOOLEAN values, the payload laid out as a value load reads it back: lo, and (lo, hi) for a decimal.  A
                                  row whose value is of any other kind (string, IRI, blank node, dateTime, date, time, duration) — the
                                  record has no room for its `aux` — fails the execute with RDFGPU_ERR_UNSUPPORTED; such a row is never
                                  answered differently, and the plan stays usable afterwards.  An input of 2^32 - 1 rows or more fails
                                  the execute with RDFGPU_ERR_UNSUPPORTED.
                                  A computed column is a value column everywhere above the node: everything the AGGREGATE entry says of
                                  carriage (projections, filters, join payload of every join type, two parents, input of COUNT / SUM / AVG)
                                  and of refusals (join key, group column, COUNT_DISTINCT input, TopK key / group / output, CLOSURE / UNION
                                  input, rdfgpu_plan_decode_terms; the sharded path exchanges object ids only) applies, the texts naming
                                  the node and the expression.  rdfgpu_plan_result_values / _fetch / rdfgpu_plan_next work unchanged.   */
  RDFGPU_NODE_SORT = 13        /* SortExec: ORDER BY over object-id and value columns, ascending or descending per key, with an optional
                                  fetch — the operator that ends the BSBM Business Intelligence plans (..Business Intelligence - Q3
                                  (Execution Plan).snap:6: `SortExec: TopK(fetch=10), expr=[ENC_SORT(DIV(xsd:float(monthCount@1),
                                  monthBeforeCount@2)) DESC, ENC_SORT(ENC_PT(product@0)) ASC]`; Q1: `ENC_SORT(reviewCount@1) DESC`).
                                  Encoding: left = input, right = -1; n_keys = 1..RDFGPU_MAX_KEYS; left_keys[i] = the column of key i;
                                  right_keys[i] = how | RDFGPU_SORT_DESC (without the flag: ascending), `how` being RDFGPU_SORT_BY_ID,
                                  _BY_TERM or _BY_DOUBLE over an object-id column — the keys RDFGPU_NODE_TOPK defines, BY_TERM's refusal of
                                  a column of mixed kinds included (it fails the execute) — or RDFGPU_SORT_BY_VALUE over a value column;
                                  table_cols = the fetch (0: none, every row); proj_off / n_proj = the output columns.
                                  Rows: no de-duplication; the output is the input's rows, the first `fetch` of them in the order below.
                                  Order: lexicographic over the keys; rows equal on every key come out in ascending input row order (the
                                  reference leaves that order open; it is defined here so that results are reproducible).  DESC reverses
                                  the whole key of that key (NULLs, which come first ascending, come last), never the final tie-break.
                                  Columns: a value column of the input is a value column of the output, its origin carried like a
                                  projection's and its entries unchanged (only the u32 entries of the columns are permuted, the 24-byte
                                  values stay where they are): rdfgpu_plan_result_values / _fetch / rdfgpu_plan_next work unchanged.
                                  Placement: anywhere a projection may sit.  The order is promised at the root and under plain PROJECTION
                                  and EXTEND nodes above it; any other operator above may reorder.
                                  RDFGPU_ERR_UNSUPPORTED / _INVALID at compile: n_keys outside 1..RDFGPU_MAX_KEYS; BY_VALUE over an
                                  object-id column, an id form over a value column; BY_VALUE in a plan without RDFGPU_PLAN_AGG_COLUMNS (there
                                  are no value columns without it); a key list whose record (below) exceeds 8 words.  The sharded path
                                  exchanges rows between ranks and keeps no order: its stages refuse the node.  An input of 2^32 - 1 rows
                                  or more fails the execute.  RDFGPU_NODE_TOPK (DISTINCT, ascending, per group) is unchanged.        */
};
/*
 * Aggregate functions of RDFGPU_NODE_AGGREGATE (ABI 4 addendum).  The reference plans SPARQL aggregates in
 * lib/logical/src/expr_builder.rs:700-760 onto its own accumulators (lib/functions/src/aggregates/); the input of SUM / AVG is
 * ENC_TV of an object-id column, or an expression program (RDFGPU_AGG_INPUT_EXPR) whose error value counts as "not numeric", exactly
 * as an unbound id does.  (A cast FROM A STRING is not on the device: BSBM BI's `AVG(xsd:float(xsd:string(?price)))` stays on the host.)
 *   COUNT_STAR      rows of the group, as xsd:integer: DataFusion count(*) then INT64_AS_TERM (graph_pattern_rewriter.rs:311-313)
 *   COUNT           rows whose input id is not 0 (unbound), xsd:integer
 *   COUNT_DISTINCT  distinct non-zero ids of the input column in the group, xsd:integer (expr_builder.rs:724-733: count_distinct over
 *                   the ids; two ids are two terms)
 *   SUM             aggregates/sum.rs:34-73.  The sum starts as xsd:integer 0.  A value that is not numeric, unbound ones included, is
 *                   skipped (sum.rs:52 has no `else`; the reference's behaviour, not the SPARQL spec's).  Kinds promote as in
 *                   NumericPair::with_casts_from (lib/model/src/xsd/numeric.rs:127-): int / integer, then decimal, then float, then
 *                   double; the result kind is the widest kind seen in the group.  An integer result outside i64 is the error value,
 *                   and so is a decimal result outside the i128 x 10^-18 range.
 *   AVG             aggregates/avg.rs:43-134.  The sum starts as xsd:DECIMAL 0, so an all-integer group averages to a decimal:
 *                   AVG(1, 2) = 1.5.  Every row of the group is counted (avg.rs:59); one value that is not numeric or unbound makes
 *                   the result the error value (avg.rs:63-78).  A count of 0 gives xsd:integer 0 (only the zero-key group over an empty
 *                   input has one).  Decimal results are Decimal::checked_div(sum, count) (lib/model/src/xsd/decimal.rs:131-162),
 *                   restated bit-exactly: the dividend is scaled by 10 while it stays inside i128, the divisor's trailing zeros are
 *                   stripped, two truncating divisions, and a scale beyond 10^38 is the error value.  Float results divide by
 *                   f32(count), double results by f64(count).
 *   MIN / MAX       aggregates/min.rs:42-53, max.rs:43-54.  Accepted only in a plan compiled with RDFGPU_PLAN_AGG_COLUMNS (like
 *                   RDFGPU_NODE_EXTEND and RDFGPU_SORT_BY_VALUE; without the flag they are RDFGPU_ERR_UNSUPPORTED at compile, as they
 *                   always were).  The input is SUM's: an object-id column read through ENC_TV, a value column of an aggregate or
 *                   EXTEND below, or an expression program (RDFGPU_AGG_INPUT_EXPR, the same refusals).  The reference's accumulator
 *                   keeps its first row's value — its error state and its NaN included — and replaces it only by a value that is
 *                   strictly less (greater), so its answer depends on row order.  The device's answer is fixed, independent of row
 *                   order, and always one the reference gives for SOME order of the same rows.  For one group:
 *                     1. no rows (the zero-key node over an empty input): the error value, RDFGPU_TV_NULL (`min: ThinError::expected()`);
 *                     2. any error value in the group — an unbound id, a value-column entry of 0, a program that yields the error
 *                        value — : the error value (the reference's answer when such a row comes first; AVG's rule here);
 *                     3. a bound value that is not numeric (string, IRI, blank node, boolean, dateTime, date, time, duration) fails the
 *                        EXECUTE with RDFGPU_ERR_UNSUPPORTED, the text naming MIN / MAX; the plan stays usable.  Such a row is never
 *                        answered differently (the 24-byte record has no room for such values, and the reference's order between
 *                        kinds is partial: its own order dependence);
 *                     4. otherwise every value is int, integer, decimal, float or double.  Each kind present gives a candidate: its
 *                        exact minimum (maximum) among that kind's values that are not NaN — int and integer compared as i64, decimal
 *                        as i128, float and double in IEEE order with the bit pattern deciding between the zeros (MIN prefers -0, MAX
 *                        +0); a kind whose values are all NaN gives a NaN candidate, and NaN candidates take part only if every
 *                        candidate is NaN.  A candidate is beaten if another is strictly less (greater) under Numeric::partial_cmp
 *                        (numeric.rs:90-99, with NumericPair::with_casts_from) — the comparison LT / GT use.  The result is the
 *                        unbeaten candidate of the lowest kind in the order int, integer, decimal, float, double, with its own tag and
 *                        payload (so RDFGPU_TV_INT can appear in an aggregate's array).  Of an all-NaN group only the tag and the
 *                        NaN-ness are promised, not the payload.
 *                   Why that is an answer of the reference: the casts of with_casts_from are monotone, so a value that is
 *                   reference-less than a candidate m is exactly less than m, and then its kind's candidate is reference-less than m
 *                   too; an unbeaten candidate is therefore not reference-greater than any value of the group, and put first in row
 *                   order it is never replaced.  (tests/test_minmax_cpu.py proves it by enumerating the orders.)
 *                   The result is a value column like any other aggregate's, under the same carriage and refusal rules.
 * Exactness.  Counts and every integer / decimal sum are exact and independent of row order (each value's i128 is added as 32-bit limbs
 * into u64 counters, carried and range-checked once per group: exact up to 2^32 rows per group).  The reference adds float and double
 * values one after the other in row order, so its result depends on that order; here the order is the device's, and the result satisfies
 *     |result - exact sum| <= n * eps * sum(|x_i|) + eta,  eps = 2^-24 and eta = 2^-149 for a float result, 2^-53 and 2^-1074 for a double one
 * where x_i is each value as the reference casts it (to f32 for a float result, to f64 for a double one), n the group's numeric values and
 * eta the spacing of the subnormals (a rounding near zero is absolute, not relative).  AVG divides that sum once more, correctly rounded.
 * The reference's integer / decimal overflow can depend on order too (a prefix overflows, the total does not); here the TOTAL decides.
 * Not on the device — refused with RDFGPU_ERR_UNSUPPORTED at compile, never answered differently: SAMPLE, GROUP_CONCAT, SUM / AVG
 * with DISTINCT, COUNT(DISTINCT *), more than RDFGPU_MAX_KEYS keys or RDFGPU_MAX_AGGREGATES aggregates; and, in a plan without
 * RDFGPU_PLAN_AGG_COLUMNS, the two functions above that need the flag.
 */
enum {
  RDFGPU_AGG_COUNT_STAR = 1, RDFGPU_AGG_COUNT = 2, RDFGPU_AGG_COUNT_DISTINCT = 3, RDFGPU_AGG_SUM = 4, RDFGPU_AGG_AVG = 5,
  RDFGPU_AGG_MIN = 6, RDFGPU_AGG_MAX = 7,   /* in plans compiled with RDFGPU_PLAN_AGG_COLUMNS; RDFGPU_ERR_UNSUPPORTED at compile without */
  /* reserved, RDFGPU_ERR_UNSUPPORTED at compile */
  RDFGPU_AGG_SAMPLE = 8, RDFGPU_AGG_GROUP_CONCAT = 9,
  RDFGPU_AGG_SUM_DISTINCT = 10, RDFGPU_AGG_AVG_DISTINCT = 11, RDFGPU_AGG_COUNT_DISTINCT_STAR = 12
};
#define RDFGPU_MAX_AGGREGATES 8u
#define RDFGPU_AGG_INPUT_EXPR 0x80000000u   /* bit 31 of an aggregate's input: the low 31 bits are the pool offset of (expr_off, expr_len) */
enum { RDFGPU_SORT_BY_ID = 0, RDFGPU_SORT_BY_TERM = 1,
       RDFGPU_SORT_BY_DOUBLE = 2,/* ENC_SORT of a numeric value: the sortable encoding orders numerics by Double::from(Numeric)
                                    (lib/encoding/src/sortable_term/builder.rs:36-39, lib/model/src/xsd/double.rs:92-102) in IEEE
                                    total order (-0 < +0, NaN last); unbound and non-numeric values sort first (the `xsd:double(...)`
                                    cast of BSBM explore Q10's ORDER BY yields an error = null for them).  Exact for Q10, whose
                                    prices are xsd:double literals; a decimal's cast goes through its lexical form in the
                                    reference and through the Decimal -> Double conversion here.                            */
       /* ABI 4 addendum, RDFGPU_NODE_SORT only */
       RDFGPU_SORT_BY_VALUE = 3  /* ENC_SORT of the typed value a value column's entry stands for: the reference's sortable encoding
                                    (lib/encoding/src/sortable_term/builder.rs:24-39,113-140, term_type.rs:56-70, as
                                    encoders/typed_value.rs:23-50 fills it; numeric.rs:52-60 for the bytes), the tuple (type, numeric,
                                    bytes).  Entry 0 (unbound, the error value) has type 0 — the encoder appends a valid struct of type
                                    Null, not an Arrow null — so unbound rows come first ascending and last descending.  A boolean has
                                    type 3, numeric 0.0 / 1.0 and its one byte.  INT / INTEGER / DECIMAL / FLOAT / DOUBLE have type 4,
                                    numeric = Double::from(Numeric) (a decimal through the Decimal -> Double routine, decimal.rs:445)
                                    compared in IEEE total order (-0 < +0, NaN after +inf), then the value's own big-endian bytes compared
                                    as byte strings (4 for INT and FLOAT, 8 for INTEGER and DOUBLE, 16 for DECIMAL; a string that is a
                                    prefix of another sorts first).  The 24-byte value record carries no other kinds.
                                    On the device a key is 64-bit words compared unsigned: one for an id form, 4 for BY_VALUE (type:3 |
                                    numeric:64 | bytes:128 | length:5), plus one word for the row index; at most 8 words in all, so that
                                    a tile of 1024 records fits 64 KB of LDS — (value, id, id, id) and (value, id) fit, two value keys
                                    do not (RDFGPU_ERR_UNSUPPORTED at compile).                                                */ };
#define RDFGPU_SORT_DESC 0x100u            /* RDFGPU_NODE_SORT, or-ed into right_keys[i]: key i descending                        */
enum { RDFGPU_JOIN_INNER = 0, RDFGPU_JOIN_LEFT = 1,
       /* ABI 4: JoinType::LeftSemi / JoinType::LeftAnti of HashJoinExec and NestedLoopJoinExec (CROSS_JOIN stays inner-only) — what
          FILTER EXISTS / FILTER NOT EXISTS become (correlated subqueries, lib/logical/src/expr_builder_context.rs:197-300, decorrelated
          by DataFusion) and what MINUS becomes (LeftAnti, lib/logical/src/minus/rewrite.rs:58-130).
          Output schema: the LEFT input's columns only; the node's projection indexes the left columns (at most 16); the join filter
          still sees [left cols, right cols].
          Rows: each left row appears at most once — it appears (SEMI) / does not appear (ANTI) when at least one right row matches it:
          equal on every key and the filter evaluates to exactly true (null or false is not a match).  Keys are NullEqualsNothing: a
          left row with a null (id 0) key never matches, so ANTI keeps it and SEMI drops it.
          NestedLoopJoinExec without a filter: SEMI keeps every left row when the right input has at least one row, ANTI keeps every
          left row when it has none (the EXISTS lowering for patterns that share no variable).
          Row order unspecified, as for the other joins; duplicate left rows are all kept.                                         */
       RDFGPU_JOIN_LEFT_SEMI = 2, RDFGPU_JOIN_LEFT_ANTI = 3,
       /* ABI 4 addendum: JoinType::LeftMark of HashJoinExec and NestedLoopJoinExec — what EXISTS becomes when it is an OPERAND (inside
          `||`, IF, a BIND: `Expr::Exists`, lib/logical/src/expr_builder_context.rs:197-300, is decorrelated by DataFusion into a
          LeftMark join wherever it is not a conjunct of its own).  Accepted only in a plan compiled with RDFGPU_PLAN_AGG_COLUMNS
          (RDFGPU_ERR_UNSUPPORTED at compile without it): the mark is a value column.
          Rows: every left row exactly once and IN LEFT INPUT ORDER (output row r is left row r).
          Output schema: [left cols, mark]; the node's projection indexes that, the mark at index n_left_cols (at most 16 columns);
          the join filter sees [left cols, right cols].
          The mark is true when at least one right row equals the left row on every key and the filter evaluates to exactly true,
          else false — never null: keys are NullEqualsNothing, a left row with a null key is false.  NestedLoopJoinExec without a
          filter: the mark is "the right input has a row".
          The mark column is a value column whose origin is the join node and whose value array has exactly two records,
          {RDFGPU_TV_BOOLEAN, 0} and {RDFGPU_TV_BOOLEAN, 1}: a row carries entry 1 (false) or 2 (true), never 0.  Everything a value column
          can do it can (ENC_TV in expressions above, SUM / COUNT / AVG, RDFGPU_SORT_BY_VALUE, a group column under RDFGPU_PLAN_VALUE_KEYS,
          rdfgpu_plan_result_values); what a value column is refused for stays refused (join key, COUNT DISTINCT, TopK, UNION, CLOSURE). */
       RDFGPU_JOIN_LEFT_MARK = 4 };
#define RDFGPU_MAX_KEYS 4u
#define RDFGPU_MAX_COLUMNS 16u
#define RDFGPU_MAX_GROUP_KEYS 8u   /* group columns of an RDFGPU_NODE_AGGREGATE in a plan compiled with RDFGPU_PLAN_VALUE_KEYS (else RDFGPU_MAX_KEYS) */
#define RDFGPU_NO_PROJECTION 0xFFFFFFFFu

typedef struct rdfgpu_plan_node {
  uint32_t kind;                          /* RDFGPU_NODE_*                                */
  int32_t left;                           /* child node index (or -1)                     */
  int32_t right;                          /* second child (joins) or -1                   */
  uint32_t join_type;                     /* RDFGPU_JOIN_*                                */
  rdfgpu_scan_instruction scan[4];        /* DATA_SOURCE: instructions in G,S,P,O order   */
  uint32_t n_keys;                        /* HASH_JOIN: number of equi-key pairs          */
  uint32_t left_keys[RDFGPU_MAX_KEYS];    /* column indices in the left child             */
  uint32_t right_keys[RDFGPU_MAX_KEYS];   /* column indices in the right child            */
  uint32_t expr_off;                      /* FILTER / join filter: offset into exprs      */
  uint32_t expr_len;                      /* 0 = no filter                                */
  uint32_t proj_off;                      /* projection: offset into the u32 pool         */
  uint32_t n_proj;                        /* RDFGPU_NO_PROJECTION = keep all columns      */
  uint32_t table_slot;                    /* TABLE: which bound table (rdfgpu_plan_bind_table) */
  uint32_t table_cols;                    /* TABLE: number of columns                     */
} rdfgpu_plan_node;

typedef struct rdfgpu_regex {             /* one constant REGEX pattern of the plan (UTF-8, not NUL-terminated) */
  const char* pattern;
  const char* flags;                      /* SPARQL flags: any of s m i x q (regex.rs:107-141); may be NULL    */
  uint32_t pattern_len;
  uint32_t flags_len;
  uint32_t pattern_id;                    /* RDFGPU_EX_REGEX_VAR entries: the object id of this pattern literal; else 0 */
  uint32_t reserved;
} rdfgpu_regex;

typedef struct rdfgpu_plan_desc {
  const rdfgpu_plan_node* nodes;
  uint32_t n_nodes;
  uint32_t root;                          /* index of the root node                       */
  const rdfgpu_expr_node* exprs;
  uint32_t n_exprs;
  const uint32_t* pool;                   /* IN-set ids and projection lists              */
  uint32_t n_pool;
  uint32_t flags;                         /* RDFGPU_PLAN_*                                */
  const rdfgpu_regex* regexes;            /* patterns referenced by RDFGPU_EX_REGEX nodes */
  uint32_t n_regexes;
  uint32_t reserved;
} rdfgpu_plan_desc;
#define RDFGPU_PLAN_ALLOW_OPAQUE 1u
#define RDFGPU_PLAN_AGG_COLUMNS 2u        /* ABI 4 addendum: aggregate values are columns (RDFGPU_NODE_AGGREGATE) */
#define RDFGPU_PLAN_VALUE_KEYS 4u         /* ABI 4 addendum: value columns may be group columns, up to RDFGPU_MAX_GROUP_KEYS of them (RDFGPU_NODE_AGGREGATE);
                                             valid only together with RDFGPU_PLAN_AGG_COLUMNS, alone it is RDFGPU_ERR_INVALID */

/* ------------------------------------------------------------------------------------ */
/* 4. Plans: compile, execute on device, stream result batches                           */
/*    replaces plan_extension (lib/storage/src/memory/planner.rs:31-64),                 */
/*    DataSource::open (pattern_data_source.rs:42-58), the stream's poll_next             */
/*    (stream.rs:39-63) and ExecutionPlan::execute of the join/filter subtree             */
/* ------------------------------------------------------------------------------------ */
typedef struct rdfgpu_plan rdfgpu_plan;

typedef struct rdfgpu_metrics {
  uint64_t output_rows;      /* BaselineMetrics::output_rows (stream.rs:48-63)            */
  uint64_t input_rows;       /* index rows covered by the located scan ranges             */
  uint64_t intermediate_rows;/* sum of rows produced by all non-root operators            */
  uint64_t device_bytes;     /* bytes of HBM held by this plan's intermediates            */
  double elapsed_compute_ms; /* device time of the last execute (HIP events)              */
  uint32_t kernels_launched;
  uint32_t host_syncs;
  /* ABI 3: why an execution was slow, when it was */
  uint32_t exact_reruns;     /* speculative sizes did not fit: the execution ran again with exact sizes (0 or 1)            */
  uint32_t device_mallocs;   /* hipMalloc calls the store's pools had to make during this execution (0 in steady state)     */
  double device_malloc_ms;   /* .. and the host time spent inside them                                                      */
  uint32_t tables_built;     /* join tables of store slices built (not found cached) during this execution                  */
  uint32_t reserved;
} rdfgpu_metrics;

/* Validates the description, chooses an index per data source (IndexPermutations::choose_index,
   permutations.rs:81-96) and allocates a HIP stream.  Does not launch kernels. */
int rdfgpu_plan_compile(rdfgpu_store* store, const rdfgpu_plan_desc* desc, rdfgpu_plan** out);
void rdfgpu_plan_destroy(rdfgpu_plan* plan);

/* Supplies the columns of a RDFGPU_NODE_TABLE (device pointers into this device's HBM,
   n rows each; must stay valid until the next execute finishes). */
int rdfgpu_plan_bind_table(rdfgpu_plan* plan, uint32_t slot, const uint32_t* const* cols,
                           uint32_t n_cols, uint64_t n_rows);

/* Runs the whole operator tree on the device.  The result stays in HBM.  Re-executable.
 *
 * On return the result's row count and every check of the execution (speculation, run-time errors) are final; the result's ROWS may
 * still be being written.  A plan whose root is a band join emitting from a slice's list (the batched BSBM Q5) learns its count in
 * front of that join's emit pass and returns while the pass — the execution's tail — runs on the plan's stream
 * (rdfgpu_early_count_eligible; RDFGPU_OPT_NO_EARLY_RESULT_COUNT restores the wait for the whole stream).  What that means for a caller:
 *   - rdfgpu_plan_result_info, _bind_table, _set_option, _enable_kernel_timing and _stream do not wait for the tail; every entry that
 *     reads result memory or finished metrics, or hands result memory out (rdfgpu_plan_fetch, _result_device, _agg_fetch, _agg_device,
 *     _result_values, _result_values_fetch, _next, _decode_terms, _rewind, _metrics, _kernel_stats) completes it first, and so does
 *     rdfgpu_plan_destroy.  Pointers from rdfgpu_plan_result_device are therefore complete for a consumer on any stream;
 *   - the tail reads no caller-bound table: the tables bound for an execution may be rebound or freed once execute has returned;
 *   - the next execute of the plan does not wait for the tail either (its work is ordered behind it on the plan's stream), and the
 *     store's mutations (extend, remove, clear, drop_tables, set_typed_values, set_strings) wait for every pending tail themselves;
 *   - rdfgpu_metrics.elapsed_compute_ms is 0 until the tail has been completed; host_syncs counts the waits inside execute, as before. */
int rdfgpu_plan_execute(rdfgpu_plan* plan);

/* Result shape.  Does not wait: the count is final when execute returns, whether or not its tail is still running. */
int rdfgpu_plan_result_info(rdfgpu_plan* plan, uint64_t* n_rows, uint32_t* n_cols);
/* *out = 1 while the last execute's tail (see rdfgpu_plan_execute) has not been completed by a call on this plan, else 0. */
int rdfgpu_plan_tail_pending(rdfgpu_plan* plan, uint32_t* out);
/* Device pointers of the result columns (valid until the next execute / destroy of THIS plan — also across mutations of the
   store: an executed plan keeps the store generation its result may point into, and keeps showing the pre-mutation rows,
   like the reference's plan keeps its snapshot, snapshot.rs:35-37). */
int rdfgpu_plan_result_device(rdfgpu_plan* plan, const uint32_t** cols, uint32_t cap_cols);
/* Copies the whole result to caller-owned host columns (each with room for n_rows). */
int rdfgpu_plan_fetch(rdfgpu_plan* plan, uint32_t* const* host_cols, uint32_t n_cols);
/*
 * ABI 4 addendum: the aggregate values of a RDFGPU_NODE_AGGREGATE root, one per result row and aggregate (row i of aggregate a belongs
 * to row i of the key columns).  24 bytes each:
 *   tag RDFGPU_TV_INTEGER   lo = the value (counts, integer sums)
 *   tag RDFGPU_TV_DECIMAL   (lo, hi) = the i128 value * 10^18
 *   tag RDFGPU_TV_FLOAT     lo = the IEEE-754 binary32 bits (zero-extended);  RDFGPU_TV_DOUBLE: lo = the binary64 bits
 *   tag RDFGPU_TV_NULL      the error value
 * A MIN / MAX keeps the tag of the value it picked, so RDFGPU_TV_INT (lo = the xsd:int value) can appear in its array.  In the array of
 * an RDFGPU_NODE_EXTEND's computed column two more tags can appear:
 *   tag RDFGPU_TV_INT       lo = the xsd:int value;  tag RDFGPU_TV_BOOLEAN: lo = 0 / 1
 * The host turns integers into xsd:integer terms (INT64_AS_TERM) and the rest into typed literals.
 */
typedef struct rdfgpu_agg_value {
  int64_t lo;
  int64_t hi;
  uint8_t tag;
  uint8_t reserved[7];
} rdfgpu_agg_value;
/* Number of aggregate columns of the executed result (0 unless the root is an RDFGPU_NODE_AGGREGATE with aggregates). */
int rdfgpu_plan_agg_count(rdfgpu_plan* plan, uint32_t* n_aggs);
/* Copies aggregate `agg` of every result row (n_rows of rdfgpu_plan_result_info) to caller-owned host memory. */
int rdfgpu_plan_agg_fetch(rdfgpu_plan* plan, uint32_t agg, rdfgpu_agg_value* host);
/* Device pointer of aggregate `agg` (n_rows values; valid until the next execute / destroy of this plan; NULL when there are no rows). */
int rdfgpu_plan_agg_device(rdfgpu_plan* plan, uint32_t agg, const rdfgpu_agg_value** values);
/*
 * ABI 4 addendum, plans compiled with RDFGPU_PLAN_AGG_COLUMNS: rdfgpu_plan_result_info / _device / _fetch count and deliver the value
 * columns like any other column (u32 entries), and rdfgpu_plan_agg_count reports 0.
 * rdfgpu_plan_result_values: the device array result column `col` indexes and its length — entry e of the column (1-based; 0 = unbound)
 * is (*values)[e - 1].  An object-id column answers NULL and 0.  Valid until the next execute / destroy of this plan.
 * rdfgpu_plan_result_values_fetch: one value per result row (n_rows of rdfgpu_plan_result_info), gathered on the host; tag 0
 * (RDFGPU_TV_NULL) where the entry is 0.  RDFGPU_ERR_INVALID for an object-id column.
 */
int rdfgpu_plan_result_values(rdfgpu_plan* plan, uint32_t col, const rdfgpu_agg_value** values, uint64_t* n);
int rdfgpu_plan_result_values_fetch(rdfgpu_plan* plan, uint32_t col, rdfgpu_agg_value* host);
/*
 * SendableRecordBatchStream::poll_next (stream.rs:39-63): exports the next batch of at
 * most batch_size rows as an Arrow struct array of UInt32 children (format "+s" / "I");
 * id 0 becomes a null.  Never yields an empty batch (scan.rs:195-198).  Returns
 * RDFGPU_END once drained.  `schema` may be NULL.  ABI 4 addendum: after the key columns, each
 * aggregate of an RDFGPU_NODE_AGGREGATE root is one more child, a struct "+s" of
 * tag: uint8 "C", lo: int64 "l", hi: int64 "l" (rdfgpu_agg_value), null where the tag is 0.  With RDFGPU_PLAN_AGG_COLUMNS a value
 * column is such a struct child in its own place among the columns, null where its entry is 0.
 */
int rdfgpu_plan_next(rdfgpu_plan* plan, struct ArrowArray* out, struct ArrowSchema* schema);
/* Restarts the batch stream over the current result. */
int rdfgpu_plan_rewind(rdfgpu_plan* plan);
int rdfgpu_plan_metrics(rdfgpu_plan* plan, rdfgpu_metrics* out);
/* Index chosen for a DATA_SOURCE node (RDFGPU_GSPO..), for plan display ("[GPOS] subject=…"). */
int rdfgpu_plan_selected_index(const rdfgpu_plan* plan, uint32_t node, uint32_t* components);
/* Opaque hipStream_t of the plan, so the host can order its own work after it. */
int rdfgpu_plan_stream(rdfgpu_plan* plan, void** hip_stream);
/*
 * ENC_PT of a result column (MemObjectIdMapping::decode_array, lib/storage/src/memory/object_id_mapping.rs:331-374): object
 * ids -> plain terms, decoded on the device from the store's string heap (rdfgpu_store_set_strings must hold the lexical
 * form of EVERY id that can appear) and typed-value table.  Rows [first_row, first_row + n_rows) of column `col`, as an
 * Arrow struct array
 *     struct<term_type: uint8, value: utf8, tag: uint8, aux: uint32>
 * term_type = PlainTermType (plain_term/encoding.rs:90-127: 0 named node, 1 blank node, 2 literal); value = the lexical
 * form; a null struct where the id is 0 / unknown (builder.append_null()).  data_type and language_tag of the reference's
 * struct are functions of (tag, aux) through the host's small tables — tag = the datatype of a typed literal (the ABI's
 * RDFGPU_TV_*; RDFGPU_TV_OTHER: aux = the host's datatype id), aux = the language id of a string (0 = none) — and are
 * attached there as dictionary arrays: the per-row string work, the gather of n_rows lexical forms out of the heap,
 * happens here.  The lexical forms of one call may not exceed 2^31 - 1 bytes (utf8 offsets are int32): decode fewer rows.
 */
int rdfgpu_plan_decode_terms(rdfgpu_plan* plan, uint32_t col, uint64_t first_row, uint64_t n_rows,
                             struct ArrowArray* out, struct ArrowSchema* schema);

/*
 * Filter push-down into a DataSourceExec leaf.  When a subtree is NOT fused into one rdfgpu plan, DataFusion's physical
 * filter push-down offers the leaf the filters above it (MemQuadPatternDataSource::try_pushdown_filters,
 * lib/storage/src/memory/storage/pattern_data_source.rs:107-151): id-level comparisons of a bound variable with an object
 * id, their conjunctions on one column, literal `true`, and DynamicFilterPhysicalExprs (predicate_pushdown.rs:62-157,
 * 161-249).  A filter here is the MemStoragePredicateExpr the host already extracted (MemStoragePredicateExpr::try_from).
 */
enum { RDFGPU_PUSH_UNSUPPORTED = 0,  /* try_from returned None: answered PushedDown::No, nothing changes                  */
       RDFGPU_PUSH_TRUE = 1,         /* literal true                                                                       */
       RDFGPU_PUSH_BINARY = 2,       /* column <op> object id, op = RDFGPU_OP_*                                             */
       RDFGPU_PUSH_BETWEEN = 3 };    /* from <= column <= to (what `>` AND `<=` on one column become, :189-249)             */
typedef struct rdfgpu_pushdown_filter {
  uint32_t kind;      /* RDFGPU_PUSH_*                                                        */
  uint32_t var;       /* the variable slot of the column (rdfgpu_scan_instruction.var)        */
  uint32_t op;        /* BINARY: RDFGPU_OP_EQ / GT / GTEQ / LT / LTEQ                         */
  uint32_t value;     /* BINARY: the object id                                                */
  uint32_t from, to;  /* BETWEEN, inclusive                                                   */
} rdfgpu_pushdown_filter;
/*
 * try_pushdown_filters on DATA_SOURCE node `node` of a compiled plan: pushed[i] receives 1 (PushedDown::Yes) or 0.  Every
 * supported filter is AND-ed into the instruction that binds its variable (MemIndexScanInstructions::apply_filter,
 * scan_instructions.rs:101-133, through try_and_with :170-210) and the index is chosen again (apply_pushdown_filters ->
 * try_find_better_index, pattern_data_source.rs:155-165, scan.rs:469-486).  The change is permanent for this plan.
 * Errors like the reference: a filter on a variable the pattern does not bind, or one that cannot be combined
 * (EqualTo), is RDFGPU_ERR_INVALID.
 */
int rdfgpu_plan_pushdown_filters(rdfgpu_plan* plan, uint32_t node, const rdfgpu_pushdown_filter* filters, uint32_t n, uint8_t* pushed);
/*
 * The CURRENT predicates of the leaf's dynamic filters — a HashJoinExec publishes its build side's key bounds when the
 * build finishes; the scan reads them on its first next() (combine_instructions_with_dynamic_filters, scan.rs:241-261) and
 * may switch index for them (collect_relevant_row_groups, scan.rs:217-239).  Applied on top of the static instructions by
 * every execute until replaced; n = 0 clears.  Only BINARY / BETWEEN / TRUE kinds.
 */
int rdfgpu_plan_set_dynamic_filters(rdfgpu_plan* plan, uint32_t node, const rdfgpu_pushdown_filter* filters, uint32_t n);
/*
 * One level of the leaf as it will be scanned (after push-down / with the current dynamic filters): level 0..3 in G,S,P,O
 * order; `*pred` as in rdfgpu_predicate (IN sets with one id: from = to = the id, n_ids = 1; larger sets: n_ids only).
 * For plan display: "[GPOS] subject=?s, predicate=<p>, object=?o" + "object in (2..9)" (pattern_data_source.rs:192-234).
 */
struct rdfgpu_predicate;
int rdfgpu_plan_source_predicate(const rdfgpu_plan* plan, uint32_t node, uint32_t level, struct rdfgpu_predicate* pred);

/*
 * Per-kernel device timing of the last execute (HIP events on the plan's stream, around every
 * launch) with the algorithmic bytes each kernel class had to move (formulas: DESIGN.md,
 * from SURVEY.md §8d).  The equivalent of DataFusion's per-operator BaselineMetrics
 * (elapsed_compute, stream.rs:48-63), at kernel granularity.  Off by default.
 */
typedef struct rdfgpu_kernel_stat {
  const char* kernel;        /* device function name as rocprofv3 prints it (prefix match)  */
  uint32_t launches;
  uint32_t reserved;
  double total_ms;           /* sum of HIP-event durations of those launches                */
  uint64_t algorithmic_bytes;/* sum over those launches                                     */
  uint64_t rows_in;          /* rows streamed by those launches                             */
} rdfgpu_kernel_stat;
/* on = 1: every launch of the plan's later executions is bracketed with HIP events (two events per launch: ~5 us of stream time
 * each, a tenth of a short step); on = 2: only the launches of the kernel that took longest in the last execution timed with
 * on = 1 — the one a roofline is quoted for — so that a timed region is not slowed down by its own instrumentation; 0: off. */
int rdfgpu_plan_enable_kernel_timing(rdfgpu_plan* plan, int on);
int rdfgpu_plan_kernel_stats(rdfgpu_plan* plan, rdfgpu_kernel_stat* out, uint32_t cap, uint32_t* n);

/* ------------------------------------------------------------------------------------ */
/* 4b. Engine options                                                                    */
/*     the session-level knobs of this path: the counterpart of DataFusion's SessionConfig */
/*     / ConfigOptions the reference threads through planning (lib/rdf-fusion/src/store.rs */
/*     :101-103, bench/src/environment.rs:71-87).  Every physical rewrite / table form /   */
/*     speculation mode can be switched off; results never depend on them (tested).       */
/* ------------------------------------------------------------------------------------ */
/*
 * Defaults are taken ONCE per process (first store creation) from the environment variables RDFGPU_<NAME>
 * (e.g. RDFGPU_NO_CHAIN_FUSION=1); after that the environment is never consulted again.  A store copies the
 * process defaults when it is created, a plan copies its store's options when it is compiled; the two setters
 * change one store (plans compiled later) or one plan (its later executions).  Nothing on the execute path reads
 * the environment.
 */
enum {
  RDFGPU_OPT_FORCE_GENERIC_VM = 0,      /* every FILTER / join filter through the stack VM (no specialised kernels)   */
  RDFGPU_OPT_NO_JOIN_REORDER,           /* keep (A x B) JOIN C as written                                             */
  RDFGPU_OPT_NO_SPECULATION,            /* size every operator exactly (one host sync per join)                       */
  RDFGPU_OPT_NO_FIRST_RUN_SPECULATION,  /* speculate only from a previous execution's cardinalities                   */
  RDFGPU_OPT_NO_STRING_VERDICTS,        /* REGEX / CONTAINS / .. per row instead of per distinct term                 */
  RDFGPU_OPT_NO_TABLE_CACHE,            /* join tables are built inside every execution, like HashJoinExec(CollectLeft)
                                           does per query; nothing is kept on the store between executions            */
  RDFGPU_OPT_NO_INDEX_JOIN,             /* never build on a store slice just because it is one                        */
  RDFGPU_OPT_NO_CHAIN_FUSION,           /* run follow-up look-up joins as separate operators                          */
  RDFGPU_OPT_NO_VALUE_TABLES,           /* no decoded integer tables next to direct tables                            */
  RDFGPU_OPT_NO_RANGE_INDEX,            /* no value-ordered CSR groups                                                */
  RDFGPU_OPT_NO_FILTER_FUSION,          /* materialise FilterExec children of joins                                   */
  RDFGPU_OPT_NO_LDS_JOIN,               /* chained HBM hash join (count / scan / write) for every HashJoinExec         */
  RDFGPU_OPT_NO_GLOBAL_TABLE_JOIN,      /* the fused join kernel only for builds that fit LDS                         */
  RDFGPU_OPT_NO_DIRECT_TABLE,           /* no direct-address / CSR tables for dense keys                              */
  RDFGPU_OPT_NO_BAND_JOIN,              /* no key-partitioned band join for fused look-up chains over small groups    */
  RDFGPU_OPT_NO_PARTITIONED_JOIN,       /* no radix-partitioned LDS hash join for large non-cached build sides        */
  RDFGPU_OPT_NO_VALUE_VERDICTS,         /* typed comparison per row instead of per distinct term of a sorted slice     */
  RDFGPU_OPT_NO_PRIMING,                /* no priming run over the first rows of big bound tables before a plan's first execution */
  RDFGPU_OPT_NO_ORDERED_JOIN,           /* no slice-ordered emission of a table x slice join / no sort-free band join on it */
  RDFGPU_OPT_NO_BAND_PACK16,            /* band join: both windows always tested with 32-bit arithmetic                    */
  RDFGPU_OPT_NO_RUN_COPY,               /* .. per distinct term, but rows streamed (verdict bits) instead of runs copied */
  RDFGPU_OPT_NO_RANGE_PARTITION,        /* partitioned join: hash-partition BOTH sides even when the probe side is a slice sorted by a join key */
  RDFGPU_OPT_LDS_MAX_BUILD,             /* value: largest build side (rows) joined through a per-workgroup LDS table  */
  RDFGPU_OPT_CSR_ROW_LANES_LOG2,        /* value + 1: lanes sharing one probe row of a CSR join (0 = automatic)        */
  RDFGPU_OPT_JOIN_WAVE_Q,               /* value: entries of a wave's candidate queue (0 = automatic)                  */
  RDFGPU_OPT_PARTITION_MIN_BUILD,       /* value: smallest non-cached build side (rows) that is radix-partitioned (default 2^21) */
  RDFGPU_OPT_PARTITION_TWO_PASS_ROWS,   /* value: expected output rows from which a partitioned join counts before it writes (default 50 M) */
  RDFGPU_OPT_NO_OWN_PARTITION_PASS,     /* flag: partitioned join: partition ids materialised and sorted with rocPRIM's radix sort instead of the hand-written passes */
  RDFGPU_OPT_NO_BAND_COMPACT,           /* flag: band join fed by an ordered slice join: 32-byte {record, aux} row records even where 16 bytes would do */
  RDFGPU_OPT_NO_PROBE_OUTER_JOIN,       /* flag: LEFT joins always build on their left input (no probe-preserving form over the right input's slice table) */
  RDFGPU_OPT_NO_STREAM_JOIN,            /* flag: joins against a direct-address table always take the generic queueing kernel (no register-resident streaming form) */
  RDFGPU_OPT_PARTITION_ROWS,            /* value: build rows per partition a partitioned join aims for (0 = automatic: 1024)   */
  RDFGPU_OPT_PARTITION_SLOTS,           /* value: slots of a partition's LDS table, a power of two from 1024 to 8192 (0 = automatic: 4096); a partition with more than slots / 2 build rows is joined chunk by chunk */
  RDFGPU_OPT_NO_SEMI_LDS,               /* flag: semi / anti joins never build their set of right rows in LDS (the HBM set, built per execution) */
  RDFGPU_OPT_NO_BAND_PAIR_COUNTS,       /* flag: band join emitting from a slice's list of surviving pairs: no per-row counts of the verdicts are read, every step streams the verdict bits to count its blocks' rows */
  RDFGPU_OPT_BAND_PAIR_COUNT_BLOCKS,    /* value: the smallest number of 64 x 64 blocks from which a step counts from the per-row counts, 64 bytes per block, instead of the bits (0 = automatic: 2^16 blocks = 32 MiB of verdicts) */
  RDFGPU_OPT_NO_EARLY_RESULT_COUNT,     /* flag: rdfgpu_plan_execute never returns at a band join's count point: it waits for the whole stream, the emit pass included, as it did before the early count existed (the newest flag; it sits here because the bindings' tests pin the five names that follow as the end of the list) */
  RDFGPU_OPT_NO_BAND_ROW_CACHE,         /* flag: band join reading a slice's rows in place: the rows' decoded windows are not kept on the slice, every step gathers 16-byte records by key */
  RDFGPU_OPT_NO_BAND_PAIR_LIST,         /* flag: band join streaming a slice's cached pair verdicts: no list of the surviving pairs is kept beside them, every step expands the verdict bits into rows */
  RDFGPU_OPT_NO_BAND_PAIR_CACHE,        /* flag: band join reading a slice's rows in place with the rows' windows kept: the pair test's verdicts are not kept on the slice, every step tests every pair */
  RDFGPU_OPT_BAND_PAIR_CACHE_BLOCKS,    /* value: the largest number of 64 x 64 blocks whose verdicts are kept on a slice, 512 bytes each (0 = automatic: 2^21 blocks = 1 GiB) */
  RDFGPU_OPT_NO_AGG_LDS,                /* flag (ABI 4 addendum): AggregateExec never keeps per-workgroup partial accumulators in LDS (every row adds into the HBM accumulators) */
  RDFGPU_OPT__COUNT
};
int rdfgpu_store_set_option(rdfgpu_store* store, uint32_t option, uint64_t value);
int rdfgpu_store_get_option(const rdfgpu_store* store, uint32_t option, uint64_t* value);
int rdfgpu_plan_set_option(rdfgpu_plan* plan, uint32_t option, uint64_t value);
/* "NO_CHAIN_FUSION" for RDFGPU_OPT_NO_CHAIN_FUSION (the environment variable is RDFGPU_ + this); NULL if out of range. */
const char* rdfgpu_option_name(uint32_t option);

/* ------------------------------------------------------------------------------------ */
/* 5. Host logic of the scan planner (no device access)                                  */
/* ------------------------------------------------------------------------------------ */
/*
 * MemQuadIndex::compute_scan_score (quad_index.rs:100-130): `instr` is in the order of the
 * index being scored.
 */
uint64_t rdfgpu_scan_score(const rdfgpu_scan_instruction instr[4]);
/*
 * IndexPermutations::choose_index (permutations.rs:81-96): `gspo` is in G,S,P,O order;
 * `available` is a bit mask of RDFGPU_GSPO.. permutations the store keeps; returns the
 * chosen permutation (ties prefer the first listed).
 */
uint32_t rdfgpu_choose_index(const rdfgpu_scan_instruction gspo[4], uint32_t available);
/*
 * Band join reading a slice's rows in place: are the rows' decoded windows kept on the slice (1) or gathered by key every step (0)?
 * operand_src / operand_keyed_by_join_key: per window w its two operands at [2w], [2w + 1] — where the ordered slice join below takes
 * the operand from (0 = table row, 1 = slice row, 2 + t = stage t's row) and whether that stage's key column is the join's own key.
 * option_set: RDFGPU_OPT_NO_BAND_ROW_CACHE.  A negative status on invalid arguments.
 */
int rdfgpu_band_row_cache_eligible(uint32_t in_place, uint32_t compact, uint32_t pack16, uint32_t option_set, uint32_t n_win,
                                   const uint32_t operand_src[4], const uint32_t operand_keyed_by_join_key[4]);
/*
 * .. and are the pair test's verdicts kept on the slice beside them (1) or is every pair tested every step (0)?  row_windows: the rows' windows are kept
 * (rdfgpu_band_row_cache_eligible, and the store's operands accepted); neq_self, pack16: the pair test is the packed form whose `!=` is by entry index;
 * option_set: RDFGPU_OPT_NO_BAND_PAIR_CACHE; n_blocks: blocks of the in-place layout; cap_blocks: RDFGPU_OPT_BAND_PAIR_CACHE_BLOCKS (0 = 2^21; inclusive).
 */
int rdfgpu_band_pair_cache_eligible(uint32_t row_windows, uint32_t neq_self, uint32_t pack16, uint32_t option_set, uint64_t n_blocks, uint64_t cap_blocks);
/*
 * .. and is a list of the surviving pairs kept beside the verdicts, 2 bytes per pair in the order the rows come out, for the emit pass to read instead of the bits (1),
 * or does every step expand the bits (0)?  pair_cached: the step streams the slice's cached verdicts; option_set: RDFGPU_OPT_NO_BAND_PAIR_LIST; survivors: set bits of
 * the verdicts; n_blocks: blocks of the in-place layout.  Kept when the list is no larger than the bits it stands in for, 2 * survivors <= 512 * n_blocks, and its
 * 32-bit offsets cannot wrap (n_blocks < 2^20).
 */
int rdfgpu_band_pair_list_eligible(uint32_t pair_cached, uint32_t option_set, uint64_t survivors, uint64_t n_blocks);
/*
 * .. and does a step that emits from the list count its blocks' rows from the per-row counts kept with the list, one byte per (block, row), without reading the
 * verdict bits (1), or does it stream the bits (0)?  has_list: the step emits from the slice's list; option_set: RDFGPU_OPT_NO_BAND_PAIR_COUNTS; n_blocks: blocks of
 * the in-place layout; min_blocks: RDFGPU_OPT_BAND_PAIR_COUNT_BLOCKS (inclusive; 0 = 2^16 blocks, whose 32 MiB of verdicts are the size of the L2).
 */
int rdfgpu_band_pair_count_eligible(uint32_t has_list, uint32_t option_set, uint64_t n_blocks, uint64_t min_blocks);
/*
 * The form one band-join step runs in, the one decision the four above feed: 0 RECORDS (row records by key, every route that does not read the slice's rows through
 * their cached windows), 1 ROW_WINDOWS (the pair test over the cached windows), 2 VERDICTS (the cached verdicts, bits expanded by the emit pass), 3 VERDICTS_LIST (..
 * emitted from the slice's list), 4 COUNTS_LIST (.. and counted from the list's per-row counts).  row_static: the step reads the slice's rows in place through their
 * cached windows; has_verdicts, has_list: the slice keeps the verdicts / the list with its counts for this chain; list_option_set, counts_option_set:
 * RDFGPU_OPT_NO_BAND_PAIR_LIST and RDFGPU_OPT_NO_BAND_PAIR_COUNTS; n_row_cols: output columns taken from the row (the list serves at most one); n_blocks, min_blocks: as for
 * rdfgpu_band_pair_count_eligible.
 */
int rdfgpu_band_step_form(uint32_t row_static, uint32_t has_verdicts, uint32_t has_list, uint32_t list_option_set, uint32_t counts_option_set,
                          uint32_t n_row_cols, uint64_t n_blocks, uint64_t min_blocks);
/*
 * The probe pass of the ordered slice join below such a band join: 0 FULL (the multimap, the stage rows and the packed records, launched where that join runs: every
 * other route), 1 LEAN (owed by that join and run by the band join as one pass that writes the batch's values by key), 2 FULL_NOW (owed, and the full pass runs in front of
 * the count pass after all).  held, in_place, row_cache: what the band join's last execution left (the write pass is held back for it; it read the slice's rows in place and
 * no key had two table rows; the rows' windows were cached on the slice); option_set: RDFGPU_OPT_NO_BAND_ROW_CACHE; row_static: the band join's step took a form that reads
 * the slice's rows through their cached windows — the ordered join itself asks with 1, and owes its probe unless the answer is FULL.
 */
int rdfgpu_oj_probe_form(uint32_t held, uint32_t in_place, uint32_t row_cache, uint32_t option_set, uint32_t row_static);
/*
 * May rdfgpu_plan_execute return at a band join's count point, in front of its emit pass (1), or does it wait for the whole stream (0)?  is_root: the band join's
 * output node is the plan's root; result_is_output: nothing is launched behind emit (no left-join tail, no held-back write pass); form: the step's form as
 * rdfgpu_band_step_form numbers it (3 VERDICTS_LIST and 4 COUNTS_LIST qualify); skip_slow: the full-semantics pass is not launched; speculative, priming: the
 * execution's mode; timing: rdfgpu_plan_enable_kernel_timing is on; option_set: RDFGPU_OPT_NO_EARLY_RESULT_COUNT.  A negative status on an unknown form.
 */
int rdfgpu_early_count_eligible(uint32_t is_root, uint32_t result_is_output, uint32_t form, uint32_t skip_slow, uint32_t speculative, uint32_t priming, uint32_t timing, uint32_t option_set);
/*
 * MemIndexScanPredicate::try_and_with (scan_instructions.rs:170-210).  Predicates are given
 * as (pred, a, b) triples where IN sets are explicit arrays.  Writes the combined predicate;
 * `out_ids` needs room for min(na, nb) ids.  Returns 1 if combinable, 0 if not (EqualTo).
 */
typedef struct rdfgpu_predicate {
  uint32_t pred;        /* RDFGPU_PRED_*                                                  */
  uint32_t from, to;    /* BETWEEN                                                        */
  const uint32_t* ids;  /* IN (sorted unique)                                             */
  uint32_t n_ids;
  uint32_t equal_to;    /* EQUAL_TO variable slot                                         */
} rdfgpu_predicate;
int rdfgpu_predicate_and(const rdfgpu_predicate* lhs, const rdfgpu_predicate* rhs,
                         rdfgpu_predicate* out, uint32_t* out_ids);
/*
 * MemStoragePredicateExpr::to_scan_predicate (predicate_pushdown.rs:120-157): rewrites
 * `column <op> value` into a scan predicate.  op: 0 Eq, 1 Gt, 2 GtEq, 3 Lt, 4 LtEq.
 * Returns 1 and fills `out` (BETWEEN / IN with one id in out->from / FALSE).
 */
enum { RDFGPU_OP_EQ = 0, RDFGPU_OP_GT = 1, RDFGPU_OP_GTEQ = 2, RDFGPU_OP_LT = 3, RDFGPU_OP_LTEQ = 4 };
int rdfgpu_pushdown_to_scan_predicate(uint32_t op, uint32_t value, rdfgpu_predicate* out);

/*
 * compile_pattern (scalar/strings/regex.rs:107-141) for the device: checks that a REGEX pattern / flags pair is inside
 * the supported subset (csrc/regex_compile.hpp) without touching a device.  Returns RDFGPU_OK and the number of
 * automaton positions in *positions (0 for a pattern that can only yield the error value: an invalid flag), or
 * RDFGPU_ERR_UNSUPPORTED with the reason in rdfgpu_last_error() — exactly what rdfgpu_plan_compile would answer.
 */
int rdfgpu_regex_check(const char* pattern, uint32_t pattern_len, const char* flags, uint32_t flags_len, uint32_t* positions);

/* ------------------------------------------------------------------------------------ */
/* 6. Multi-GPU exchange steps (one process per GPU; no reference counterpart) */
/* ------------------------------------------------------------------------------------ */
/*
 * Triples are sharded by rdfgpu_shard_of(subject) over the ranks of a communicator; object ids are global and the typed-value
 * table is replicated.  Joins on the shard key are local; the other two cases are one exchange step each, on binding tables
 * that live in HBM (e.g. rdfgpu_plan_result_device of one plan -> rdfgpu_plan_bind_table of the next):
 *   rdfgpu_exchange_allgatherv   every rank contributes its rows, every rank receives all ranks' rows (rank order)
 *   rdfgpu_exchange_repartition  row i goes to rank rdfgpu_shard_of(cols[key_col][i]): re-shards a table by the key of the
 *                                next join.  STABLE: a rank receives, source rank after source rank, that rank's rows for it
 *                                in their original order (a table sorted by key_col arrives as `world` sorted runs; the
 *                                received bytes do not depend on scheduling)
 * Row counts travel first, receive buffers are sized from them (nothing is padded or clipped).  Both calls are collective
 * (every rank of the communicator calls them in the same order) and return when the received columns are complete; the
 * columns belong to the communicator and stay valid until its next exchange.
 * Transport: RCCL over xGMI (grouped ncclSend / ncclRecv, one pair per peer; the library dlopens librccl.so.1), or — for
 * several ranks on one GPU and for tests — staging through host memory with the wire supplied by the caller.
 */
typedef struct rdfgpu_comm rdfgpu_comm;
#define RDFGPU_COMM_ID_BYTES 128
/* ncclGetUniqueId: called on one rank, the 128 bytes are handed to the others by the launcher (torchrun's store, MPI, a file). */
int rdfgpu_comm_unique_id(uint8_t id[RDFGPU_COMM_ID_BYTES]);
/* ncclCommInitRank on `device` (-1 = current). */
int rdfgpu_comm_create(const uint8_t id[RDFGPU_COMM_ID_BYTES], uint32_t rank, uint32_t world, int32_t device, rdfgpu_comm** out);
/* The caller's wire: an all-to-all of byte blocks in host memory — block p of `send` (send_bytes[p] bytes, blocks back to back)
   goes to rank p, block p of `recv` (recv_bytes[p] bytes) comes from rank p; returns 0 on success. */
typedef int (*rdfgpu_host_alltoallv_fn)(void* ctx, const void* send, const uint64_t* send_bytes, void* recv, const uint64_t* recv_bytes);
int rdfgpu_comm_create_host(uint32_t rank, uint32_t world, int32_t device, rdfgpu_host_alltoallv_fn fn, void* ctx, rdfgpu_comm** out);
void rdfgpu_comm_destroy(rdfgpu_comm* comm);
int rdfgpu_exchange_allgatherv(rdfgpu_comm* comm, const uint32_t* const* cols, uint32_t n_cols, uint64_t n_rows,
                               const uint32_t** out_cols, uint64_t* out_rows);
int rdfgpu_exchange_repartition(rdfgpu_comm* comm, const uint32_t* const* cols, uint32_t n_cols, uint64_t n_rows, uint32_t key_col,
                                const uint32_t** out_cols, uint64_t* out_rows);
/* The shard of an object id among `world` ranks (host logic, no device access): the function triples are sharded by. */
uint32_t rdfgpu_shard_of(uint32_t id, uint32_t world);

/* ------------------------------------------------------------------------------------ */
/* 7. Bulk load, first half: N-Triples text -> object ids on the device                   */
/* ------------------------------------------------------------------------------------ */
/*
 * The reference parses on the host and interns the three terms of every quad through a DashMap (Store::load_from_reader /
 * bulk_loader, lib/rdf-fusion/src/store.rs:477-493 -> MemObjectIdMapping::encode_quad, lib/storage/src/memory/
 * object_id_mapping.rs:106-116).  rdfgpu_ntriples_parse does the per-triple half on the device: line and term splitting,
 * one id per DISTINCT term (first_id .. first_id + n_terms - 1; a bijection, not the reference's insertion order — no query
 * can observe the difference), and the s / p / o id columns in HBM, ready for rdfgpu_store_extend_device (graph column =
 * zeros = the default graph).  The distinct terms come back as written in the file (`<iri>`, `_:b1`, `"lex"`, `"lex"@en`,
 * `"lex"^^<dt>`: rdfgpu_ntriples_terms) and decoded + typed (rdfgpu_ntriples_decoded): the host builds its dictionary from them —
 * per distinct term, not per triple.  Text: UTF-8, one triple per line (lines end at LF; one CR before it, or before the end of the
 * text, belongs to the line end), blank lines and `#` comment lines allowed and not counted.  A malformed line is RDFGPU_ERR_INVALID
 * with its number among the counted lines (the first one, if several are).  Malformed is what the terminals of the N-Triples grammar
 * refuse: IRIREF (no byte up to 0x20 and none of < > " { } | ^ ` \ inside, but UCHAR escapes), BLANK_NODE_LABEL (a label ends at the
 * first byte that cannot belong to it, and not in `.`), LANGTAG, STRING_LITERAL_QUOTE (no raw LF or CR; ECHAR and UCHAR escapes, a UCHAR
 * names a Unicode scalar value), an IRI as predicate, `.` and an optional comment after the object; white space between tokens is
 * optional.  Not checked, and accepted: what lies behind the terminals (relative IRIs, BCP 47 subtag lengths, a UCHAR that decodes
 * to a character no IRI may hold) and whether a code point above U+007F in a blank-node label is one of PN_CHARS.  A lone CR between
 * terms is taken as white space; CR-only line ends and a leading byte-order mark are refused like any malformed line.  Two different
 * terms with one 64-bit hash (probability ~ n_terms^2 / 2^65) is RDFGPU_ERR_UNSUPPORTED — loud, never a wrong id.
 */
typedef struct rdfgpu_ntriples rdfgpu_ntriples;
int rdfgpu_ntriples_parse(int32_t device, const char* text, uint64_t text_bytes, uint32_t first_id, rdfgpu_ntriples** out);
int rdfgpu_ntriples_info(const rdfgpu_ntriples* nt, uint64_t* n_triples, uint32_t* n_terms, uint64_t* term_bytes);
/* offsets[n_terms + 1] and the terms' bytes (term t has id first_id + t); either pointer may be null */
int rdfgpu_ntriples_terms(const rdfgpu_ntriples* nt, uint64_t* offsets, uint8_t* bytes);
/*
 * The distinct terms as the reference's parser hands them to its dictionary (oxttl -> oxrdf: escapes decoded) and the typed values
 * of the literals (ABI 3).  Terms are interned by this CANONICAL form: `"a\u0041"` and `"aA"`, `"x"^^xsd:string` and `"x"`, `"v"@EN`
 * and `"v"@en` are one term with one id (rdfgpu_ntriples_terms hands out one of its spellings).  Per term t (id first_id + t):
 *   kind[t]    1 IRI, 2 blank node, 3 simple literal, 4 language-tagged literal, 5 typed literal
 *   lex        the lexical form, ECHAR / UCHAR escapes decoded to UTF-8: lex_bytes[lex_off[t] .. lex_off[t + 1])
 *   suffix     the language tag in lower case / the datatype IRI (decoded): suffix_bytes[suffix_off[t] .. suffix_off[t + 1])
 *   typed[t]   the typed-value row the device derives (encoding/typed_value.rs:27-83, lib/model/src/typed_value.rs:349-411): tag;
 *              IRIs / blank nodes / strings carry lo = 0 (their rank in `str` order is the dictionary's to give) and aux = 0 (the
 *              host numbers languages / datatypes); xsd:integer and its derived types, xsd:int, xsd:boolean, xsd:decimal (low
 *              64 bits in lo, high in dec_hi[t]: the host's decimal side table) are parsed here, an invalid lexical form gives
 *              RDFGPU_TV_NULL like the reference's Invalid; xsd:double / xsd:float are parsed when the conversion is exact in one
 *              IEEE operation (<= 15 / 7 digits, |exponent| <= 22 / 10), otherwise — and for dateTime / time / date / durations —
 *              flags carries RDFGPU_TVF_NEEDS_HOST and the tag says what to parse the lexical form as.
 * Any pointer may be null.  Sizes: rdfgpu_ntriples_decoded_info.
 */
int rdfgpu_ntriples_decoded_info(const rdfgpu_ntriples* nt, uint64_t* lex_bytes, uint64_t* suffix_bytes);
int rdfgpu_ntriples_decoded(const rdfgpu_ntriples* nt, uint8_t* kind, uint64_t* lex_off, uint8_t* lex_bytes, uint64_t* suffix_off,
                            uint8_t* suffix_bytes, rdfgpu_typed_value* typed, int64_t* dec_hi);
/* device pointers of the id columns (n_triples each, file order); valid until rdfgpu_ntriples_destroy */
int rdfgpu_ntriples_columns(const rdfgpu_ntriples* nt, const uint32_t** s, const uint32_t** p, const uint32_t** o);
void rdfgpu_ntriples_destroy(rdfgpu_ntriples* nt);

#ifdef __cplusplus
}
#endif
#endif /* RDFGPU_H */
