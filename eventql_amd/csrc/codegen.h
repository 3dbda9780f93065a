// codegen.h -- plan analysis and HIP source generation for the fused
// scan -> filter -> GROUP BY kernel ("csql::VM bytecode lowered to fused HIP
// kernels", BASELINE.json north_star).
#pragma once
#include <string>
#include <vector>
#include "cstable_format.h"
#include "plan_ir.h"

namespace evql {

// how the fused kernel reads one scan column
struct ColAccess {
  // NARROW: the table's flat narrow copy of a LEB128 / PLAIN integer column (bits = 8 / 16 / 32)
  // NARROW_F32: the table's flat float32 copy of a FLOAT_IEEE754 column whose values are all
  // exactly float32 (bits = 32, packed); widened back to the file's 64 bits by the accessor.
  // Only the tile loops read it: row-addressed readers (RtColumn) keep the file's pages.
  enum Mode { PLAIN64 = 0, PLAIN32 = 1, BITPACKED = 2, SOA = 3, NARROW = 4, NARROW_F32 = 5 };
  std::string name;
  uint32_t stype = EVQL_T_NIL;  // evql_stype seen by the VM
  Mode mode = PLAIN64;
  uint32_t bits = 0;          // BITPACKED / NARROW width
  bool has_tags = false;      // SOA with a tag byte array (nullable column)
  bool bool_normalize = false;  // BOOLEAN column: value = (raw > 0)
  bool from_uint_to_float = false;  // FLOAT64 stype over a uint column: (double) u
  bool string_hash = false;   // STRING column materialised as hash64
  bool string_bytes = false;  // ... and compared bytewise on the device (strpos array)
  bool packed = false;        // NARROW / NARROW_F32: read from the copy, not from the file's pages
  bool dict_code = false;     // PLAIN32 over the table's dictionary codes of a STRING column
  int layout_index = -1;      // index into TableLayout::columns
};

// one 8-byte aggregate state word
struct StateWord {
  int op;  // EVQL_OP_* (evql_device.h)
};

struct AggPlan {
  uint32_t fn = EVQL_AGG_NONE;
  ExprPtr arg;         // over scan columns; null for count
  int first_word = 0;  // index into state words
  int nwords = 0;
  // count_distinct: index of the (group, value) pair set in EvqlArgs::pairset; the
  // state word counts the pairs this aggregate inserted first
  int distinct_index = -1;
  // EVQL_FLOAT_SUM_EXACT: the sum is kept as two integer words (high part, low 31
  // bits) of multiples of a quantum; index into EvqlArgs::fscale / fbound
  int exact_index = -1;
  // partitioned path: the argument is an unsigned value known to stay below 2^32 - 1
  // (column statistics, value_bounds.cc choose_tuple_widths); it travels as 32 bits
  bool narrow_arg = false;
};

static const int kMaxExactSums = 4;

static const int kMaxDistinct = 4;

// slots of the numeric literal pool in the kernel arguments (EvqlArgs::lit, EVQL_MAX_LITS)
static const int kMaxLits = 32;

// Zone maps: rows per zone, aligned to row 0.  A kernel tile is
// block * 2 * unroll rows (block 256 or 1024, unroll a power of two): a whole number of
// zones, or a divisor of one.
static const uint64_t kZoneRows = 2048;
static const int kMaxZoneConjuncts = 4;

// a top-level conjunct `column <op> literal` of WHERE that can exclude zones
struct ZoneConjunct {
  int col = -1;       // scan column (index into KernelPlan::cols)
  uint32_t op = 0;    // ZoneOp (aot_kernels.h), as seen from the column side
  uint64_t lit = 0;   // the literal; data of k_zone_select, never part of the kernel text
};

enum KeyMode {
  KEY_NONE = 0,    // no GROUP BY: one global group, register accumulators
  KEY_EXACT = 1,   // one fixed-width key: identity = value bits (+ NULL slot)
  KEY_HASHED = 2   // several keys / string keys: identity = 64-bit tuple hash
};

struct KernelPlan {
  std::vector<ColAccess> cols;
  ExprPtr where;                // over scan columns, may be null
  std::vector<ExprPtr> group;   // over scan columns
  std::vector<AggPlan> aggs;    // one per aggregate select expression
  std::vector<StateWord> states;
  KeyMode key_mode = KEY_NONE;
  bool need_first_row = false;
  bool has_row_filter = false;
  int n_distinct = 0;  // count_distinct aggregates (one HBM pair set each)
  int n_exact = 0;     // exact float sums
  // slot layout: word 0 identity, [second identity word], [first_row], states.
  // Hashed keys (several keys / strings) are identified by TWO independent
  // 64-bit hashes of the key tuple -- like the reference, which identifies a
  // group by a hash of its tuple bytes (SHA1, groupby.cc:129-135).
  bool has_ident2() const { return key_mode == KEY_HASHED; }
  int first_row_word() const { return 1 + (has_ident2() ? 1 : 0); }
  int words_per_slot() const { return state_word_base() + int(states.size()); }
  int state_word_base() const { return first_row_word() + (need_first_row ? 1 : 0); }
  // launch shape
  int block = 256;
  int unroll = 4;
  int lds_slots = 0;  // 0 => aggregate straight into the HBM table
  // entries of the lane-private accumulator cache in front of the LDS table (1, or 4 for
  // plans with 2 .. 4 expected groups), codegen_kernels.inc evql_update
  int lane_cache = 1;
  // evql_scan_agg loads the next tile, raw, while it evaluates the current one (DESIGN.md 3.1,
  // codegen_kernels.inc scan_kernel).  Chosen by choose_launch_shape where `prefetch_allowed`:
  // false for nested scans, under EVQL_SCAN_PREFETCH=0 (build_kernel_plan), and once the
  // prefetching kernel of the plan has compiled with scratch memory (compile_plan_kernels).
  bool prefetch = false;
  bool prefetch_allowed = false;
  // The staging form of the prefetching loop (codegen_kernels.inc stage_step):
  // every row runs WHERE only and the passing rows leave what the group key and the aggregate
  // arguments read (stage_tuple_layout) in a ring of the wave in LDS; the group table is
  // updated once per 64 staged rows, with a full exec mask.  Chosen by choose_launch_shape
  // among the prefetching plans where `stage_allowed`: false under EVQL_SCAN_STAGE=0
  // (build_kernel_plan) and once the staging kernel has compiled with scratch memory.
  bool stage = false;
  bool stage_allowed = false;
  // high cardinality: radix-partition the passing rows into 2^part_bits buckets
  // of tuples, then aggregate each bucket in LDS (codegen_kernels.inc)
  bool partitioned = false;
  int part_bits = 12;
  // two-level partitioning without the count pass: tuples go into slack-allocated coarse
  // buckets (capacity EvqlPartArgs::coarse_cap each), the fine-bucket sizes are counted
  // while they are scattered; false = exact offsets from evql_part_count first
  bool part_fused = false;
  // partition tuples are arrays of 32-bit words: the identity of a single unsigned key
  // and the first-row index travel as 32 bits where the table's statistics bound them
  bool narrow_ident = false;
  bool narrow_first_row = false;
  // nested scans whose WHERE reads columns of different repetition depth: an extra
  // kernel (evql_where_rows) writes the predicate of every row, from which the runtime
  // reproduces the reference's reset of parent values behind a rejected row
  bool where_rows_kernel = false;
  // bare scan (neither GROUP BY nor aggregates): the values of `scan_out` -- the scan
  // select list over scan columns -- leave the device for every passing row, in row order
  // (codegen_kernels.inc bare_scan_kernels: evql_scan_count / evql_scan_emit)
  bool bare_scan = false;
  std::vector<ExprPtr> scan_out;
  std::vector<bool> scan_out_nullable;  // may the value carry STAG_NULL?
  // The 64-bit values of the plan's pooled numeric literals, in the order the generator met
  // them (codegen.cc, case Expr::LITERAL): the text reads slot i as A.lit[i], every launch
  // passes the values (fill_host_args).  Filled by generate_kernel_source; NOT part of the
  // text, so plans that differ only here share one code object.
  std::vector<uint64_t> lit_pool;
  // The conjuncts of WHERE that prune zones (planner.cc zone_conjuncts_of).  Non-empty: the
  // tile loops test EvqlArgs::tile_skip.  Whether a conjunct is listed depends on the plan's
  // shape only, never on the literal's value.
  std::vector<ZoneConjunct> zone_conjuncts;
  int tile_rows() const { return block * 2 * unroll; }
};

// One field of a staged tuple: scan column `col` as the bits of its copy (8-bit values take a
// 16-bit field), at bit `shift` of 32-bit word `word`.
struct StageField {
  int col = -1;
  int bits = 0;
  bool f32 = false;  // the raw word of a float32 copy, widened again behind the ring
  int word = 0;
  int shift = 0;
};
// Entries of a wave's staging ring: at most 63 tuples are pending when a row is staged, and
// a row adds at most 64.
static const int kStageRing = 128;
// LDS bytes a workgroup may have (gfx950)
static const uint64_t kLdsBytes = 160 * 1024;
// The tuple of a staging plan: the columns the group key and the aggregate arguments read, by
// column index, two fields of <= 16 bits to a word first, the 32-bit fields behind them.
// Returns its 32-bit words.
int stage_tuple_layout(const KernelPlan& kp, std::vector<StageField>* fields);

// launch shape for `hint` expected groups (planner.cc)
void choose_launch_shape(KernelPlan* kp, uint64_t hint);
uint64_t lds_table_max_slots(const KernelPlan& kp);
extern const uint64_t kPartitionAboveSlots;  // partitioned path for hint > this * LDS slots
bool partitioned_path_possible(const KernelPlan& kp);

// does evaluating `e` print a zero-divisor check anywhere (an integer div / mod whose divisor
// is not a non-zero literal)?  Such an expression can raise; the emitter's own condition.
bool expr_prints_zero_check(const ExprPtr& e);

// the generated translation unit (device library excluded); fills kp->lit_pool
std::string generate_kernel_source(KernelPlan* kp);
// 32-bit words of one partition tuple (identity, [identity 2], [row], update words)
int partition_tuple_u32_words(const KernelPlan& kp);

// the embedded text of evql_device.h
const char* device_library_source();

}  // namespace evql
