// runtime.h -- device context, HBM-resident tables and query objects behind the
// C ABI (include/evql_gpu.h).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>
#include <algorithm>
#include <functional>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <vector>
#include "aot_kernels.h"
#include "codegen.h"
#include "cstable_format.h"
#include "materialize_plan.h"
#include "order_sort_plan.h"
#include "plan_ir.h"

namespace evql {

// host mirror of the device-side EvqlArgs / EvqlColArg (evql_device.h)
struct HostColArg {
  const uint64_t* pages;
  const uint64_t* soa;
  const uint8_t* tags;
  uint64_t npages;
  const uint64_t* strpos;
  const uint8_t* base;
};
static const uint32_t EVQL_MAX_COLS_HOST = 16;
struct HostArgs {
  const uint8_t* image;
  uint64_t row_begin, row_end, ntiles, tile0;
  const uint8_t* row_filter;
  uint64_t row_filter_len;
  uint64_t* gtab;
  uint64_t gcap;
  uint32_t* status;
  uint64_t* counters;
  const uint32_t* tile_skip;  // evql_query::tile_skip
  HostColArg col[16];
  uint64_t* pairset[4];
  uint64_t pairset_cap[4];
  double fscale[4];
  double fbound[4];
  uint64_t lit[kMaxLits];  // KernelPlan::lit_pool
};

struct Status {
  int code = EVQL_OK;
  std::string msg;
  bool ok() const { return code == EVQL_OK; }
  static Status error(int c, const std::string& m) {
    Status s;
    s.code = c;
    s.msg = m;
    return s;
  }
};

struct Module {
  hipModule_t mod = nullptr;
  hipFunction_t fn = nullptr;
  // partitioned high-cardinality path (present only when the plan asks for it)
  hipFunction_t fn_count = nullptr, fn_scatter = nullptr, fn_aggregate = nullptr;
  hipFunction_t fn_refine = nullptr;  // second scatter level (part_bits > 8)
  hipFunction_t fn_where = nullptr;   // evql_where_rows (nested scans, mixed-depth WHERE)
  // bare scans (KernelPlan::bare_scan): instead of `fn`
  hipFunction_t fn_scan_count = nullptr, fn_scan_emit = nullptr;
  size_t code_size = 0;
};

// host mirror of the generated EvqlPartArgs
struct HostPartArgs {
  uint64_t tiles_per_wg;
  uint32_t* counts;
  const uint64_t* bucket_start;
  uint64_t* tuples;
  uint64_t nwg;
  uint64_t* tuples_tmp;
  uint32_t* cursors;
  uint64_t* dense;
  uint64_t dense_cap;
  uint64_t coarse_cap;  // tuples per coarse bucket of tuples_tmp (KernelPlan::part_fused)
};
struct HostArgsWithPart {
  HostArgs a;
  HostPartArgs p;
};
// 992 bytes of pointers and bounds + the 256 bytes of the literal pool; with the largest
// trailing struct a launch stays far below the 4 KiB kernel-argument segment
static_assert(sizeof(HostArgs) == 1248, "device side: EvqlArgs (evql_device.h)");
static_assert(sizeof(HostArgsWithPart) == 1328 && sizeof(HostArgsWithPart) <= 4096,
              "kernel-argument segment");

// what the kernel cache did (evql_ctx_kernel_cache_stats)
struct KernelCacheStats {
  uint64_t memory_hits = 0, disk_hits = 0, compiles = 0;
  double compile_ms = 0;
};

// Pinned host blocks of one size that the device stores to (the eager step tail,
// query_run.cc): taken by an operator on first use, handed back when it closes -- an
// operator per step (config 5w) then pays no hipHostMalloc.  Shared by the context and the
// operators that hold a block, so that it outlives whichever is destroyed first.
static const size_t kTailBlockBytes = 256 << 10;
struct PinnedPool {
  std::vector<void*> free_blocks;
  PinnedPool() = default;
  PinnedPool(const PinnedPool&) = delete;
  PinnedPool& operator=(const PinnedPool&) = delete;
  ~PinnedPool() {
    for (void* p : free_blocks) hipHostFree(p);
  }
  hipError_t take(void** out) {
    if (!free_blocks.empty()) {
      *out = free_blocks.back();
      free_blocks.pop_back();
      return hipSuccess;
    }
    return hipHostMalloc(out, kTailBlockBytes, hipHostMallocDefault);
  }
  void give(void* p) { free_blocks.push_back(p); }
};

}  // namespace evql

struct evql_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int num_cus = 256;
  std::map<std::string, evql::Module> modules;  // by source fingerprint
  evql::KernelCacheStats kstats;
  std::shared_ptr<evql::PinnedPool> pinned = std::make_shared<evql::PinnedPool>();
};

namespace evql {
// owning device pointer (move-only): freed on every exit path (HIP_TRY returns early on
// errors), or with the cache entry that holds it
template <typename T>
struct DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.release()) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p = o.release();
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  hipError_t alloc(size_t bytes) {
    reset();
    return hipMalloc(reinterpret_cast<void**>(&p), bytes ? bytes : 1);
  }
  void reset() {
    if (p) hipFree(p);
    p = nullptr;
  }
  T* release() {
    T* r = p;
    p = nullptr;
    return r;
  }
  operator T*() const { return p; }
};
}  // namespace evql

// a decoded-to-SoA column cached on the table (owns its device arrays)
struct MaterializedColumn {
  uint64_t* d_values = nullptr;
  uint8_t* d_tags = nullptr;
  // a required UINT64_LEB128 or UINT64_PLAIN column (table.cc materialize_column /
  // narrow_plain_column) kept as a flat array of 8 / 16 / 32 bits per value (the narrowest
  // that holds the column's maximum; layout: narrow_copy_bytes below): the fused kernel
  // then reads 1 - 4 bytes per value instead of an 8-byte SoA word
  uint8_t* d_packed = nullptr;
  uint32_t packed_bits = 0;
  // d_packed holds float32 bits, not unsigned integers: the copy of a required FLOAT_IEEE754
  // column whose values are all exactly float32 (table.cc narrow_float_column, packed_bits =
  // 32).  Only the fused kernels' tile loads read it (evql_f32_x2); integer readers of
  // packed_bits (evql_narrow_rt) must skip such an entry.
  bool packed_f32 = false;
  bool string_hash = false;
  // strings: (len << 40) | byte position of the value in the column's page stream,
  // per row (bytewise compares in the fused kernel, result emission)
  uint64_t* d_strpos = nullptr;

  MaterializedColumn() = default;
  MaterializedColumn(const MaterializedColumn&) = delete;
  MaterializedColumn& operator=(const MaterializedColumn&) = delete;
  MaterializedColumn(MaterializedColumn&& o) noexcept { *this = std::move(o); }
  MaterializedColumn& operator=(MaterializedColumn&& o) noexcept {
    std::swap(d_values, o.d_values);
    std::swap(d_tags, o.d_tags);
    std::swap(d_strpos, o.d_strpos);
    std::swap(string_hash, o.string_hash);
    std::swap(d_packed, o.d_packed);
    std::swap(packed_bits, o.packed_bits);
    std::swap(packed_f32, o.packed_f32);
    return *this;
  }
  ~MaterializedColumn() {
    if (d_values) hipFree(d_values);
    if (d_tags) hipFree(d_tags);
    if (d_strpos) hipFree(d_strpos);
    if (d_packed) hipFree(d_packed);
  }
};

// Dictionary of a STRING column: one dense 32-bit code per distinct value, EXACT (equal
// codes <=> equal bytes, verified when it is built, string_dict.cc).  A GROUP BY over the
// column then runs on the codes -- a 4-byte exact key instead of 64-bit hashes plus a row
// index -- and its group records are translated back (code -> hashed identity + first
// row) only where they leave the operator.
struct StringDict {
  bool tried = false;
  bool usable = false;
  uint64_t n_codes = 0;
  uint32_t* d_codes = nullptr;       // per row, padded like the other column buffers
  uint64_t* d_code_pages = nullptr;  // "page" offsets into d_codes (131,072 codes each)
  uint64_t* d_entries = nullptr;     // [n_codes][3]: string hash, first row, bit0 NULL
  std::string why;                   // when not usable
  StringDict() = default;
  StringDict(const StringDict&) = delete;
  StringDict& operator=(const StringDict&) = delete;
  ~StringDict() {
    if (d_codes) hipFree(d_codes);
    if (d_code_pages) hipFree(d_code_pages);
    if (d_entries) hipFree(d_entries);
  }
};

struct evql_table {
  evql_ctx* ctx = nullptr;
  evql::TableLayout layout;
  uint8_t* d_image = nullptr;
  uint64_t image_len = 0;
  // device page tables: [column][0 data, 1 rlevel, 2 dlevel]
  std::vector<std::vector<uint64_t*>> d_pages;
  std::vector<uint64_t> payload_bytes;
  std::map<std::string, MaterializedColumn> materialized;
  std::map<std::string, StringDict> dicts;  // by column name
  // maximum |value| per column ("name#f" float view, "name#u" integer view): bounds of
  // exact float sums (EVQL_FLOAT_SUM_EXACT)
  std::map<std::string, double> col_absmax;
  // zone maps: unsigned minimum and maximum of every kZoneRows rows of a
  // required unsigned / datetime column, built by the first query that prunes on it
  // (16 B per 2048 rows; left out of evql_table_device_bytes)
  struct ZoneMap {
    evql::DevBuf<uint64_t> zmin, zmax;
    uint64_t n_zones = 0;
  };
  std::map<std::string, ZoneMap> zone_maps;
  // required UINT64_PLAIN columns are kept narrow from this many rows on (~0 = never)
  uint64_t narrow_min_rows;
  // required FLOAT_IEEE754 columns are tried as float32 copies from this many rows on (~0 =
  // never); the columns a pass refused (some value is not exactly float32), so that no
  // later operator repeats it; and the passes run so far
  uint64_t narrow_float_min_rows;
  std::set<std::string> narrow_float_refused;
  uint64_t narrow_float_passes = 0;
  // nested scans: column flattened to one value per output row of the scans whose
  // deepest repeated column is `leaf` -- key (column, leaf) layout indices.  Like
  // `materialized`, decoded once per table and shared by every operator.
  struct NestedFlat {
    evql::DevBuf<uint64_t> d_values;  // per row: value bits; strings: (len << 40 | position)
    uint64_t nflat = 0;
    evql::DevBuf<uint64_t> d_hash;    // strings: 64-bit hash of the row's bytes
    // the values once more as a flat array of 8 / 16 / 32 bits each (when their maximum
    // fits): what the fused kernel streams instead of the 8-byte words
    evql::DevBuf<uint8_t> d_packed;
    uint32_t packed_bits = 0;
    bool pack_tried = false;
  };
  std::map<std::pair<int, int>, NestedFlat> nested_cache;
  // record scans (WITHIN RECORD): the leaf's decoded repetition levels (one byte
  // per slot) and the scanned per-tile counts of its level-0 slots (= records
  // started before the tile), keyed by the leaf's layout index.  An entry outlives
  // every query on the table: operators hold pointers to it.
  struct LeafLevels {
    evql::DevBuf<uint8_t> levels;
    evql::DevBuf<uint64_t> rec_offsets;
  };
  std::map<int, LeafLevels> leaf_cache;
  evql_table();
  ~evql_table();
};

struct evql_query {
  evql_ctx* ctx = nullptr;
  evql_table* table = nullptr;
  // plan
  std::vector<evql::LoweredProgram> scan_select, group, select;
  evql::LoweredProgram where;
  bool has_where = false;
  evql::KernelPlan kp;
  // Dictionary-coded string key (StringDict): `kp` is then the plan the kernels run --
  // KEY_EXACT over the code column -- and `rkp` the plan its group RECORDS follow once
  // they leave the scan (hashed string key + first row: what the plan is without a
  // dictionary).  Emission, ORDER BY, the exchange and chain merges read rplan().
  bool dict_key = false;
  int dict_candidate = -1;  // scan column a dictionary could code (planner), or -1
  evql::KernelPlan rkp;
  const evql::KernelPlan& rplan() const { return dict_key ? rkp : kp; }
  uint64_t* d_conv = nullptr;  // the groups as records of rplan()'s layout
  uint64_t conv_cap = 0;       // records
  bool conv_valid = false;
  std::vector<int> select_agg_index;  // select expr -> index into kp.aggs or -1
  std::vector<bool> select_passthrough;
  uint32_t group_mode = EVQL_MODE_FINAL;
  uint64_t groups_hint = 0;
  // EVQL_FLOAT_SUM_EXACT: quantum exponent / bound per exact sum (index AggPlan::exact_index)
  uint32_t float_sum_mode = 0;
  double float_sum_bound = 0;
  int fsum_exp[4] = {0, 0, 0, 0};   // quantum = 2^fsum_exp
  double fsum_bound[4] = {0, 0, 0, 0};
  uint64_t row_begin = 0, row_end = 0;
  std::vector<uint8_t> row_filter_host;
  uint64_t row_filter_len = 0;
  uint8_t* d_row_filter = nullptr;
  bool row_filter_owned = true;  // false: the bits belong to an evql_lsm_chain
  // nested scans: one bit per record on entry; query_prepare replaces it by its expansion to
  // one bit per flattened row where the two differ (nested.cc expand_record_filter)
  uint64_t reported_rows_scanned = ~0ull;  // != ~0: the reference's count, where it is not the row range
  // evql_query_create_chain: this query scans the first table of a partition's chain;
  // `chain` holds the queries of the tables behind it (owned).  After execute their
  // groups are merged in chain order into d_mtab (chain_merge.cc).
  std::vector<evql_query*> chain;
  // partitioned path buffers
  uint32_t* d_part_counts = nullptr;
  uint64_t* d_bucket_start = nullptr;
  uint64_t* d_tuples = nullptr;
  uint64_t* d_tuples_tmp = nullptr;  // coarse-bucket order (two-level scatter)
  uint32_t* d_part_cursors = nullptr;
  uint64_t tuples_cap = 0;  // in tuples
  uint64_t tuples_tmp_cap = 0;  // in tuples
  bool part_fused_off = false;  // a coarse bucket overflowed its slack once: exact offsets from now on
  // partitioned path: the groups of every bucket that fitted its LDS table, as dense
  // records [kind, identity, (identity 2), (first row), states...]; the HBM table
  // then only holds the groups of overflowed buckets
  uint64_t* d_dense = nullptr;
  uint64_t dense_cap = 0;  // records
  uint64_t dense_n = 0;
  // after evql_query_exchange: the merged groups of all ranks (or of this rank's key
  // range) in a table of their own, whose slots also carry the first-row value words
  // of plans that need them (exchange.cc); results are then emitted from here
  bool merged = false;
  uint64_t* d_mtab = nullptr;
  uint64_t mcap = 0;
  uint32_t m_words = 0;
  std::vector<uint8_t> m_heap;  // received string bytes
  // `merged` by chain_merge and not (yet) by an exchange: d_mtab holds this partition's own
  // groups, which evql_query_exchange takes as its source (instead of d_gtab); the string
  // words of its slots point into m_heap, kept once more on the device for that export
  bool chain_merged = false;
  evql::DevBuf<uint8_t> d_mheap;
  uint64_t mheap_cap = 0;  // bytes allocated; m_heap.size() of them are filled
  // large merges (exchange.cc bucketed_merge) leave dense records [kind, slot words...]
  // instead of a table
  bool merged_dense = false;
  uint64_t* d_mdense = nullptr;
  uint64_t mdense_cap = 0;  // records
  uint64_t mdense_n = 0;
  int n_update_words = 0;   // update words per row (tuple payload)
  // nested (Dremel) scans: flattened per-row SoA columns, one per scan column
  bool nested = false;
  uint64_t nested_rows = 0;
  std::vector<uint64_t*> nested_flat;
  std::vector<uint64_t*> nested_strpos;  // string columns: (len << 40 | position) per row
  // nested scans over flat narrow copies of the flattened columns (ColAccess::packed)
  struct PackedSource {
    const uint8_t* base = nullptr;
  };
  std::vector<PackedSource> nested_packed;
  int nested_leaf = -1;  // layout index of the leaf column of the scan
  std::vector<uint64_t*> nested_owned;
  bool nested_where_mixed = false;  // WHERE over columns of different repetition depth
  bool nested_siblings = false;     // columns of sibling repeated groups: zipped (materialize_nested_zip)
  // EVQL_SCAN_NESTED_WITHIN_RECORD (CSTableScan.cc:440-487,
  // AGGREGATE_WITHIN_RECORD_FLAT): the scan select list holds one aggregate per
  // expression, reduced to one value per record; those per-record arrays are
  // the `kp.cols` the operators above the scan read.
  struct WithinAgg {
    bool is_count = false;
    int col = -1;        // index into wr_cols, or -1: literal / no argument
    uint64_t lit = 0;
    uint32_t level = 0;  // select_list_[i].rep_level
  };
  bool within_record = false;
  double within_record_ms = 0;  // device time of k_within_record (part of this operator's work)
  std::vector<evql::ColAccess> wr_cols;  // the columns the record scan reads
  std::vector<WithinAgg> wr_aggs;
  std::string source;
  evql::Module module;
  // execution state
  uint64_t* d_gtab = nullptr;
  uint64_t gcap = 0;
  uint32_t* d_status = nullptr;
  uint64_t* d_counters = nullptr;
  uint64_t* d_small_rec = nullptr;  // 1 MiB: dense records of small results
  // The eager step tail (query_run.cc eager_tail_records): behind the scan one
  // epilogue kernel leaves status words, counters, group count and -- for small results --
  // the group records themselves in a pinned host block; finish waits once and reads it,
  // next_batch packs from it without touching the device.
  enum EagerTail { EAGER_OFF = 0, EAGER_RECORDS = 1, EAGER_ON = 2 };
  int eager_tail = EAGER_ON;    // EVQL_EAGER_TAIL, read when the operator is created
  bool in_chain = false;        // one table of a partition's file chain (merged by chain_merge)
  std::shared_ptr<evql::PinnedPool> tail_pool;  // where h_tail came from and goes back to
  uint64_t* h_tail = nullptr;   // the block (host address)
  uint64_t* d_tail = nullptr;   // the block as the device addresses it
  uint64_t tail_seq = 0;        // stamp of the last epilogue enqueued
  uint32_t tail_armed = 0;      // records the enqueued epilogue may write (0: lazy tail enqueued)
  bool tail_valid = false;      // the block holds ALL groups of the table as finish saw it
  // count_distinct pair sets (3 word planes of pairset_cap slots each)
  uint64_t* d_pairset[4] = {nullptr, nullptr, nullptr, nullptr};
  uint64_t pairset_cap = 0;
  // after an exchange / chain merge: the merged pair sets (the union of the ranks' /
  // tables' sets for the groups this query now holds); PARTIAL rows read their values here
  uint64_t* d_mset[4] = {nullptr, nullptr, nullptr, nullptr};
  uint64_t mset_cap[4] = {0, 0, 0, 0};
  // zone maps: the bitmap of excluded zones of this query's pruning conjuncts, built once by
  // query_prepare; `tile_skip` is what the kernels get: NULL when no zone is excluded
  evql::DevBuf<uint32_t> d_zone_bits;
  const uint32_t* tile_skip = nullptr;
  evql_zone_stats_t zstats{};
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool probed = false;    // cardinality probe done (plans without groups_hint)
  bool keep_table = false;  // launch without emptying the group table / counters (the
                            // cardinality probe aggregates several row ranges into one)
  // heartbeat of the running evql_query_execute: also beaten between the launches of the
  // cardinality probe and between the re-runs after a full table
  int (*hb)(void*) = nullptr;
  void* hb_user = nullptr;
  bool hb_abort = false;
  bool launched = false;
  bool executed = false;
  bool fetched = false;  // groups copied to the host (lazy, on first nextBatch)
  int grid = 0;
  // results
  std::vector<uint64_t> records;  // dense [kind, ident, (first_row), states...]
  size_t rec_stride = 0;          // words per fetched record (>= words_per_slot + 1)
  uint64_t ngroups = 0;
  std::vector<uint64_t> first_vals;  // [col][group]
  std::vector<uint8_t> first_tags;
  std::vector<uint8_t> first_str_heap;  // bytes of the first-row strings
  std::vector<uint64_t> first_str_off;  // [col][group] offset into the heap
  uint64_t emit_pos = 0;
  std::vector<std::vector<uint8_t>> out_cols;
  // large results packed on the device (results.cc emit_on_device): every output column
  // of ALL groups as SVector bytes in pinned host memory, next_batch hands out slices
  struct DeviceEmit {
    bool active = false;
    std::vector<uint8_t*> col;      // pinned (hipHostMalloc), per select expression
    std::vector<size_t> col_cap;
    std::vector<uint32_t> elem;     // bytes per element; 0 = STRING
    std::vector<uint64_t*> off;     // strings: pinned [n + 1] byte offsets
    std::vector<size_t> off_cap;
  } demit;
  // EVQL_MODE_PARTIAL rows of large results take the same way: column 0 the keys (25 bytes
  // each), column 1 the saved states (results.cc emit_partial_on_device)
  bool partial_device_emit = true;  // EVQL_PARTIAL_DEVICE_EMIT, read when the operator is created
  evql_emit_stats_t estats{};       // how the last fetched result left the device
  // EVQL_MODE_PARTIAL with count_distinct: the distinct values of every group, per
  // aggregate, read back from the HBM pair set; key = (identity, identity 2 | NULL flag)
  std::vector<std::map<std::pair<uint64_t, uint64_t>, std::vector<uint64_t>>> distinct_values;
  // Bare scans (kp.bare_scan, bare_scan.cc).  execute counts the passing rows of every
  // tile; next_batch emits and packs one WINDOW of consecutive tiles at a time -- the result
  // can be as large as the table and is never held whole -- into demit's pinned columns and
  // hands out slices of it.
  struct BareScan {
    uint64_t window_rows = 0;         // most passing rows of one window (>= one tile)
    uint64_t ntiles = 0;
    evql::DevBuf<uint32_t> d_tile_count;
    evql::DevBuf<uint64_t> d_tile_off;  // [ntiles + 1] exclusive scan of the counts
    uint64_t tiles_cap = 0;
    bool counted_on_device = false;
    std::vector<uint64_t> tile_off;   // host copy
    // passing rows are numbered in row order; [lo, hi) of them are the result (LIMIT / OFFSET)
    uint64_t lo = 0, hi = 0, pos = 0;  // pos: the next row next_batch hands out
    uint64_t win_base = 0, win_rows = 0;  // rows [win_base, win_base + win_rows) are staged
    evql::DevBuf<uint64_t> d_words;   // [column][win_rows] value words of the window
    evql::DevBuf<uint8_t> d_tags;
    uint64_t stage_cap = 0;           // elements d_words / d_tags hold
    double emit_ms = 0;               // device time of the window kernels so far
    // the heartbeat of the last evql_query_execute: the window kernels of next_batch beat
    // it too (a scan's device work continues behind execute)
    int (*hb)(void*) = nullptr;
    void* hb_user = nullptr;
    uint64_t windows = 0;
  } bare;
  // ORDER BY .. LIMIT fused above the GROUP BY (evql_query_set_order)
  std::vector<evql::LoweredProgram> order;  // over the select list
  std::vector<bool> order_desc;
  bool has_limit = false;
  uint64_t limit = 0, offset = 0;
  evql::OrderKeyArgs order_key{};     // where the device finds sort key 0 in a record
  std::vector<uint64_t> emit_order;  // record indices in output order (when ordered)
  // ORDER BY over a large result sorted on the device (results.cc sort_on_device)
  bool order_device_sort = true;  // EVQL_ORDER_DEVICE_SORT, read when the operator is created
  bool order_applied = false;     // the fetched records are the ordered OFFSET / LIMIT slice:
                                  // order_fetched does not run; cleared wherever `fetched` is
  evql_order_stats_t ostats{};    // how the last fetched result was ordered
  evql_query_stats_t stats{};
  ~evql_query();
};

struct evql_writer {
  std::unique_ptr<evql::TableWriter> w;
  std::vector<evql::ColumnSpec> specs;
};

#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      return Status::error(EVQL_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    }                                                                                        \
  } while (0)

namespace evql {
// capi.cc: the calling thread's last error
void set_last_error(const std::string& m);
int fail(int code, const std::string& m);

// kernel_cache.cc
void set_cache_dir(const std::string& d);
// `stats`: the counters to bump; NULL = the process-wide ones (evql_compile_only)
Status compile_to_code_object(const std::string& source, std::vector<char>* code, bool use_cache,
                              KernelCacheStats* stats = nullptr);
KernelCacheStats process_kernel_cache_stats();
Status compile_kernel(evql_ctx* ctx, const std::string& source, Module* out,
                      bool load_module);
Status build_kernel_plan(const TableLayout& layout, const evql_plan_desc_t* plan,
                         evql_query* q, bool* unsupported);
// row-addressable device view of a flat column (direct pages or cached SoA decode)
Status table_rt_column(evql_table* t, const std::string& name, RtColumn* out,
                       const uint64_t** strpos);
// device copies of the page offset lists of `t->layout` -> t->d_pages
Status upload_page_tables(evql_table* t);
// string_dict.cc: the (cached) dictionary of STRING column `li`; built on first use
Status table_string_dict(evql_table* t, int li, StringDict** out);

// table.cc
Status table_from_image(evql_ctx* ctx, const void* image, size_t len, bool keep_host,
                        evql_table** out);
inline uint64_t padded_rows(uint64_t n) {
  const uint64_t pad = 8192;  // largest tile
  return (n + pad - 1) / pad * pad + pad;
}
// bit width of a bit-packed stream: bitpack_width of the 4-byte header of its first page
Status stream_bits(evql_table* t, const std::vector<PageRef>& pages, uint32_t* bits);
// Where the `nvalues` defined values of column `li` are read from: its data pages as they lie
// (PLAIN64 / PLAIN32 / BITPACKED with its width), or SOA over a buffer decoded (LEB128) or
// located (STRING_PLAIN: (len << 40) | position) here.  That buffer is `dst` when the caller
// has one for LEB128 values, else it is allocated into `*owned`.
Status defined_value_source(evql_table* t, int li, uint64_t nvalues, uint64_t* dst, RtColumn* src,
                            DevBuf<uint64_t>* owned);
// A narrow copy (ColAccess::NARROW) of `n` values of `bits` = 8 / 16 / 32 bits is one
// allocation: the little-endian values in row order from byte 0 (256-byte aligned, as the
// allocator hands it out), zeros up to a whole number of kNarrowUnit values and through
// kNarrowSlack bytes more, then the 4-byte maximum a value of that width can take.  A tile
// of the fused kernels (at most 16384 rows, whole tiles from row 0) reads at most 64 KiB
// behind the last row: zeros, inside the allocation, whatever `n`.
static const uint64_t kNarrowUnit = 131072;
static const uint64_t kNarrowSlack = 1ull << 20;
inline uint64_t narrow_copy_max_word_at(uint64_t n, uint32_t bits) {
  const uint64_t units = std::max<uint64_t>((n + kNarrowUnit - 1) / kNarrowUnit, 1);
  return units * kNarrowUnit * (bits / 8) + kNarrowSlack;
}
inline uint64_t narrow_copy_bytes(uint64_t n, uint32_t bits) {
  return narrow_copy_max_word_at(n, bits) + 256;
}
Status pack_narrow(hipStream_t s, const uint64_t* d_values, uint64_t n, DevBuf<uint8_t>* d_packed,
                   uint32_t* bits_out);
// Required UINT64_PLAIN columns kept narrow: in tables of at least
// kNarrowMinRows rows (EVQL_NARROW_PLAIN overrides, read when a table becomes resident)
static const uint64_t kNarrowMinRows = 1ull << 26;
uint64_t narrow_plain_min_rows();
Status narrow_plain_column(evql_table* t, int li, uint64_t maxv);
// Required FLOAT_IEEE754 columns kept once more as float32 where every value
// is exactly a float32 zero, normal, infinity or quiet NaN: in tables of at least
// kNarrowMinRows rows (EVQL_NARROW_FLOAT overrides; EVQL_NARROW_PLAIN=0 turns it off too).
uint64_t narrow_float_min_rows();
Status narrow_float_column(evql_table* t, int li);
Status materialize_column(evql_table* t, const ColAccess& ca);

// nested.cc: the scans of a nested query, run by query_prepare
using LeafLevels = evql_table::LeafLevels;
Status materialize_nested(evql_query* q, const std::vector<ColAccess>& cols,
                          std::vector<uint64_t*>* flat_out, uint64_t* nrows_out,
                          const LeafLevels** keep, std::vector<uint64_t*>* strpos_out = nullptr);
Status materialize_nested_zip(evql_query* q, const std::vector<ColAccess>& cols,
                              std::vector<uint64_t*>* flat_out, uint64_t* nrows_out,
                              std::vector<uint64_t*>* strpos_out);
Status materialize_within_record(evql_query* q);
Status expand_record_filter(evql_query* q, const LeafLevels* leaf);
Status apply_where_resets(evql_query* q, const LeafLevels* leaf);
// A repeated / nested column as the device writer takes one (chain_compact.cc): levels as one
// byte per slot, one value word per slot (0 where d != dlevel_max; strings: len << 40 |
// position).  The repetition levels are borrowed from the table's leaf cache where it has
// them, everything else is owned; all arrays are padded to a tile multiple.
struct ColumnSlots {
  uint64_t nslots = 0;
  const uint8_t* rlevels = nullptr;       // NULL: rlevel_max == 0, one slot per record
  const uint64_t* rec_offsets = nullptr;  // scanned per-tile counts of the level-0 slots
  const uint8_t* dlevels = nullptr;
  const uint64_t* values = nullptr;
  DevBuf<uint8_t> rlevels_owned, dlevels_owned;
  DevBuf<uint64_t> rec_offsets_owned, values_owned;
};
Status nested_column_slots(evql_table* t, int li, ColumnSlots* out);

// zone_maps.cc
// the (cached) zone statistics of flat column `name`; EVQL_EARG when it does not qualify
Status table_zone_map(evql_table* t, const std::string& name, const evql_table::ZoneMap** out);
bool zone_column_qualifies(const ColumnLayout& cl);
// query_prepare: statistics of the pruning columns -> q->d_zone_bits / tile_skip
Status query_zone_select(evql_query* q);
// tiles of the last launch / skipped tiles -> q->zstats
void zone_stats_after_run(evql_query* q, uint64_t ntiles, uint64_t skipped);

// value_bounds.cc
Status choose_exact_sum_scales(evql_query* q);
Status choose_tuple_widths(evql_query* q);
// maximum |value| of scan column i as the kernel sees it (cached per table column)
Status column_abs_max(evql_query* q, size_t i, double* out);

// query_run.cc
Status query_prepare(evql_query* q);
Status query_launch(evql_query* q);
Status query_finish(evql_query* q);
Status query_reset(evql_query* q);
Status query_recount(evql_query* q);
Status query_dense_into_table(evql_query* q);
Status query_reserve_groups(evql_query* q, uint64_t extra);
Status query_import_pairs(evql_query* q, int which, const uint64_t* d_triples, uint64_t n);
void fill_host_args(evql_query* q, HostArgs* ap);
// how many group records the epilogue of the next launch may leave in the pinned block;
// 0: the lazy tail runs (count pass, blocking copies, compaction on the first next_batch)
uint32_t eager_tail_records(const evql_query* q);

// bare_scan.cc: the life cycle of a bare-scan query (kp.bare_scan)
void bare_configure(evql_query* q);
Status bare_launch(evql_query* q);
Status bare_finish(evql_query* q);
Status bare_reset(evql_query* q);
Status bare_set_limit(evql_query* q, uint32_t n_specs, int64_t limit, uint64_t offset);
Status bare_next_batch(evql_query* q, size_t max_rows, evql_column_buf_t* cols, size_t* nrows);

// results.cc
Status query_set_order(evql_query* q, const evql_sort_spec_t* specs, uint32_t n, int64_t limit,
                       uint64_t offset);
Status query_next_batch(evql_query* q, size_t max_rows, evql_column_buf_t* cols, size_t* nrows);
// what plan_partial_emit (partial_emit_plan.h) decides on for a result of n groups of q
PartialEmitInput partial_emit_input(const evql_query* q, uint64_t n);
// what plan_order_sort (order_sort_plan.h) decides on for n records of q entering the sort
OrderSortInput order_sort_input(const evql_query* q, uint64_t n);
// the groups as dense device records [kind, slot words...] on their way to the host or to the
// device writer (materialize.cc)
struct FetchedRecords {
  uint32_t nwords = 0;        // slot words of a record
  uint64_t* d_rec = nullptr;  // borrowed (small buffer, merged dense records) or `own`
  DevBuf<uint64_t> own;       // records that do not fit the small buffer
  uint64_t n = 0;
  uint64_t total = 0;         // groups of the result before LIMIT
};
Status collect_records(evql_query* q, FetchedRecords* r);
// The value of every scan column at every group's first row, as the result kernels read it
// (result_cell.h, kind 2).  `host_cols` is the source of an asynchronous copy: a FirstRows
// lives until the stream has been synchronised behind gather_first_rows, and as long as a
// kernel reads vals / tags.
struct FirstRows {
  DevBuf<uint64_t> rows;  // [n] the first row of every group
  DevBuf<uint64_t> vals;  // [scan column][n] value words (strings: len << 40 | position)
  DevBuf<uint8_t> tags;   // [scan column][n] bit 0: NULL
  DevBuf<RtColumn> cols;
  std::vector<RtColumn> host_cols;
};
static const uint64_t kNoRowLimit = ~0ull;
// Two kernels, no wait.  The rows are word 1 + first_row_word of the n records at d_rec, rw
// words each -- with a row_limit, a row at or behind it reads as NULL and raises status[1]
// (k_mat_first_rows) -- or, where d_rec is NULL, what the caller has put into fr->rows.
Status gather_first_rows(evql_query* q, const uint64_t* d_rec, uint64_t n, uint32_t rw,
                         uint64_t row_limit, uint64_t* d_status, FirstRows* fr);
// the pinned buffer *p of *cap bytes holds at least `bytes` (grown with some slack)
Status pinned_reserve(uint8_t** p, size_t* cap, size_t bytes);
// One packing of an EmitArgs column set (n, ncols, the cells, elem and -- for strings -- pages
// filled in) as SVector bytes into q->demit, in two phases; the caller owns the wait in
// between, which brings the string totals to the host, and the one behind the second.  The job
// lives until that one.
struct EmitColumnsJob {
  std::vector<DevBuf<uint8_t>> d_out;
  std::vector<DevBuf<uint64_t>> d_off;
  std::vector<uint64_t> str_bytes;
  DevBuf<EmitArgs> d_args;
  uint32_t launches = 0;  // kernels enqueued so far
};
// buffers, the fixed-width kernel, then sizes, scan and total per string column
Status emit_columns_begin(evql_query* q, EmitArgs* ea, EmitColumnsJob* job);
// heaps and bytes kernels of the string columns, one pinned copy per column
Status emit_columns_finish(evql_query* q, EmitArgs* ea, EmitColumnsJob* job);
// materialize.cc: evql_table_from_query
MatInput materialize_input(const evql_query* q, const std::vector<MatSpec>* specs, int sort_column);
Status table_from_query(evql_query* q, const std::vector<ColumnSpec>& specs, int sort_column,
                        int page_order, evql_table** out, evql_materialize_stats_t* stats);
Status sha1_ranges_on_device(evql_ctx* ctx, const void* bytes, size_t len, const uint64_t* offsets,
                             size_t n, uint8_t* out20);

// chain_merge.cc / lsm.cc
Status chain_merge(evql_query* head);
size_t lsm_chain_parts(const evql_lsm_chain* ch, std::vector<evql_table*>* tables,
                       std::vector<const uint8_t*>* d_filters);
evql_ctx* lsm_chain_ctx(const evql_lsm_chain* ch);
// rows every table's filter keeps (all of them where it has none), in chain order
void lsm_chain_rows_kept(const evql_lsm_chain* ch, std::vector<uint64_t>* kept);
// chain_compact.cc: evql_lsm_chain_compact
// `sort` != NULL: evql_lsm_chain_compact_sorted -- the same call with the key statistics, the
// radix sort and the permutes between the gather and the writer
struct CompactSort {
  const char* key_column;
  evql_compact_sort_stats_t* stats;  // may be NULL
};
Status chain_compact(evql_lsm_chain* ch, const std::vector<ColumnSpec>& specs, int row_order,
                     int page_order, evql_table** out, evql_compact_stats_t* stats,
                     const CompactSort* sort = nullptr);
// the query's groups as dense records of rplan()'s layout: `dense` holds the first `nd`
// groups, the remaining ngroups - nd sit in the HBM group table (compact them from there)
struct RecordsView {
  const uint64_t* dense = nullptr;
  uint64_t nd = 0;
};
Status query_records_view(evql_query* q, RecordsView* out);

// group_records.cc: groups that leave the scan (group imports, chain_merge.cc, exchange.cc)
static const int kFreshGroupCounter = 4;  // d_counters word: occupied slots (a launch / a merge)
static const int kScratchCounter = 6;     // d_counters word: records / triples a kernel wrote
static const uint32_t kMergeSkip = 254;   // (rt_atomic knows no such op: the word is left alone)
// A group outside the scan: a dense record [kind, slot words of rplan()] of rw_in words; sent
// by plans that read first-row values as a wire record of rw words (+ one value word per scan
// column, strings as len << 40 | heap offset, + one word of NULL tags); merged into a slot of
// mw words (a wire record without its kind).
struct GroupRecordLayout {
  uint32_t W = 0, nc = 0;  // slot words of the scan's table, scan columns
  bool resolved = false;   // first-row values travel in the records (need_first_row)
  uint32_t rw_in = 0, rw = 0, mw = 0;
  std::vector<uint32_t> str_cols;  // the string columns among the resolved ones
  uint64_t str_mask = 0;
  uint32_t first_row_word = 0xffffffffu;  // slot word of the first row (all ones: none)
  uint32_t has_ident2 = 0;
};
GroupRecordLayout group_record_layout(const KernelPlan& kp);
// what a merged table / the string kernels cannot hold (plan_kind: "an exchanged", "a chain")
Status group_record_layout_check(const GroupRecordLayout& L, const char* plan_kind);
// an empty slot's first nwords words: all ones (identity, first row), the states' identities, 0
void slot_identities(const KernelPlan& kp, uint32_t nwords, uint64_t* out);
// a->nwords (words_per_slot), has_ident2, ops[]; skip_distinct: count_distinct words stay as
// they are (kMergeSkip): they count the pairs of the MERGED set, which are inserted separately
void merge_ops(const KernelPlan& kp, bool skip_distinct, MergeArgs* a);
// row-addressable views of q's scan columns, for gathers at the groups' first rows
Status first_row_columns(evql_query* q, std::vector<RtColumn>* out);
// n dense records -> wire records; *rc (host copy of d_cols) lives until the next synchronisation
Status resolve_first_rows(evql_query* q, const GroupRecordLayout& L, uint64_t rank_tag,
                          std::vector<RtColumn>* rc, RtColumn* d_cols, const uint64_t* in, uint64_t n,
                          uint64_t* out);
// q's ngroups groups (view: query_records_view) as one run of dense records at dst
Status query_dense_records(evql_query* q, const GroupRecordLayout& L, const RecordsView& view,
                           uint64_t* dst);
// stored triples of a pair set (NULL: none) -> *n; one synchronisation
Status pairset_count(evql_query* q, const uint64_t* set, uint64_t cap, uint64_t* n);
// q->d_mtab as an empty table for total_records groups at load factor <= 1/2 (a failed
// allocation leaves d_mtab NULL and mcap 0); *ma ready for one merge launch per rank / table
Status merged_table_prepare(evql_query* q, const GroupRecordLayout& L, uint64_t total_records,
                            MergeResolvedArgs* ma);
// q->d_mset[which] as an empty set of cap slots, then n triples inserted (counted in `word`)
Status merged_set_fill(evql_query* q, const GroupRecordLayout& L, int which, uint64_t cap,
                       uint32_t word, const uint64_t* d_triples, uint64_t n);
// The string words of n wire records (nseg owner segments, seg[nseg + 1] their first records)
// become offsets into a heap of heap_for(bytes) (NULL = failed), which gets the bytes (from
// `flat`, or the columns' pages); segoff[nseg + 1]: byte offset of every segment.  One sync.
Status wire_strings(evql_query* q, const GroupRecordLayout& L, const uint8_t* flat, uint64_t* records,
                    uint64_t n, const uint64_t* seg, uint32_t nseg, uint64_t* d_sizes, uint64_t* d_seg,
                    const std::function<uint8_t*(uint64_t)>& heap_for, uint64_t* segoff);
// d_status word 0 behind a merge: bit 1 = the group table is full, bit 3 = a pair set is
Status merge_status_error(uint32_t status, const char* what);
// device_writer.cc: a cstable v0.2.0 image encoded on the device from SoA columns
struct DeviceColumnIn {
  const uint64_t* values;  // device, num_rows value words
  const uint8_t* nulls;    // device, num_rows bytes (1 = NULL) or nullptr
  const uint8_t* bytes;    // device, string columns: the heap `values` point into
  // repeated / nested columns: one (r, d, value) triple per SLOT
  const uint8_t* rlevels;  // device, num_slots bytes (rlevel_max > 0)
  const uint8_t* dlevels;  // device, num_slots bytes (instead of `nulls`)
  uint64_t num_slots;      // 0 = one slot per row
};
Status table_from_device_columns(evql_ctx* ctx, const std::vector<ColumnSpec>& specs,
                                 const std::vector<DeviceColumnIn>& in, uint64_t num_rows,
                                 int page_order, evql_table** out);
}  // namespace evql
