// chain_compact_plan.h -- the host-only part of evql_lsm_chain_compact (chain_compact.cc):
// which column of which table feeds an output column, and how large the flat output is.
// No HIP call and no device state: it builds and runs on its own (tools/chain_compact_plan_check.cc).
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "cstable_format.h"

namespace evql {

static const uint64_t kCompactTile = 2048;  // rows / slots per workgroup of the k_cmp_* kernels

struct CompactColumn {
  // levels per slot (rlevel_max > 0 || dlevel_max > 1): what the device writer calls nested
  bool nested = false;
  bool is_string = false;
  // `__lsm_is_update`: false for every row, no table is read (compaction_strategy.cc:161)
  bool constant_false = false;
  // per table (chain order): layout index of the column, -1 = absent -> one NULL per record
  std::vector<int> source;
};

struct CompactPlan {
  std::vector<CompactColumn> columns;
  // per table (chain order): position in the output (0 = first)
  std::vector<uint32_t> position;
  // per table (chain order): first output row, tiles in front of it
  std::vector<uint64_t> row_base, tile_base;
  uint64_t rows_in = 0, rows_out = 0, tiles = 0;
};

// The column rules of evql_lsm_chain_compact (include/evql_gpu.h).  `tables` / `rows_kept` in
// chain order (newest first); reverse_order: EVQL_COMPACT_FILE_ORDER.  Returns "" or the
// message of the EVQL_EARG error.
std::string plan_chain_compact(const std::vector<const TableLayout*>& tables,
                               const std::vector<uint64_t>& rows_kept,
                               const std::vector<ColumnSpec>& specs, bool reverse_order,
                               CompactPlan* out);

// The key rule of evql_lsm_chain_compact_sorted (include/evql_gpu.h): the key is one of
// `specs`, flat and required, unsigned integer or datetime; no output column is repeated or
// nested (the permutation moves rows, not records with their slot runs); the row index is u32.
// Returns "" and *key_index, or the message of the error; *not_supported tells EVQL_ENOTSUP
// from EVQL_EARG.  `key_column` may be NULL (EVQL_EARG).
std::string plan_compact_sort_key(const std::vector<ColumnSpec>& specs, const char* key_column,
                                  size_t* key_index, bool* not_supported);
// rows_out of a plan that the sort can index
std::string plan_compact_sort_rows(uint64_t rows_out, bool* not_supported);

}  // namespace evql
