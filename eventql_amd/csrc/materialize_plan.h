// materialize_plan.h -- the host-only part of materialising a GROUP BY result as a resident
// cstable (materialize.cc, evql_table_from_query): which executed queries qualify, and what
// every output column is read from.  No HIP call and no device state: it builds and runs on
// its own (tools/materialize_plan_check.cc).
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "result_cell.h"

namespace evql {

// one output column: where the k_mat_* kernels read it (result_cell.h; aot_kernels.h MatCol
// takes the cell as it is) and what only the host needs to know
struct MatCell : ResultCell {
  uint32_t optional = 0;   // the spec's dlevel_max == 1: the column takes NULL bytes
};

// why not; the C ABI hands the numbers out (evql_plan_materialize)
enum MatDecision {
  MAT_DEVICE = 0,
  MAT_PARTIAL_MODE = 1,   // EVQL_MODE_PARTIAL                                  EVQL_EARG
  MAT_COLUMN_COUNT = 2,   // ncols != select count                               EVQL_EARG
  MAT_NESTED_SPEC = 3,    // rlevel_max > 0 or dlevel_max > 1                    EVQL_EARG
  MAT_TYPE_MISMATCH = 4,  // the return type does not fit the logical type       EVQL_EARG
  MAT_SORT_COLUMN = 5,    // sort_column outside [-1, ncols)                     EVQL_EARG
  MAT_BARE_SCAN = 6,      // everything below: EVQL_ENOTSUP
  MAT_ORDER_LIMIT = 7,    // ORDER BY / LIMIT set on the query
  MAT_TOO_WIDE = 8,       // more than kMaxMatCols columns
  MAT_POST_AGGREGATE = 9, // sum(a) + 1
  MAT_EXACT_SUM = 10,     // an exact float sum
  MAT_INT64 = 11,         // an INT64-typed column
  MAT_NIL = 12,           // a NIL-typed column
  MAT_KEY_EXPR = 13,      // a computed or hashed key / select expression that is no bare column
  MAT_FIRST_ROW = 14,     // a first-row column of a merged result or of a nested scan
  MAT_SORT_KEY = 15,      // the sort column is optional or not unsigned-integer / datetime
  MAT_SORT_ROWS = 16      // more than 2^32 - 1 rows with a sort column
};
static const uint32_t kMaxMatCols = 32;

// what the plan needs to know of an output column's spec
struct MatSpec {
  std::string name;
  uint32_t logical_type = 0;  // ColumnType
  uint32_t rlevel_max = 0, dlevel_max = 0;
};

struct MatInput {
  uint32_t group_mode = 0;   // EVQL_MODE_*
  uint64_t n = 0;            // groups of the result (0 where it is not known yet)
  bool merged = false;       // the records come out of an exchange / a chain merge
  bool nested = false;       // a nested (Dremel) scan
  bool ordered = false;      // ORDER BY / LIMIT set
  const KernelPlan* kp = nullptr;  // the plan the records follow (evql_query::rplan)
  const std::vector<LoweredProgram>* scan_select = nullptr;
  const std::vector<LoweredProgram>* select = nullptr;
  const std::vector<int>* select_agg_index = nullptr;
  const std::vector<bool>* select_passthrough = nullptr;
  const std::vector<MatSpec>* specs = nullptr;
  int sort_column = -1;
};

struct MatPlan {
  std::vector<MatCell> cells;  // one per output column = select expression
  bool need_first = false;     // some cell is of kind 2
  std::string reason;          // of a refusal: what evql_last_error reports
};

// EVQL_EARG / EVQL_ENOTSUP of a refusal (EVQL_OK for MAT_DEVICE)
int mat_decision_code(MatDecision d);

// The rules of DESIGN.md 3.12.  Returns MAT_DEVICE and fills out->cells, or why not.
MatDecision plan_materialize(const MatInput& in, MatPlan* out);

}  // namespace evql
