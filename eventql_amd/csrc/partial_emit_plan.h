// partial_emit_plan.h -- the host-only part of packing EVQL_MODE_PARTIAL rows on the device
// (results.cc emit_partial_on_device): which results take the device path, and what every
// cell of a row's group tuple and saved-state string is read from.  No HIP call and no device
// state: it builds and runs on its own (tools/partial_emit_plan_check.cc).
#pragma once
#include <cstdint>
#include <vector>
#include "result_cell.h"

namespace evql {

// results of at least this many groups are packed on the device (FINAL and PARTIAL)
static const uint64_t kDeviceEmitMinGroups = 1 << 16;
static const uint32_t kMaxEmitCols = 32;

// one cell of a PARTIAL row, as the k_partial_* kernels read it: where it lives (result_cell.h)
// and what a PARTIAL row adds
struct PartialCell : ResultCell {
  uint32_t state = 0;     // kind 1: PartialState
  const uint64_t* pages = nullptr;  // strings: data pages of the source column (set by the runtime)
};
enum PartialState {
  PSTATE_VARUINT = 0,       // count / integer sum: LEB128 of the word
  PSTATE_RAW8 = 1,          // sum(float64): the 8 bytes of the word
  PSTATE_COUNT_RAW8 = 2     // min / max / mean: LEB128 of the count, the 8 bytes (0 without a value)
};

enum PartialEmitDecision {
  PEMIT_DEVICE = 0,
  PEMIT_NOT_PARTIAL = 1,    // EVQL_MODE_FINAL
  PEMIT_FEW_GROUPS = 2,     // n < kDeviceEmitMinGroups
  PEMIT_SWITCHED_OFF = 3,   // EVQL_PARTIAL_DEVICE_EMIT=0
  PEMIT_GROUP_EXPR = 4,     // a group expression needs eval_expr / a merged result's first row
  PEMIT_SELECT_EXPR = 5,    // a non-aggregate select expression does
  PEMIT_AGGREGATE = 6,      // count_distinct, an exact float sum
  PEMIT_TOO_WIDE = 7,       // more than kMaxEmitCols cells, or none
  PEMIT_NIL_COLUMN = 8,     // a NIL-typed cell
  PEMIT_NESTED = 9          // a nested (Dremel) scan
};

struct PartialEmitInput {
  uint32_t group_mode = 0;  // EVQL_MODE_*
  uint64_t n = 0;           // groups of the result
  bool enabled = true;      // EVQL_PARTIAL_DEVICE_EMIT, read when the query was created
  bool merged = false;      // the records come out of an exchange / a chain merge
  bool nested = false;      // a nested (Dremel) scan
  const KernelPlan* kp = nullptr;  // the plan the records follow (evql_query::rplan)
  const std::vector<LoweredProgram>* scan_select = nullptr;
  const std::vector<LoweredProgram>* group = nullptr;
  const std::vector<LoweredProgram>* select = nullptr;
  const std::vector<int>* select_agg_index = nullptr;
  const std::vector<bool>* select_passthrough = nullptr;
};

struct PartialEmitPlan {
  std::vector<PartialCell> tuple;  // in tuple order: the LAST group expression first
  std::vector<PartialCell> data;   // in select-list order
  bool need_first = false;         // some cell is of kind 2
};

// The rules of DESIGN.md 3.7.  Returns PEMIT_DEVICE and fills *out, or why the host loop of
// query_next_batch keeps the result.
PartialEmitDecision plan_partial_emit(const PartialEmitInput& in, PartialEmitPlan* out);

}  // namespace evql
