// order_sort_plan.h -- the host-only part of ORDER BY above a large GROUP BY result sorted on
// the device (results.cc sort_on_device): which results take the device path, and where every
// sort key is read from in a group record.  No HIP call and no device state: it builds and runs
// on its own (tools/order_sort_plan_check.cc).
#pragma once
#include <cstdint>
#include <vector>

namespace evql {

struct KernelPlan;
struct LoweredProgram;

static const uint32_t kMaxOrderSortSpecs = 8;

// where the device finds one sort key in a record: the host-side fields of OrderKeyArgs
// (aot_kernels.h)
struct OrderKeySpec {
  uint32_t from_ident;  // 1: the group key itself (record[0] = kind, record[1] = identity)
  uint32_t word;        // record word holding the value (state word / identity)
  int32_t count_word;   // >= 0: non-null input count (min / max / mean); 0 => value reads 0
  uint32_t type;        // 0 unsigned, 1 signed, 2 float64
  uint32_t is_mean;     // value = f64(word) / count
  uint32_t descending;
};

// one sort expression against the select list
enum OrderKeyClass {
  OKEY_RECORD = 0,      // a plain output column whose value a record holds
  OKEY_EXPRESSION = 1,  // not a plain output column
  OKEY_EXACT_SUM = 2,   // an exact float sum (rounded from 128 bits on the host)
  OKEY_UNREADABLE = 3   // a string, a first-row column, post-aggregate arithmetic
};

enum OrderSortDecision {
  OSORT_DEVICE = 0,
  OSORT_NO_ORDER = 1,         // no sort spec (LIMIT alone), or not EVQL_MODE_FINAL
  OSORT_FEW_RECORDS = 2,      // fewer than kDeviceEmitMinGroups records enter the sort
  OSORT_SWITCHED_OFF = 3,     // EVQL_ORDER_DEVICE_SORT=0
  OSORT_EXPRESSION = 4,       // a spec is an expression
  OSORT_UNREADABLE = 5,       // a spec column cannot be read from a record
  OSORT_TOO_MANY_SPECS = 6,   // more than kMaxOrderSortSpecs
  OSORT_TOO_MANY_RECORDS = 7, // 2^32 records or more
  OSORT_NAN_KEY = 8           // (set by the runtime: a float key was NaN, the host ordered)
};

struct OrderSortInput {
  uint32_t group_mode = 0;  // EVQL_MODE_*
  uint64_t n = 0;           // records entering the sort (after the top-k selection, if it ran)
  bool enabled = true;      // EVQL_ORDER_DEVICE_SORT, read when the query was created
  const KernelPlan* kp = nullptr;  // the plan the records follow (evql_query::rplan)
  const std::vector<LoweredProgram>* select = nullptr;
  const std::vector<int>* select_agg_index = nullptr;
  const std::vector<bool>* select_passthrough = nullptr;
  const std::vector<LoweredProgram>* order = nullptr;  // over the select list
  const std::vector<bool>* order_desc = nullptr;
};

struct OrderSortPlan {
  std::vector<OrderKeySpec> keys;  // one per sort spec, in spec order
  uint32_t base_word = 1;          // the record word sort_host_records orders by
};

// What query_set_order accepts as the first sort spec, for any spec.  Fills *out for
// OKEY_RECORD.
OrderKeyClass classify_order_key(const KernelPlan& kp, const std::vector<LoweredProgram>& select,
                                 const std::vector<int>& select_agg_index,
                                 const std::vector<bool>& select_passthrough,
                                 const LoweredProgram& spec, bool descending, OrderKeySpec* out);

// The rules of DESIGN.md 3.13.  Returns OSORT_DEVICE and fills *out, or why order_fetched
// keeps the result.
OrderSortDecision plan_order_sort(const OrderSortInput& in, OrderSortPlan* out);

}  // namespace evql
