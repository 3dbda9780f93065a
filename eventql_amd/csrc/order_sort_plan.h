// order_sort_plan.h -- the host-only part of ORDER BY above a large GROUP BY result sorted on
// the device (results.cc sort_on_device): which results take the device path, and where every
// sort key is read from in a group record.  No HIP call and no device state: it builds and runs
// on its own (tools/order_sort_plan_check.cc).
#pragma once
#include <cstdint>
#include <vector>
#include "result_cell.h"

namespace evql {

static const uint32_t kMaxOrderSortSpecs = 8;

// The 64-bit order-preserving key of one sort expression, per dense record: where the device
// finds the value in a record (result_cell.h: the key, kind 0 with word 1, or a state, kind 1;
// a NULL reads 0) and how it orders.  The plan fills the cell, type, descending and from_ident;
// the runtime adds the pointers and counts (k_order_keys, k_ord_key_perm: aot_kernels.h).
struct OrderKeyArgs : ResultCell {
  const uint64_t* records = nullptr;  // [n][record_words]
  uint32_t record_words = 0;
  uint64_t n = 0;
  uint32_t from_ident = 0;  // 1: the group key itself (record[0] = kind, record[1] = identity)
  uint32_t type = 0;        // 0 unsigned, 1 signed, 2 float64 (cmp_uint64 / _int64 / _float64)
  uint32_t descending = 0;
  uint64_t* keys = nullptr;
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
  std::vector<OrderKeyArgs> keys;  // one per sort spec, in spec order
  uint32_t base_word = 1;          // the record word sort_host_records orders by
};

// What query_set_order accepts as the first sort spec, for any spec.  Fills *out for
// OKEY_RECORD.
OrderKeyClass classify_order_key(const KernelPlan& kp, const std::vector<LoweredProgram>& select,
                                 const std::vector<int>& select_agg_index,
                                 const std::vector<bool>& select_passthrough,
                                 const LoweredProgram& spec, bool descending, OrderKeyArgs* out);

// The rules of DESIGN.md 3.13.  Returns OSORT_DEVICE and fills *out, or why order_fetched
// keeps the result.
OrderSortDecision plan_order_sort(const OrderSortInput& in, OrderSortPlan* out);

}  // namespace evql
