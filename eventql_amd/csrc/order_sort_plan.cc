// order_sort_plan.cc -- see order_sort_plan.h
#include "order_sort_plan.h"
#include "codegen.h"
#include "partial_emit_plan.h"

namespace evql {

OrderKeyClass classify_order_key(const KernelPlan& kp, const std::vector<LoweredProgram>& select,
                                 const std::vector<int>& select_agg_index,
                                 const std::vector<bool>& select_passthrough,
                                 const LoweredProgram& spec, bool descending, OrderKeySpec* out) {
  if (!spec.call || spec.call->kind != Expr::INPUT) return OKEY_EXPRESSION;
  const uint32_t si = spec.call->input;
  if (si >= select.size()) return OKEY_UNREADABLE;
  const LoweredProgram& sp = select[si];
  auto type_code = [](uint32_t t) { return t == EVQL_T_INT64 ? 1u : (t == EVQL_T_FLOAT64 ? 2u : 0u); };
  OrderKeySpec ok{};
  ok.count_word = -1;
  ok.descending = descending;
  if (si < select_passthrough.size() && select_passthrough[si] && sp.return_type != EVQL_T_STRING) {
    ok.from_ident = 1;
    ok.word = 1;
    ok.type = type_code(sp.return_type);
  } else if (sp.is_aggregate && sp.call && sp.call->kind == Expr::AGG_GET) {
    const int ai = si < select_agg_index.size() ? select_agg_index[si] : -1;
    if (ai < 0 || size_t(ai) >= kp.aggs.size()) return OKEY_UNREADABLE;
    const AggPlan& a = kp.aggs[ai];
    ok.word = uint32_t(1 + kp.state_word_base() + a.first_word);
    switch (a.fn) {
      case EVQL_AGG_COUNT:
      case EVQL_AGG_COUNT_DISTINCT_UINT64:  // (one word: the number of distinct values)
      case EVQL_AGG_SUM_UINT64: ok.type = 0; break;
      case EVQL_AGG_SUM_INT64: ok.type = 1; break;
      case EVQL_AGG_SUM_FLOAT64:
        if (a.exact_index >= 0) return OKEY_EXACT_SUM;
        ok.type = 2;
        break;
      case EVQL_AGG_MEAN_UINT64:
      case EVQL_AGG_MEAN_INT64:
      case EVQL_AGG_MEAN_FLOAT64:
        ok.type = 2;
        ok.is_mean = 1;
        ok.count_word = int32_t(ok.word + 1);
        break;
      default:  // min / max
        ok.type = type_code(sp.return_type);
        ok.count_word = int32_t(ok.word + 1);
    }
  } else {
    return OKEY_UNREADABLE;
  }
  *out = ok;
  return OKEY_RECORD;
}

OrderSortDecision plan_order_sort(const OrderSortInput& in, OrderSortPlan* out) {
  *out = OrderSortPlan();
  if (in.group_mode != EVQL_MODE_FINAL || !in.order || in.order->empty()) return OSORT_NO_ORDER;
  if (in.n < kDeviceEmitMinGroups) return OSORT_FEW_RECORDS;
  if (!in.enabled) return OSORT_SWITCHED_OFF;
  const size_t ns = in.order->size();
  if (ns > kMaxOrderSortSpecs) return OSORT_TOO_MANY_SPECS;
  if (in.n >= (1ull << 32)) return OSORT_TOO_MANY_RECORDS;
  const KernelPlan& kp = *in.kp;
  for (size_t j = 0; j < ns; ++j) {
    OrderKeySpec ok{};
    const bool desc = j < in.order_desc->size() && (*in.order_desc)[j];
    switch (classify_order_key(kp, *in.select, *in.select_agg_index, *in.select_passthrough,
                               (*in.order)[j], desc, &ok)) {
      case OKEY_RECORD: break;
      case OKEY_EXPRESSION: return OSORT_EXPRESSION;
      default: return OSORT_UNREADABLE;
    }
    out->keys.push_back(ok);
  }
  // sort_host_records: by first row (scan order) or by identity
  out->base_word = kp.need_first_row ? uint32_t(1 + kp.first_row_word()) : 1u;
  return OSORT_DEVICE;
}

}  // namespace evql
