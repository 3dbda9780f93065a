// order_sort_plan.cc -- see order_sort_plan.h
#include "order_sort_plan.h"
#include "codegen.h"
#include "partial_emit_plan.h"

namespace evql {

OrderKeyClass classify_order_key(const KernelPlan& kp, const std::vector<LoweredProgram>& select,
                                 const std::vector<int>& select_agg_index,
                                 const std::vector<bool>& select_passthrough,
                                 const LoweredProgram& spec, bool descending, OrderKeyArgs* out) {
  if (!spec.call || spec.call->kind != Expr::INPUT) return OKEY_EXPRESSION;
  const uint32_t si = spec.call->input;
  if (si >= select.size()) return OKEY_UNREADABLE;
  const LoweredProgram& sp = select[si];
  auto type_code = [](uint32_t t) { return t == EVQL_T_INT64 ? 1u : (t == EVQL_T_FLOAT64 ? 2u : 0u); };
  OrderKeyArgs ok{};
  ok.stype = sp.return_type;
  ok.descending = descending;
  if (si < select_passthrough.size() && select_passthrough[si] && sp.return_type != EVQL_T_STRING) {
    // (no key-mode rule: a hashed key's identity orders as the host orders it)
    ok.kind = 0;
    ok.from_ident = 1;
    ok.word = 1;
    ok.type = type_code(sp.return_type);
  } else if (sp.is_aggregate && sp.call && sp.call->kind == Expr::AGG_GET) {
    const int ai = si < select_agg_index.size() ? select_agg_index[si] : -1;
    const AggPlan* a = nullptr;
    if (!aggregate_cell(kp, ai, &ok, &a)) return OKEY_UNREADABLE;
    // how the state orders: the function's own type, not the expression's, except for min / max
    if (a->fn == EVQL_AGG_SUM_FLOAT64) {
      if (a->exact_index >= 0) return OKEY_EXACT_SUM;
      ok.type = 2;
    } else if (a->fn == EVQL_AGG_SUM_INT64) {
      ok.type = 1;
    } else if (ok.is_mean) {
      ok.type = 2;
    } else {  // min / max by the expression's type; the counts are unsigned
      ok.type = ok.count_word >= 0 ? type_code(sp.return_type) : 0u;
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
    OrderKeyArgs ok{};
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
