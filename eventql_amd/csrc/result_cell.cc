// result_cell.cc -- see result_cell.h
#include "result_cell.h"
#include "codegen.h"

namespace evql {

bool aggregate_cell(const KernelPlan& kp, int agg_index, ResultCell* cell, const AggPlan** agg) {
  if (agg_index < 0 || size_t(agg_index) >= kp.aggs.size()) return false;
  const AggPlan& a = kp.aggs[agg_index];
  if (agg) *agg = &a;
  cell->kind = 1;
  cell->word = uint32_t(1 + kp.state_word_base() + a.first_word);
  cell->count_word = -1;
  cell->is_mean = 0;
  switch (a.fn) {
    case EVQL_AGG_COUNT: case EVQL_AGG_SUM_UINT64: case EVQL_AGG_SUM_INT64:
    case EVQL_AGG_SUM_FLOAT64:
    case EVQL_AGG_COUNT_DISTINCT_UINT64:  // (one word: the number of distinct values)
      break;
    case EVQL_AGG_MEAN_UINT64: case EVQL_AGG_MEAN_INT64: case EVQL_AGG_MEAN_FLOAT64:
      cell->is_mean = 1;
      cell->count_word = int32_t(cell->word + 1);
      break;
    default:  // min / max
      cell->count_word = int32_t(cell->word + 1);
  }
  return true;
}

bool bare_column(const KernelPlan& kp, const std::vector<LoweredProgram>& scan_select,
                 const LoweredProgram& lp, uint32_t* col) {
  if (!lp.call || lp.call->kind != Expr::INPUT) return false;
  const uint32_t j = lp.call->input;
  if (j >= scan_select.size()) return false;
  const ExprPtr& se = scan_select[j].call;
  if (!se || se->kind != Expr::INPUT) return false;
  *col = se->input;
  return *col < kp.cols.size();
}

bool first_row_cell(const KernelPlan& kp, const std::vector<LoweredProgram>& scan_select,
                    const LoweredProgram& lp, ResultCell* cell) {
  uint32_t c = 0;
  if (!bare_column(kp, scan_select, lp, &c)) return false;
  const ColAccess& ca = kp.cols[c];
  if (ca.stype != lp.return_type) return false;
  cell->kind = 2;
  cell->stype = lp.return_type;
  cell->src = c;
  cell->to_float = ca.stype == EVQL_T_FLOAT64 && ca.from_uint_to_float;
  cell->is_string = ca.string_hash;
  cell->is_bool = lp.return_type == EVQL_T_BOOL;
  return true;
}

}  // namespace evql
