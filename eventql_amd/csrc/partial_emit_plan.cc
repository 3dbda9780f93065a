// partial_emit_plan.cc -- see partial_emit_plan.h
#include "partial_emit_plan.h"
#include "codegen.h"

namespace evql {

namespace {

// a bare column: `lp` = X_INPUT(j) of the scan select list, whose expression j = X_INPUT(c) of
// the scan columns
bool bare_column(const PartialEmitInput& in, const LoweredProgram& lp, uint32_t* col) {
  if (!lp.call || lp.call->kind != Expr::INPUT) return false;
  const uint32_t j = lp.call->input;
  if (j >= in.scan_select->size()) return false;
  const ExprPtr& se = (*in.scan_select)[j].call;
  if (!se || se->kind != Expr::INPUT) return false;
  *col = se->input;
  return *col < in.kp->cols.size();
}

// ... read from the group's first row: what device_emit_columns (results.cc) accepts as kind 2
bool first_row_cell(const PartialEmitInput& in, const LoweredProgram& lp, PartialCell* cell) {
  const KernelPlan& kp = *in.kp;
  if (in.merged || !kp.need_first_row) return false;
  uint32_t c = 0;
  if (!bare_column(in, lp, &c)) return false;
  const ColAccess& ca = kp.cols[c];
  if (ca.stype != lp.return_type) return false;
  if ((lp.return_type == EVQL_T_STRING) != ca.string_hash) return false;
  cell->kind = 2;
  cell->stype = lp.return_type;
  cell->src = c;
  cell->to_float = ca.stype == EVQL_T_FLOAT64 && ca.from_uint_to_float;
  cell->is_string = ca.string_hash;
  cell->is_bool = lp.return_type == EVQL_T_BOOL;
  return true;
}

}  // namespace

PartialEmitDecision plan_partial_emit(const PartialEmitInput& in, PartialEmitPlan* out) {
  *out = PartialEmitPlan();
  if (in.group_mode != EVQL_MODE_PARTIAL) return PEMIT_NOT_PARTIAL;
  if (in.n < kDeviceEmitMinGroups) return PEMIT_FEW_GROUPS;
  if (!in.enabled) return PEMIT_SWITCHED_OFF;
  if (in.nested) return PEMIT_NESTED;
  const KernelPlan& kp = *in.kp;
  const size_t ngroup = in.group->size(), nsel = in.select->size();
  if (ngroup == 0 || ngroup > kMaxEmitCols || nsel == 0 || nsel > kMaxEmitCols) return PEMIT_TOO_WIDE;
  // the group tuple: append_svector(group[i]) for i = n_group - 1 .. 0 (groupby.cc:112-135)
  for (size_t gi = ngroup; gi-- > 0;) {
    const LoweredProgram& lp = (*in.group)[gi];
    PartialCell cell{};
    if (lp.return_type == EVQL_T_NIL) return PEMIT_NIL_COLUMN;
    if (kp.key_mode == KEY_EXACT) {
      // one fixed-width key, a bare column: the record's identity word (also after a merge).
      // A computed key (`a + 1`) keeps the host loop like every other evaluated expression.
      uint32_t c = 0;
      if (ngroup != 1 || lp.return_type == EVQL_T_STRING || !bare_column(in, lp, &c)) {
        return PEMIT_GROUP_EXPR;
      }
      cell.kind = 0;
      cell.stype = lp.return_type;
      cell.is_bool = lp.return_type == EVQL_T_BOOL;
    } else if (kp.key_mode != KEY_HASHED || !first_row_cell(in, lp, &cell)) {
      return PEMIT_GROUP_EXPR;
    }
    out->tuple.push_back(cell);
  }
  for (size_t i = 0; i < nsel; ++i) {
    const LoweredProgram& lp = (*in.select)[i];
    PartialCell cell{};
    if (lp.is_aggregate) {
      // (PARTIAL rows carry the saved state, whatever the expression does with the value)
      const int ai = (*in.select_agg_index)[i];
      if (ai < 0 || size_t(ai) >= kp.aggs.size()) return PEMIT_AGGREGATE;
      const AggPlan& a = kp.aggs[ai];
      cell.kind = 1;
      cell.word = uint32_t(1 + kp.state_word_base() + a.first_word);
      switch (a.fn) {
        case EVQL_AGG_COUNT: case EVQL_AGG_SUM_UINT64: case EVQL_AGG_SUM_INT64:
          cell.state = PSTATE_VARUINT;
          break;
        case EVQL_AGG_SUM_FLOAT64:
          if (a.exact_index >= 0) return PEMIT_AGGREGATE;  // (128-bit rounding: host)
          cell.state = PSTATE_RAW8;
          break;
        case EVQL_AGG_MIN_UINT64: case EVQL_AGG_MAX_UINT64: case EVQL_AGG_MIN_INT64:
        case EVQL_AGG_MAX_INT64: case EVQL_AGG_MIN_FLOAT64: case EVQL_AGG_MAX_FLOAT64:
        case EVQL_AGG_MEAN_UINT64: case EVQL_AGG_MEAN_INT64: case EVQL_AGG_MEAN_FLOAT64:
          cell.state = PSTATE_COUNT_RAW8;
          break;
        default:  // count_distinct: the saved state is a set
          return PEMIT_AGGREGATE;
      }
    } else {
      if (lp.return_type == EVQL_T_NIL) return PEMIT_NIL_COLUMN;
      if (i < in.select_passthrough->size() && (*in.select_passthrough)[i]) {
        if (kp.key_mode != KEY_EXACT || lp.return_type == EVQL_T_STRING) return PEMIT_SELECT_EXPR;
        cell.kind = 0;
        cell.stype = lp.return_type;
        cell.is_bool = lp.return_type == EVQL_T_BOOL;
      } else if (!first_row_cell(in, lp, &cell)) {
        return PEMIT_SELECT_EXPR;
      }
    }
    out->data.push_back(cell);
  }
  for (const PartialCell& c : out->tuple) out->need_first = out->need_first || c.kind == 2;
  for (const PartialCell& c : out->data) out->need_first = out->need_first || c.kind == 2;
  return PEMIT_DEVICE;
}

}  // namespace evql
