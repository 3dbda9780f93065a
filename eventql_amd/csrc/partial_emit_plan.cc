// partial_emit_plan.cc -- see partial_emit_plan.h
#include "partial_emit_plan.h"
#include "codegen.h"

namespace evql {

namespace {

// the exact key: the record's identity word (also after a merge)
void key_cell(const LoweredProgram& lp, PartialCell* cell) {
  cell->kind = 0;
  cell->stype = lp.return_type;
  cell->is_bool = lp.return_type == EVQL_T_BOOL;
}

// a first-row cell as PARTIAL takes it: never of a merged result, a STRING only from a hashed
// string column
bool partial_first_row_cell(const PartialEmitInput& in, const LoweredProgram& lp, PartialCell* cell) {
  if (in.merged || !in.kp->need_first_row) return false;
  if (!first_row_cell(*in.kp, *in.scan_select, lp, cell)) return false;
  return (lp.return_type == EVQL_T_STRING) == bool(cell->is_string);
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
      // one fixed-width key, a bare column.  A computed key (`a + 1`) keeps the host loop like
      // every other evaluated expression.
      uint32_t c = 0;
      if (ngroup != 1 || lp.return_type == EVQL_T_STRING || !bare_column(kp, *in.scan_select, lp, &c)) {
        return PEMIT_GROUP_EXPR;
      }
      key_cell(lp, &cell);
    } else if (kp.key_mode != KEY_HASHED || !partial_first_row_cell(in, lp, &cell)) {
      return PEMIT_GROUP_EXPR;
    }
    out->tuple.push_back(cell);
  }
  for (size_t i = 0; i < nsel; ++i) {
    const LoweredProgram& lp = (*in.select)[i];
    PartialCell cell{};
    if (lp.is_aggregate) {
      // PARTIAL rows carry the saved state, whatever the expression does with the value: no
      // AGG_GET rule here, unlike the FINAL routes
      const AggPlan* a = nullptr;
      if (!aggregate_cell(kp, (*in.select_agg_index)[i], &cell, &a)) return PEMIT_AGGREGATE;
      switch (a->fn) {
        case EVQL_AGG_COUNT: case EVQL_AGG_SUM_UINT64: case EVQL_AGG_SUM_INT64:
          cell.state = PSTATE_VARUINT;
          break;
        case EVQL_AGG_SUM_FLOAT64:
          if (a->exact_index >= 0) return PEMIT_AGGREGATE;  // (128-bit rounding: host)
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
        // (the key mode must be EXACT here; FINAL asks for no key mode)
        if (kp.key_mode != KEY_EXACT || lp.return_type == EVQL_T_STRING) return PEMIT_SELECT_EXPR;
        key_cell(lp, &cell);
      } else if (!partial_first_row_cell(in, lp, &cell)) {
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
