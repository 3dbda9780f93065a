// materialize_plan.cc -- see materialize_plan.h
#include "materialize_plan.h"
#include "codegen.h"

namespace evql {

namespace {

MatDecision refuse(MatPlan* out, MatDecision d, const std::string& why) {
  out->cells.clear();
  out->need_first = false;
  out->reason = why;
  return d;
}

// the table of DESIGN.md 3.12: which logical type takes a program's return type
bool type_fits(uint32_t stype, uint32_t logical) {
  switch (stype) {
    case EVQL_T_UINT64: return logical == uint32_t(ColumnType::UNSIGNED_INT);
    case EVQL_T_TIMESTAMP64: return logical == uint32_t(ColumnType::DATETIME);
    case EVQL_T_FLOAT64: return logical == uint32_t(ColumnType::FLOAT);
    case EVQL_T_BOOL: return logical == uint32_t(ColumnType::BOOLEAN);
    case EVQL_T_STRING: return logical == uint32_t(ColumnType::STRING);
    default: return false;
  }
}

}  // namespace

int mat_decision_code(MatDecision d) {
  if (d == MAT_DEVICE) return EVQL_OK;
  return d < MAT_BARE_SCAN ? EVQL_EARG : EVQL_ENOTSUP;
}

MatDecision plan_materialize(const MatInput& in, MatPlan* out) {
  *out = MatPlan();
  const KernelPlan& kp = *in.kp;
  const std::vector<MatSpec>& specs = *in.specs;
  if (in.group_mode != EVQL_MODE_FINAL) {
    return refuse(out, MAT_PARTIAL_MODE, "materialise: the query runs in EVQL_MODE_PARTIAL");
  }
  if (kp.bare_scan) return refuse(out, MAT_BARE_SCAN, "materialise: a bare scan has no groups");
  if (in.ordered) return refuse(out, MAT_ORDER_LIMIT, "materialise: the query has ORDER BY / LIMIT set");
  const size_t nsel = in.select->size();
  if (specs.size() != nsel) {
    return refuse(out, MAT_COLUMN_COUNT, "materialise: " + std::to_string(specs.size()) +
                                             " column specs for " + std::to_string(nsel) +
                                             " select expressions");
  }
  if (nsel == 0 || nsel > kMaxMatCols) {
    return refuse(out, MAT_TOO_WIDE, "materialise: more than 32 columns (or none)");
  }
  if (in.sort_column < -1 || in.sort_column >= int(nsel)) {
    return refuse(out, MAT_SORT_COLUMN, "materialise: bad sort column");
  }
  for (const MatSpec& sp : specs) {
    if (sp.rlevel_max > 0 || sp.dlevel_max > 1) {
      return refuse(out, MAT_NESTED_SPEC, "materialise: a repeated / nested output column: " + sp.name);
    }
  }
  for (size_t i = 0; i < nsel; ++i) {
    const LoweredProgram& lp = (*in.select)[i];
    const MatSpec& sp = specs[i];
    MatCell cell;
    cell.optional = sp.dlevel_max == 1;
    cell.stype = lp.return_type;
    cell.is_bool = lp.return_type == EVQL_T_BOOL;
    if (lp.return_type == EVQL_T_NIL) {
      return refuse(out, MAT_NIL, "materialise: a NIL-typed column: " + sp.name);
    }
    if (lp.return_type == EVQL_T_INT64) {
      return refuse(out, MAT_INT64, "materialise: an INT64-typed column (cstable has no signed "
                                    "column here): " + sp.name);
    }
    if (lp.is_aggregate) {
      if (!lp.call || lp.call->kind != Expr::AGG_GET) {
        return refuse(out, MAT_POST_AGGREGATE, "materialise: post-aggregate arithmetic: " + sp.name);
      }
      const int ai = i < in.select_agg_index->size() ? (*in.select_agg_index)[i] : -1;
      const AggPlan* a = nullptr;
      if (!aggregate_cell(kp, ai, &cell, &a)) {
        return refuse(out, MAT_POST_AGGREGATE, "materialise: no aggregate state behind: " + sp.name);
      }
      if (a->exact_index >= 0) {
        return refuse(out, MAT_EXACT_SUM, "materialise: an exact float sum: " + sp.name);
      }
    } else if (i < in.select_passthrough->size() && (*in.select_passthrough)[i]) {
      // the exact key: the record's identity word (also after a merge).  A computed key
      // (`a + 1`) is refused like every other evaluated expression.  (The key mode must be
      // EXACT here; FINAL asks for no key mode.)
      uint32_t c = 0;
      if (kp.key_mode != KEY_EXACT || lp.return_type == EVQL_T_STRING ||
          !bare_column(kp, *in.scan_select, lp, &c)) {
        return refuse(out, MAT_KEY_EXPR, "materialise: a computed key: " + sp.name);
      }
      cell.kind = 0;
    } else {
      // a bare column read from the group's first row (the columns of a hashed key among them)
      uint32_t c = 0;
      if (!bare_column(kp, *in.scan_select, lp, &c) || !kp.need_first_row) {
        return refuse(out, MAT_KEY_EXPR, "materialise: a computed or hashed key or select expression "
                                         "that is not a first-row bare column: " + sp.name);
      }
      if (in.merged || in.nested) {
        return refuse(out, MAT_FIRST_ROW, std::string("materialise: a first-row column of a ") +
                                              (in.merged ? "merged result: " : "nested scan: ") + sp.name);
      }
      // (a STRING only from a hashed string column: FINAL does not ask)
      if (!first_row_cell(kp, *in.scan_select, lp, &cell) ||
          (lp.return_type == EVQL_T_STRING) != bool(cell.is_string)) {
        return refuse(out, MAT_KEY_EXPR, "materialise: the column's type is not the expression's: " + sp.name);
      }
      out->need_first = true;
    }
    if (!type_fits(lp.return_type, sp.logical_type)) {
      return refuse(out, MAT_TYPE_MISMATCH, "materialise: the select expression's type does not fit "
                                            "the column's logical type: " + sp.name);
    }
    out->cells.push_back(cell);
  }
  if (in.sort_column >= 0) {
    // the rule of sorted compaction (chain_compact_plan.cc plan_compact_sort_key)
    const MatSpec& sp = specs[in.sort_column];
    if (sp.dlevel_max > 0) {
      return refuse(out, MAT_SORT_KEY, "materialise: sort key is an optional column (NULLs have no "
                                       "place in the order): " + sp.name);
    }
    if (sp.logical_type != uint32_t(ColumnType::UNSIGNED_INT) &&
        sp.logical_type != uint32_t(ColumnType::DATETIME)) {
      return refuse(out, MAT_SORT_KEY, "materialise: sort key is not an unsigned-integer or datetime "
                                       "column: " + sp.name);
    }
    if (in.n > 0xffffffffull) {
      return refuse(out, MAT_SORT_ROWS, "materialise: a sort of more than 2^32 - 1 rows");
    }
  }
  return MAT_DEVICE;
}

}  // namespace evql
