// value_bounds.cc -- what the values of the scanned columns imply for a plan: the quantum
// of exact float sums and the tuple members that fit 32 bits.
#include <cmath>
#include <cstring>
#include <limits>
#include "runtime.h"

namespace evql {

// ---------------------------------------------------------------------------
// EVQL_FLOAT_SUM_EXACT: bound of |argument| and the quantum of every exact sum
// ---------------------------------------------------------------------------
// upper bound of |e| given upper bounds of |column i|; +inf = unknown
static double expr_abs_bound(const ExprPtr& e, const std::vector<double>& colmax) {
  const double inf = std::numeric_limits<double>::infinity();
  switch (e->kind) {
    case Expr::INPUT:
      return e->input < colmax.size() ? colmax[e->input] : inf;
    case Expr::LITERAL:
      switch (e->type) {
        case EVQL_T_UINT64: case EVQL_T_TIMESTAMP64: return double(e->lit_bits);
        case EVQL_T_INT64: return std::fabs(double(int64_t(e->lit_bits)));
        case EVQL_T_FLOAT64: {
          double d;
          memcpy(&d, &e->lit_bits, 8);
          return std::fabs(d);
        }
        case EVQL_T_BOOL: return 1.0;
        default: return inf;
      }
    case Expr::IF:
      return std::max(expr_abs_bound(e->args[1], colmax), expr_abs_bound(e->args[2], colmax));
    case Expr::CALL: {
      std::vector<double> b;
      for (const auto& a : e->args) b.push_back(expr_abs_bound(a, colmax));
      switch (e->family) {
        case EVQL_FAM_ADD: case EVQL_FAM_SUB: return b[0] + b[1];
        case EVQL_FAM_MUL: return b[0] * b[1];
        case EVQL_FAM_MOD: return b[0];
        case EVQL_FAM_DIV:
          if (e->type != EVQL_T_FLOAT64) return b[0];
          if (e->args[1]->kind == Expr::LITERAL) {
            double d;
            memcpy(&d, &e->args[1]->lit_bits, 8);
            if (d != 0.0) return b[0] / std::fabs(d);
          }
          return inf;
        case EVQL_FAM_TO_INT64: case EVQL_FAM_TO_TIMESTAMP64: return b[0];
        case EVQL_FAM_CMP: case EVQL_FAM_EQ: case EVQL_FAM_NEQ: case EVQL_FAM_LT:
        case EVQL_FAM_LTE: case EVQL_FAM_GT: case EVQL_FAM_GTE: case EVQL_FAM_LOGICAL_AND:
        case EVQL_FAM_LOGICAL_OR: case EVQL_FAM_NEG:
          return 1.0;
        default: return inf;
      }
    }
    default:
      return inf;
  }
}

// maximum |value| of scan column i as the kernel sees it (cached per table column)
Status column_abs_max(evql_query* q, size_t i, double* out) {
  evql_table* t = q->table;
  hipStream_t s = q->ctx->stream;
  const ColAccess& c = q->kp.cols[i];
  if (c.string_hash) {
    *out = std::numeric_limits<double>::infinity();
    return Status();
  }
  if (c.dict_code) {  // dense codes 0 .. n_codes - 1
    *out = double(t->dicts[c.name].n_codes - 1);
    return Status();
  }
  const bool is_float = c.stype == EVQL_T_FLOAT64 && !c.from_uint_to_float;
  const std::string key = c.name + (is_float ? "#f" : "#u");
  if (!q->nested) {
    auto hit = t->col_absmax.find(key);
    if (hit != t->col_absmax.end()) {
      *out = hit->second;
      return Status();
    }
  }
  RtColumn rc{};
  rc.pages = c.layout_index >= 0 ? t->d_pages[c.layout_index][0] : nullptr;
  rc.mode = c.mode;
  rc.bits = c.bits;
  uint64_t n = t->layout.num_rows;
  if (q->nested) {
    rc.mode = ColAccess::SOA;  // (the 8-byte words stay beside a packed copy)
    rc.soa = q->nested_flat[i];
    n = q->nested_rows;
  } else if (c.mode == ColAccess::NARROW_F32) {
    rc.mode = ColAccess::PLAIN64;  // (the file's pages hold the same values)
    rc.bits = 0;
  } else if (c.packed) {
    const MaterializedColumn& m = t->materialized[c.name];
    rc.pages = nullptr;  // (a flat array: ColAccess::NARROW)
    rc.base = m.d_packed;
  } else if (c.mode == ColAccess::SOA) {
    rc.soa = t->materialized[c.name].d_values;
  }
  DevBuf<uint64_t> d_max;
  HIP_TRY(d_max.alloc(8));
  HIP_TRY(hipMemsetAsync(d_max, 0, 8, s));
  HIP_TRY(launch_column_abs_max(t->d_image, rc, n, is_float ? 1 : 0, d_max, s));
  uint64_t bits = 0;
  HIP_TRY(hipMemcpyAsync(&bits, d_max, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  double m;
  if (is_float) {
    memcpy(&m, &bits, 8);  // (NaN / inf order above every finite |x| as integers)
    if (!(m == m)) m = std::numeric_limits<double>::infinity();
  } else {
    m = double(bits);
  }
  if (!q->nested) t->col_absmax[key] = m;
  *out = m;
  return Status();
}

Status choose_exact_sum_scales(evql_query* q) {
  std::vector<double> colmax(q->kp.cols.size(), std::numeric_limits<double>::infinity());
  bool have = false;
  for (const auto& a : q->kp.aggs) {
    if (a.exact_index < 0) continue;
    double bound = q->float_sum_bound;
    if (!(bound > 0)) {
      if (!have) {
        for (size_t i = 0; i < colmax.size(); ++i) {
          Status st = column_abs_max(q, i, &colmax[i]);
          if (!st.ok()) return st;
        }
        have = true;
      }
      bound = a.arg ? expr_abs_bound(a.arg, colmax) : 0.0;
      if (!std::isfinite(bound)) {
        return Status::error(EVQL_ENOTSUP, "exact float sum: no finite bound of the argument "
                                           "follows from the table; pass float_sum_bound");
      }
    }
    // quantum 2^e with bound * 2^-e < 2^61: |q| < 2^61, the high parts (|q| >> 31
    // < 2^30) and the low parts (< 2^31) of up to 2^32 rows add up inside 64 bits.
    // e >= -1023 keeps the kernel's scale 2^-e finite (a bound below 2^-962 would make
    // it +inf); terms of magnitude <= 2^-1024 then round to 0, and a subnormal total is
    // -1, 0 or 1 quantum, which exact_sum_value scales without a second rounding
    int ex = 0;
    std::frexp(bound > 0 ? bound : 1.0, &ex);  // bound < 2^ex
    q->fsum_exp[a.exact_index] = std::max(ex - 61, -1023);
    q->fsum_bound[a.exact_index] = bound;
  }
  return Status();
}

// ---------------------------------------------------------------------------
// partitioned path: which tuple members fit 32 bits
// ---------------------------------------------------------------------------
// upper bound of the unsigned value of e given upper bounds of the columns; +inf where
// the value may wrap or is not an unsigned integer
static double expr_unsigned_bound(const ExprPtr& e, const std::vector<double>& colmax) {
  const double inf = std::numeric_limits<double>::infinity();
  const bool uns = e->type == EVQL_T_UINT64 || e->type == EVQL_T_TIMESTAMP64 || e->type == EVQL_T_BOOL;
  if (!uns) return inf;
  switch (e->kind) {
    case Expr::INPUT:
      return e->input < colmax.size() ? colmax[e->input] : inf;
    case Expr::LITERAL:
      return e->type == EVQL_T_BOOL ? 1.0 : double(e->lit_bits);
    case Expr::IF:
      return std::max(expr_unsigned_bound(e->args[1], colmax), expr_unsigned_bound(e->args[2], colmax));
    case Expr::CALL: {
      if (e->type == EVQL_T_BOOL) return 1.0;
      std::vector<double> b;
      for (const auto& a : e->args) b.push_back(expr_unsigned_bound(a, colmax));
      switch (e->family) {
        case EVQL_FAM_ADD: return b[0] + b[1];  // (< 2^53: exact in a double; larger sums
        case EVQL_FAM_MUL: return b[0] * b[1];  //  are far beyond the 2^32 threshold)
        case EVQL_FAM_MOD: case EVQL_FAM_DIV: return b[0];
        default: return inf;
      }
    }
    default:
      return inf;
  }
}

// Sets narrow_ident / narrow_first_row / AggPlan::narrow_arg from the maxima of the
// referenced columns (one streaming pass per table column, cached): a member that
// provably stays below 2^32 - 1 travels as 4 bytes through scatter / refine / aggregate.
Status choose_tuple_widths(evql_query* q) {
  KernelPlan& kp = q->kp;
  const double lim = 4294967295.0;  // strictly below: 32 ones are a minimum's identity
  std::vector<double> colmax(kp.cols.size(), std::numeric_limits<double>::infinity());
  for (size_t i = 0; i < colmax.size(); ++i) {
    const ColAccess& c = kp.cols[i];
    if (c.string_hash || (c.stype == EVQL_T_FLOAT64 && !c.from_uint_to_float)) continue;
    if (c.stype != EVQL_T_UINT64 && c.stype != EVQL_T_TIMESTAMP64 && c.stype != EVQL_T_BOOL) continue;
    Status st = column_abs_max(q, i, &colmax[i]);
    if (!st.ok()) return st;
  }
  kp.narrow_ident = kp.key_mode == KEY_EXACT && expr_unsigned_bound(kp.group[0], colmax) < lim;
  const uint64_t nrows = q->nested ? q->nested_rows : q->table->layout.num_rows;
  kp.narrow_first_row = nrows < (1ull << 32);
  for (auto& a : kp.aggs) {
    a.narrow_arg = a.arg && expr_unsigned_bound(a.arg, colmax) < lim;
  }
  return Status();
}

}  // namespace evql
