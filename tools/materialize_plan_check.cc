// materialize_plan_check.cc -- the host-only part of materialising a GROUP BY result as a
// resident cstable (which queries qualify, what every output column is read from:
// eventql_amd/csrc/materialize_plan.cc) exercised on its own, so that it can run under
// AddressSanitizer / UBSan without a device or the HIP runtime:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I eventql_amd/csrc tools/materialize_plan_check.cc \
//       eventql_amd/csrc/materialize_plan.cc -o /tmp/materialize_plan_check
//
// Exit status 0 and "ok" when every expectation holds.
#include <cstdio>
#include <cstdlib>
#include "codegen.h"
#include "materialize_plan.h"

using namespace evql;

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      ++failures;                                                 \
    }                                                             \
  } while (0)

static ExprPtr input(uint32_t i, uint32_t type) {
  ExprPtr e = std::make_shared<Expr>();
  e->kind = Expr::INPUT;
  e->input = i;
  e->type = type;
  return e;
}

static ExprPtr call1(ExprPtr arg, uint32_t type) {
  ExprPtr e = std::make_shared<Expr>();
  e->kind = Expr::CALL;
  e->type = type;
  e->args.push_back(arg);
  return e;
}

static LoweredProgram prog(ExprPtr e, uint32_t type) {
  LoweredProgram p;
  p.call = e;
  p.return_type = type;
  return p;
}

static LoweredProgram agg(uint32_t fn, uint32_t type) {
  LoweredProgram p;
  p.call = std::make_shared<Expr>();
  p.call->kind = Expr::AGG_GET;
  p.call->type = type;
  p.is_aggregate = true;
  p.aggregate_fn = fn;
  p.return_type = type;
  return p;
}

static uint32_t logical_of(uint32_t stype) {
  switch (stype) {
    case EVQL_T_UINT64: return uint32_t(ColumnType::UNSIGNED_INT);
    case EVQL_T_TIMESTAMP64: return uint32_t(ColumnType::DATETIME);
    case EVQL_T_FLOAT64: return uint32_t(ColumnType::FLOAT);
    case EVQL_T_BOOL: return uint32_t(ColumnType::BOOLEAN);
    case EVQL_T_STRING: return uint32_t(ColumnType::STRING);
    default: return uint32_t(ColumnType::SIGNED_INT);
  }
}

static uint32_t agg_type(uint32_t fn) {
  switch (fn) {
    case EVQL_AGG_SUM_INT64: case EVQL_AGG_MIN_INT64: case EVQL_AGG_MAX_INT64: return EVQL_T_INT64;
    case EVQL_AGG_SUM_FLOAT64: case EVQL_AGG_MIN_FLOAT64: case EVQL_AGG_MAX_FLOAT64:
    case EVQL_AGG_MEAN_UINT64: case EVQL_AGG_MEAN_INT64: case EVQL_AGG_MEAN_FLOAT64:
      return EVQL_T_FLOAT64;
    default: return EVQL_T_UINT64;
  }
}

// a query over scan columns 0 u (UINT64), 1 s (STRING), 2 b (BOOL), 3 f (FLOAT64 over a uint
// column), 4 t (TIMESTAMP64); the scan select list reads them one to one, entry 5 is computed
struct Fixture {
  KernelPlan kp;
  std::vector<LoweredProgram> scan_select, select;
  std::vector<int> agg_index;
  std::vector<bool> passthrough;
  std::vector<MatSpec> specs;
  MatInput in;

  Fixture() {
    const uint32_t types[5] = {EVQL_T_UINT64, EVQL_T_STRING, EVQL_T_BOOL, EVQL_T_FLOAT64,
                               EVQL_T_TIMESTAMP64};
    for (int i = 0; i < 5; ++i) {
      ColAccess c;
      c.name = "c" + std::to_string(i);
      c.stype = types[i];
      c.string_hash = types[i] == EVQL_T_STRING;
      c.from_uint_to_float = i == 3;
      c.layout_index = i;
      kp.cols.push_back(c);
      scan_select.push_back(prog(input(uint32_t(i), types[i]), types[i]));
    }
    scan_select.push_back(prog(call1(input(0, EVQL_T_UINT64), EVQL_T_UINT64), EVQL_T_UINT64));
    in.group_mode = EVQL_MODE_FINAL;
  }
  // group by the scan select entries `keys`; select them, then the aggregates `fns`; the
  // specs fit the types, optional where the cell can be NULL
  void plan(const std::vector<uint32_t>& keys, const std::vector<uint32_t>& fns) {
    select.clear();
    agg_index.clear();
    passthrough.clear();
    specs.clear();
    kp.aggs.clear();
    kp.states.clear();
    bool exact = keys.size() == 1;
    for (uint32_t j : keys) exact = exact && scan_select[j].return_type != EVQL_T_STRING;
    kp.key_mode = keys.empty() ? KEY_NONE : (exact ? KEY_EXACT : KEY_HASHED);
    kp.need_first_row = !exact && !keys.empty();
    for (uint32_t j : keys) {
      const uint32_t t = scan_select[j].return_type;
      select.push_back(prog(input(j, t), t));
      agg_index.push_back(-1);
      passthrough.push_back(exact);
      specs.push_back(MatSpec{"k" + std::to_string(j), logical_of(t), 0, 1});
    }
    for (uint32_t fn : fns) {
      AggPlan a;
      a.fn = fn;
      a.first_word = int(kp.states.size());
      a.nwords = fn >= EVQL_AGG_MIN_UINT64 && fn <= EVQL_AGG_MEAN_FLOAT64 ? 2 : 1;
      for (int w = 0; w < a.nwords; ++w) kp.states.push_back(StateWord{0});
      select.push_back(agg(fn, agg_type(fn)));
      agg_index.push_back(int(kp.aggs.size()));
      passthrough.push_back(false);
      specs.push_back(MatSpec{"a" + std::to_string(kp.aggs.size()), logical_of(agg_type(fn)), 0,
                              a.nwords == 2 ? 1u : 0u});
      kp.aggs.push_back(a);
    }
  }
  MatDecision decide(MatPlan* out) {
    in.kp = &kp;
    in.scan_select = &scan_select;
    in.select = &select;
    in.select_agg_index = &agg_index;
    in.select_passthrough = &passthrough;
    in.specs = &specs;
    return plan_materialize(in, out);
  }
};

int main() {
  MatPlan p;
  {
    // one exact key; count, an integer sum, a fast float sum, count_distinct, min / max / mean
    Fixture f;
    f.plan({0}, {EVQL_AGG_COUNT, EVQL_AGG_SUM_UINT64, EVQL_AGG_SUM_FLOAT64,
                 EVQL_AGG_COUNT_DISTINCT_UINT64, EVQL_AGG_MIN_UINT64, EVQL_AGG_MAX_FLOAT64,
                 EVQL_AGG_MEAN_UINT64});
    EXPECT(f.decide(&p) == MAT_DEVICE && p.reason.empty());
    EXPECT(p.cells.size() == 8 && p.cells[0].kind == 0 && p.cells[0].optional == 1 && !p.need_first);
    // record words: kind, identity, then the states
    EXPECT(p.cells[1].kind == 1 && p.cells[1].word == 2 && p.cells[1].count_word == -1);
    EXPECT(p.cells[4].word == 5 && p.cells[5].word == 6 && p.cells[5].count_word == 7 && !p.cells[5].is_mean);
    EXPECT(p.cells[6].word == 8 && p.cells[7].word == 10 && p.cells[7].count_word == 11 &&
           p.cells[7].is_mean == 1 && p.cells[7].optional == 1);
    EXPECT(mat_decision_code(MAT_DEVICE) == EVQL_OK);
    // a merged result with an exact key qualifies
    f.in.merged = true;
    EXPECT(f.decide(&p) == MAT_DEVICE);
    f.in.merged = false;
    // modes and switches
    f.in.group_mode = EVQL_MODE_PARTIAL;
    EXPECT(f.decide(&p) == MAT_PARTIAL_MODE && p.cells.empty() && !p.reason.empty());
    EXPECT(mat_decision_code(MAT_PARTIAL_MODE) == EVQL_EARG);
    f.in.group_mode = EVQL_MODE_FINAL;
    f.in.ordered = true;
    EXPECT(f.decide(&p) == MAT_ORDER_LIMIT && mat_decision_code(MAT_ORDER_LIMIT) == EVQL_ENOTSUP);
    f.in.ordered = false;
    f.kp.bare_scan = true;
    EXPECT(f.decide(&p) == MAT_BARE_SCAN && mat_decision_code(MAT_BARE_SCAN) == EVQL_ENOTSUP);
    f.kp.bare_scan = false;
    // specs: their number, nesting, types
    f.specs.pop_back();
    EXPECT(f.decide(&p) == MAT_COLUMN_COUNT && mat_decision_code(MAT_COLUMN_COUNT) == EVQL_EARG);
    f.plan({0}, {EVQL_AGG_COUNT});
    f.specs[1].rlevel_max = 1;
    EXPECT(f.decide(&p) == MAT_NESTED_SPEC);
    f.specs[1].rlevel_max = 0;
    f.specs[1].dlevel_max = 2;
    EXPECT(f.decide(&p) == MAT_NESTED_SPEC && mat_decision_code(MAT_NESTED_SPEC) == EVQL_EARG);
    f.specs[1].dlevel_max = 0;
    f.specs[1].logical_type = uint32_t(ColumnType::FLOAT);
    EXPECT(f.decide(&p) == MAT_TYPE_MISMATCH && mat_decision_code(MAT_TYPE_MISMATCH) == EVQL_EARG);
    f.specs[1].logical_type = uint32_t(ColumnType::DATETIME);
    EXPECT(f.decide(&p) == MAT_TYPE_MISMATCH);
    f.specs[1].logical_type = uint32_t(ColumnType::UNSIGNED_INT);
    EXPECT(f.decide(&p) == MAT_DEVICE);
  }
  {
    // refused aggregates and types
    Fixture f;
    f.plan({0}, {EVQL_AGG_SUM_FLOAT64});
    f.kp.aggs[0].exact_index = 0;
    EXPECT(f.decide(&p) == MAT_EXACT_SUM);
    f.plan({0}, {EVQL_AGG_SUM_UINT64});
    f.select[1].call = call1(f.select[1].call, EVQL_T_UINT64);  // sum(a) + 1
    EXPECT(f.decide(&p) == MAT_POST_AGGREGATE);
    f.plan({0}, {EVQL_AGG_COUNT});
    f.agg_index[1] = 7;  // (an index outside the plan's aggregates is refused, not read)
    EXPECT(f.decide(&p) == MAT_POST_AGGREGATE);
    f.agg_index.clear();  // (a short index list too)
    EXPECT(f.decide(&p) == MAT_POST_AGGREGATE);
    f.plan({0}, {EVQL_AGG_SUM_INT64});
    EXPECT(f.decide(&p) == MAT_INT64 && mat_decision_code(MAT_INT64) == EVQL_ENOTSUP);
    f.plan({0}, {EVQL_AGG_MIN_INT64});
    EXPECT(f.decide(&p) == MAT_INT64);
    f.plan({0}, {EVQL_AGG_COUNT});
    f.select[1].return_type = EVQL_T_NIL;
    EXPECT(f.decide(&p) == MAT_NIL);
    // a computed exact key
    f.plan({5}, {EVQL_AGG_COUNT});
    EXPECT(f.decide(&p) == MAT_KEY_EXPR && mat_decision_code(MAT_KEY_EXPR) == EVQL_ENOTSUP);
  }
  {
    // hashed keys: bare columns of the first row
    Fixture f;
    f.plan({0, 1, 2, 3, 4}, {EVQL_AGG_COUNT});
    EXPECT(f.decide(&p) == MAT_DEVICE && p.need_first && p.cells.size() == 6);
    EXPECT(p.cells[0].kind == 2 && p.cells[0].src == 0 && !p.cells[0].is_string && !p.cells[0].is_bool);
    EXPECT(p.cells[1].is_string == 1 && p.cells[2].is_bool == 1 && p.cells[3].to_float == 1);
    EXPECT(p.cells[4].src == 4 && p.cells[5].kind == 1 && p.cells[5].word == 4);
    // ... not out of merged records, not of a nested scan
    f.in.merged = true;
    EXPECT(f.decide(&p) == MAT_FIRST_ROW && !p.need_first);
    f.in.merged = false;
    f.in.nested = true;
    EXPECT(f.decide(&p) == MAT_FIRST_ROW && mat_decision_code(MAT_FIRST_ROW) == EVQL_ENOTSUP);
    f.in.nested = false;
    // a computed key beside a bare one
    f.plan({0, 5}, {EVQL_AGG_COUNT});
    EXPECT(f.decide(&p) == MAT_KEY_EXPR);
    // a scan select index / a column index outside the lists
    f.plan({0, 1}, {EVQL_AGG_COUNT});
    f.select[1].call->input = 99;
    EXPECT(f.decide(&p) == MAT_KEY_EXPR);
    f.plan({0, 1}, {EVQL_AGG_COUNT});
    f.scan_select[1].call->input = 99;
    EXPECT(f.decide(&p) == MAT_KEY_EXPR);
    f.scan_select[1].call->input = 1;
    // the column's type is not the expression's
    f.kp.cols[1].stype = EVQL_T_UINT64;
    EXPECT(f.decide(&p) == MAT_KEY_EXPR);
  }
  {
    // a first-row column beside an exact key
    Fixture f;
    f.plan({0}, {EVQL_AGG_COUNT});
    f.kp.need_first_row = true;
    f.select.push_back(prog(input(1, EVQL_T_STRING), EVQL_T_STRING));
    f.agg_index.push_back(-1);
    f.passthrough.push_back(false);
    f.specs.push_back(MatSpec{"s", uint32_t(ColumnType::STRING), 0, 0});
    EXPECT(f.decide(&p) == MAT_DEVICE && p.need_first && p.cells[2].kind == 2 && p.cells[2].src == 1);
    EXPECT(p.cells[1].word == 3 && p.cells[2].optional == 0);  // kind, identity, first row, state
    f.in.merged = true;
    EXPECT(f.decide(&p) == MAT_FIRST_ROW);
    f.in.merged = false;
    f.select[2] = prog(input(5, EVQL_T_UINT64), EVQL_T_UINT64);  // computed
    EXPECT(f.decide(&p) == MAT_KEY_EXPR);
  }
  {
    // width
    Fixture f;
    f.plan({0}, std::vector<uint32_t>(kMaxMatCols - 1, EVQL_AGG_COUNT));
    EXPECT(f.decide(&p) == MAT_DEVICE && p.cells.size() == kMaxMatCols);
    f.plan({0}, std::vector<uint32_t>(kMaxMatCols, EVQL_AGG_COUNT));
    EXPECT(f.decide(&p) == MAT_TOO_WIDE && mat_decision_code(MAT_TOO_WIDE) == EVQL_ENOTSUP);
  }
  {
    // the sort column
    Fixture f;
    f.plan({0}, {EVQL_AGG_COUNT, EVQL_AGG_MAX_UINT64, EVQL_AGG_SUM_FLOAT64});
    f.specs[0].dlevel_max = 0;
    for (int sc : {-1, 0, 1}) {
      f.in.sort_column = sc;
      EXPECT(f.decide(&p) == MAT_DEVICE);
    }
    for (int sc : {-2, 4, 1000}) {
      f.in.sort_column = sc;
      EXPECT(f.decide(&p) == MAT_SORT_COLUMN && mat_decision_code(MAT_SORT_COLUMN) == EVQL_EARG);
    }
    f.in.sort_column = 2;  // optional
    EXPECT(f.decide(&p) == MAT_SORT_KEY && mat_decision_code(MAT_SORT_KEY) == EVQL_ENOTSUP);
    f.in.sort_column = 3;  // float
    EXPECT(f.decide(&p) == MAT_SORT_KEY);
    f.in.sort_column = 0;
    f.specs[0].dlevel_max = 1;
    EXPECT(f.decide(&p) == MAT_SORT_KEY);
    f.specs[0].dlevel_max = 0;
    f.in.n = 0xffffffffull;
    EXPECT(f.decide(&p) == MAT_DEVICE);
    f.in.n = 0x100000000ull;
    EXPECT(f.decide(&p) == MAT_SORT_ROWS && mat_decision_code(MAT_SORT_ROWS) == EVQL_ENOTSUP);
    f.in.sort_column = -1;
    EXPECT(f.decide(&p) == MAT_DEVICE);
    // a datetime key sorts, a string key does not
    Fixture g;
    g.plan({4}, {EVQL_AGG_COUNT});
    g.specs[0].dlevel_max = 0;
    g.in.sort_column = 0;
    EXPECT(g.decide(&p) == MAT_DEVICE);
    g.plan({1}, {EVQL_AGG_COUNT});
    g.specs[0].dlevel_max = 0;
    EXPECT(g.decide(&p) == MAT_SORT_KEY);
  }
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
