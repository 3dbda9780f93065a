// partial_emit_plan_check.cc -- the host-only part of packing EVQL_MODE_PARTIAL rows on the
// device (which plans qualify, what every cell is read from: eventql_amd/csrc/
// partial_emit_plan.cc) exercised on its own, so that it can run under AddressSanitizer / UBSan
// without a device or the HIP runtime:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I eventql_amd/csrc tools/partial_emit_plan_check.cc \
//       eventql_amd/csrc/partial_emit_plan.cc -o /tmp/partial_emit_plan_check
//
// Exit status 0 and "ok" when every expectation holds.
#include <cstdio>
#include <cstdlib>
#include "codegen.h"
#include "partial_emit_plan.h"

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

// a query over scan columns 0 u (UINT64), 1 s (STRING), 2 b (BOOL), 3 f (FLOAT64 over a uint
// column); the scan select list reads them one to one, entry 4 is computed (u + 1)
struct Fixture {
  KernelPlan kp;
  std::vector<LoweredProgram> scan_select, group, select;
  std::vector<int> agg_index;
  std::vector<bool> passthrough;
  PartialEmitInput in;

  Fixture() {
    const uint32_t types[4] = {EVQL_T_UINT64, EVQL_T_STRING, EVQL_T_BOOL, EVQL_T_FLOAT64};
    for (int i = 0; i < 4; ++i) {
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
    in.group_mode = EVQL_MODE_PARTIAL;
    in.n = kDeviceEmitMinGroups;
  }
  // group by the scan select entries `keys`; select them, then the aggregates `fns`
  void plan(const std::vector<uint32_t>& keys, const std::vector<uint32_t>& fns) {
    group.clear();
    select.clear();
    agg_index.clear();
    passthrough.clear();
    kp.aggs.clear();
    kp.states.clear();
    bool exact = keys.size() == 1;
    for (uint32_t j : keys) exact = exact && scan_select[j].return_type != EVQL_T_STRING;
    kp.key_mode = exact ? KEY_EXACT : KEY_HASHED;
    kp.need_first_row = !exact;
    for (uint32_t j : keys) {
      const uint32_t t = scan_select[j].return_type;
      group.push_back(prog(input(j, t), t));
      select.push_back(prog(input(j, t), t));
      agg_index.push_back(-1);
      passthrough.push_back(exact);
    }
    for (uint32_t fn : fns) {
      AggPlan a;
      a.fn = fn;
      a.first_word = int(kp.states.size());
      a.nwords = fn >= EVQL_AGG_MIN_UINT64 && fn <= EVQL_AGG_MEAN_FLOAT64 ? 2 : 1;
      for (int w = 0; w < a.nwords; ++w) kp.states.push_back(StateWord{0});
      select.push_back(agg(fn, EVQL_T_UINT64));
      agg_index.push_back(int(kp.aggs.size()));
      passthrough.push_back(false);
      kp.aggs.push_back(a);
    }
  }
  PartialEmitDecision decide(PartialEmitPlan* out) {
    in.kp = &kp;
    in.scan_select = &scan_select;
    in.group = &group;
    in.select = &select;
    in.select_agg_index = &agg_index;
    in.select_passthrough = &passthrough;
    return plan_partial_emit(in, out);
  }
};

int main() {
  PartialEmitPlan p;
  {
    // one exact key; count, integer sums, a fast float sum, min / max / mean
    Fixture f;
    f.plan({0}, {EVQL_AGG_COUNT, EVQL_AGG_SUM_UINT64, EVQL_AGG_SUM_INT64, EVQL_AGG_SUM_FLOAT64,
                 EVQL_AGG_MIN_UINT64, EVQL_AGG_MAX_FLOAT64, EVQL_AGG_MEAN_INT64});
    EXPECT(f.decide(&p) == PEMIT_DEVICE);
    EXPECT(p.tuple.size() == 1 && p.tuple[0].kind == 0 && p.tuple[0].stype == EVQL_T_UINT64);
    EXPECT(p.data.size() == 8 && p.data[0].kind == 0 && !p.need_first);
    // record words: kind, identity, then the states
    EXPECT(p.data[1].kind == 1 && p.data[1].word == 2 && p.data[1].state == PSTATE_VARUINT);
    EXPECT(p.data[3].state == PSTATE_VARUINT && p.data[4].state == PSTATE_RAW8 && p.data[4].word == 5);
    EXPECT(p.data[5].state == PSTATE_COUNT_RAW8 && p.data[5].word == 6);
    EXPECT(p.data[6].word == 8 && p.data[7].word == 10 && p.data[7].state == PSTATE_COUNT_RAW8);
    // the thresholds and switches
    f.in.n = kDeviceEmitMinGroups - 1;
    EXPECT(f.decide(&p) == PEMIT_FEW_GROUPS && p.tuple.empty() && p.data.empty());
    f.in.n = kDeviceEmitMinGroups;
    f.in.group_mode = EVQL_MODE_FINAL;
    EXPECT(f.decide(&p) == PEMIT_NOT_PARTIAL);
    f.in.group_mode = EVQL_MODE_PARTIAL;
    f.in.enabled = false;
    EXPECT(f.decide(&p) == PEMIT_SWITCHED_OFF);
    f.in.enabled = true;
    f.in.nested = true;
    EXPECT(f.decide(&p) == PEMIT_NESTED);
    f.in.nested = false;
    // a merged result with an exact key qualifies
    f.in.merged = true;
    EXPECT(f.decide(&p) == PEMIT_DEVICE);
  }
  {
    // refused aggregates
    Fixture f;
    f.plan({0}, {EVQL_AGG_COUNT, EVQL_AGG_COUNT_DISTINCT_UINT64});
    EXPECT(f.decide(&p) == PEMIT_AGGREGATE);
    f.plan({0}, {EVQL_AGG_SUM_FLOAT64});
    f.kp.aggs[0].exact_index = 0;
    EXPECT(f.decide(&p) == PEMIT_AGGREGATE);
    f.plan({0}, {EVQL_AGG_COUNT});
    f.agg_index[1] = 7;  // (an index outside the plan's aggregates is refused, not read)
    EXPECT(f.decide(&p) == PEMIT_AGGREGATE);
  }
  {
    // hashed keys: bare columns of the first row, the LAST group expression first
    Fixture f;
    f.plan({0, 1, 2, 3}, {EVQL_AGG_COUNT});
    EXPECT(f.decide(&p) == PEMIT_DEVICE && p.need_first);
    EXPECT(p.tuple.size() == 4 && p.tuple[0].src == 3 && p.tuple[3].src == 0);
    EXPECT(p.tuple[0].to_float == 1 && p.tuple[1].is_bool == 1 && p.tuple[2].is_string == 1);
    EXPECT(p.tuple[3].kind == 2 && !p.tuple[3].is_string && !p.tuple[3].is_bool);
    EXPECT(p.data.size() == 5 && p.data[1].is_string == 1 && p.data[4].word == 4);
    // a string key alone
    f.plan({1}, {EVQL_AGG_COUNT});
    EXPECT(f.decide(&p) == PEMIT_DEVICE && p.tuple[0].is_string == 1);
    // ... not out of merged records
    f.in.merged = true;
    EXPECT(f.decide(&p) == PEMIT_GROUP_EXPR);
    f.in.merged = false;
    // a computed key, alone and beside a bare one
    f.plan({4}, {EVQL_AGG_COUNT});
    EXPECT(f.decide(&p) == PEMIT_GROUP_EXPR);
    f.plan({0, 4}, {EVQL_AGG_COUNT});
    EXPECT(f.decide(&p) == PEMIT_GROUP_EXPR);
    // a scan select index / a column index outside the lists
    f.plan({0, 1}, {EVQL_AGG_COUNT});
    f.group[1].call->input = 99;
    EXPECT(f.decide(&p) == PEMIT_GROUP_EXPR);
    f.plan({0, 1}, {EVQL_AGG_COUNT});
    f.scan_select[1].call->input = 99;
    EXPECT(f.decide(&p) == PEMIT_GROUP_EXPR);
    f.scan_select[1].call->input = 1;
    // the column's type is not the expression's
    f.kp.cols[1].stype = EVQL_T_UINT64;
    EXPECT(f.decide(&p) == PEMIT_GROUP_EXPR);
  }
  {
    // non-aggregate select expressions beside an exact key
    Fixture f;
    f.plan({0}, {EVQL_AGG_COUNT});
    f.kp.need_first_row = true;
    f.select.push_back(prog(input(1, EVQL_T_STRING), EVQL_T_STRING));
    f.agg_index.push_back(-1);
    f.passthrough.push_back(false);
    EXPECT(f.decide(&p) == PEMIT_DEVICE && p.need_first && p.data[2].kind == 2 && p.data[2].src == 1);
    // word of the count: kind, identity, first row, state
    EXPECT(p.data[1].word == 3);
    f.in.merged = true;
    EXPECT(f.decide(&p) == PEMIT_SELECT_EXPR);
    f.in.merged = false;
    f.select[2] = prog(input(4, EVQL_T_UINT64), EVQL_T_UINT64);  // computed
    EXPECT(f.decide(&p) == PEMIT_SELECT_EXPR);
    f.select[2] = prog(input(0, EVQL_T_NIL), EVQL_T_NIL);
    EXPECT(f.decide(&p) == PEMIT_NIL_COLUMN);
  }
  {
    // width
    Fixture f;
    f.plan({0}, std::vector<uint32_t>(kMaxEmitCols - 1, EVQL_AGG_COUNT));
    EXPECT(f.kp.states.size() == kMaxEmitCols - 1 && f.decide(&p) == PEMIT_DEVICE);
    f.plan({0}, std::vector<uint32_t>(kMaxEmitCols, EVQL_AGG_COUNT));
    EXPECT(f.decide(&p) == PEMIT_TOO_WIDE);
    f.plan({}, {EVQL_AGG_COUNT});
    EXPECT(f.decide(&p) == PEMIT_TOO_WIDE);
  }
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
