// order_sort_plan_check.cc -- the host-only part of ORDER BY sorted on the device (which
// results qualify, where every sort key is read from: eventql_amd/csrc/order_sort_plan.cc)
// exercised on its own, so that it can run under AddressSanitizer / UBSan without a device or
// the HIP runtime:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I eventql_amd/csrc tools/order_sort_plan_check.cc \
//       eventql_amd/csrc/order_sort_plan.cc -o /tmp/order_sort_plan_check
//
// Exit status 0 and "ok" when every expectation holds.
#include <cstdio>
#include <cstdlib>
#include "codegen.h"
#include "order_sort_plan.h"
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

static LoweredProgram prog(ExprPtr e, uint32_t type) {
  LoweredProgram p;
  p.call = e;
  p.return_type = type;
  return p;
}

// select list: 0 the key (passthrough, `key_type`), then one bare aggregate per entry of
// `fns`, then `sum + 1` (post-aggregate arithmetic) and a first-row string column
struct Fixture {
  KernelPlan kp;
  std::vector<LoweredProgram> select, order;
  std::vector<int> agg_index;
  std::vector<bool> passthrough, desc;
  OrderSortInput in;
  uint32_t arith = 0, first_row_string = 0;

  Fixture(uint32_t key_type, const std::vector<uint32_t>& fns, const std::vector<uint32_t>& types,
          bool need_first_row = false, int exact = -1) {
    kp.key_mode = KEY_EXACT;
    kp.need_first_row = need_first_row;
    select.push_back(prog(input(0, key_type), key_type));
    agg_index.push_back(-1);
    passthrough.push_back(true);
    for (size_t i = 0; i < fns.size(); ++i) {
      AggPlan a;
      a.fn = fns[i];
      a.first_word = int(kp.states.size());
      a.nwords = fns[i] >= EVQL_AGG_MIN_UINT64 && fns[i] <= EVQL_AGG_MEAN_FLOAT64 ? 2 : 1;
      if (int(i) == exact) a.exact_index = 0;
      for (int w = 0; w < a.nwords; ++w) kp.states.push_back(StateWord{0});
      LoweredProgram p;
      p.call = std::make_shared<Expr>();
      p.call->kind = Expr::AGG_GET;
      p.call->type = types[i];
      p.is_aggregate = true;
      p.aggregate_fn = fns[i];
      p.return_type = types[i];
      select.push_back(p);
      agg_index.push_back(int(kp.aggs.size()));
      passthrough.push_back(false);
      kp.aggs.push_back(a);
    }
    // sum + 1: an aggregate program whose call is not a bare AGG_GET
    {
      LoweredProgram p = select[1];
      ExprPtr c = std::make_shared<Expr>();
      c->kind = Expr::CALL;
      c->type = p.return_type;
      c->args.push_back(p.call);
      p.call = c;
      arith = uint32_t(select.size());
      select.push_back(p);
      agg_index.push_back(0);
      passthrough.push_back(false);
    }
    first_row_string = uint32_t(select.size());
    select.push_back(prog(input(1, EVQL_T_STRING), EVQL_T_STRING));
    agg_index.push_back(-1);
    passthrough.push_back(false);
    in.group_mode = EVQL_MODE_FINAL;
    in.n = kDeviceEmitMinGroups;
  }
  void by(const std::vector<std::pair<uint32_t, bool>>& specs) {
    order.clear();
    desc.clear();
    for (const auto& s : specs) {
      order.push_back(prog(input(s.first, select[s.first].return_type), select[s.first].return_type));
      desc.push_back(s.second);
    }
  }
  OrderSortDecision decide(OrderSortPlan* out) {
    in.kp = &kp;
    in.select = &select;
    in.select_agg_index = &agg_index;
    in.select_passthrough = &passthrough;
    in.order = &order;
    in.order_desc = &desc;
    return plan_order_sort(in, out);
  }
};

int main() {
  OrderSortPlan p;
  const std::vector<uint32_t> fns = {EVQL_AGG_COUNT, EVQL_AGG_SUM_INT64, EVQL_AGG_SUM_FLOAT64,
                                     EVQL_AGG_MIN_INT64, EVQL_AGG_MEAN_FLOAT64,
                                     EVQL_AGG_COUNT_DISTINCT_UINT64, EVQL_AGG_MAX_FLOAT64};
  const std::vector<uint32_t> types = {EVQL_T_UINT64, EVQL_T_INT64, EVQL_T_FLOAT64, EVQL_T_INT64,
                                       EVQL_T_FLOAT64, EVQL_T_UINT64, EVQL_T_FLOAT64};
  {
    // every accepted column, as the first spec and behind it; record words: kind, identity,
    // then the states
    Fixture f(EVQL_T_UINT64, fns, types);
    f.by({{1, true}, {0, false}, {2, false}, {3, true}, {4, false}, {5, true}, {6, false}, {7, true}});
    EXPECT(f.decide(&p) == OSORT_DEVICE);
    EXPECT(p.keys.size() == 8 && p.base_word == 1);
    EXPECT(p.keys[0].word == 2 && p.keys[0].type == 0 && p.keys[0].descending == 1 &&
           p.keys[0].count_word == -1 && !p.keys[0].from_ident);
    EXPECT(p.keys[1].from_ident == 1 && p.keys[1].word == 1 && p.keys[1].type == 0 &&
           p.keys[1].descending == 0);
    EXPECT(p.keys[2].word == 3 && p.keys[2].type == 1);
    EXPECT(p.keys[3].word == 4 && p.keys[3].type == 2 && p.keys[3].descending == 1);
    EXPECT(p.keys[4].word == 5 && p.keys[4].type == 1 && p.keys[4].count_word == 6 && !p.keys[4].is_mean);
    EXPECT(p.keys[5].word == 7 && p.keys[5].type == 2 && p.keys[5].count_word == 8 && p.keys[5].is_mean == 1);
    EXPECT(p.keys[6].word == 9 && p.keys[6].type == 0 && p.keys[6].count_word == -1);
    EXPECT(p.keys[7].word == 10 && p.keys[7].type == 2 && p.keys[7].count_word == 11);
    // nine specs
    f.by({{1, true}, {0, false}, {2, false}, {3, true}, {4, false}, {5, true}, {6, false}, {7, true},
          {1, false}});
    EXPECT(f.decide(&p) == OSORT_TOO_MANY_SPECS && p.keys.empty());
    // the thresholds and switches
    f.by({{1, true}, {0, false}});
    f.in.n = kDeviceEmitMinGroups - 1;
    EXPECT(f.decide(&p) == OSORT_FEW_RECORDS);
    f.in.n = kDeviceEmitMinGroups;
    EXPECT(f.decide(&p) == OSORT_DEVICE && p.keys.size() == 2);
    f.in.n = (1ull << 32) - 1;
    EXPECT(f.decide(&p) == OSORT_DEVICE);
    f.in.n = 1ull << 32;
    EXPECT(f.decide(&p) == OSORT_TOO_MANY_RECORDS);
    f.in.n = kDeviceEmitMinGroups;
    f.in.enabled = false;
    EXPECT(f.decide(&p) == OSORT_SWITCHED_OFF);
    f.in.enabled = true;
    f.in.group_mode = EVQL_MODE_PARTIAL;
    EXPECT(f.decide(&p) == OSORT_NO_ORDER);
    f.in.group_mode = EVQL_MODE_FINAL;
    f.by({});
    EXPECT(f.decide(&p) == OSORT_NO_ORDER);
    // what a record does not hold, as the second spec
    f.by({{1, false}, {f.arith, false}});
    EXPECT(f.decide(&p) == OSORT_UNREADABLE);
    f.by({{1, false}, {f.first_row_string, false}});
    EXPECT(f.decide(&p) == OSORT_UNREADABLE);
    // an expression over the output columns
    f.by({{1, false}, {2, false}});
    {
      ExprPtr c = std::make_shared<Expr>();
      c->kind = Expr::CALL;
      c->type = EVQL_T_INT64;
      c->args.push_back(f.order[1].call);
      f.order[1].call = c;
    }
    EXPECT(f.decide(&p) == OSORT_EXPRESSION);
    f.order[1].call = nullptr;
    EXPECT(f.decide(&p) == OSORT_EXPRESSION);
    // an input index beyond the select list (query_set_order refuses it earlier)
    f.by({{1, false}});
    f.order[0].call->input = 100;
    EXPECT(f.decide(&p) == OSORT_UNREADABLE);
  }
  {
    // a signed and a float key; a string key is not a record word
    Fixture fi(EVQL_T_INT64, fns, types);
    fi.by({{0, true}});
    EXPECT(fi.decide(&p) == OSORT_DEVICE && p.keys[0].from_ident == 1 && p.keys[0].type == 1);
    Fixture ff(EVQL_T_FLOAT64, fns, types);
    ff.by({{0, false}});
    EXPECT(ff.decide(&p) == OSORT_DEVICE && p.keys[0].type == 2);
    Fixture fs(EVQL_T_STRING, fns, types);
    fs.by({{1, false}, {0, false}});
    EXPECT(fs.decide(&p) == OSORT_UNREADABLE);
  }
  {
    // with a first row the states move one word up, and the base order is the first row's
    Fixture f(EVQL_T_UINT64, fns, types, true);
    f.by({{1, false}});
    EXPECT(f.decide(&p) == OSORT_DEVICE && p.base_word == 2 && p.keys[0].word == 3);
  }
  {
    // an exact float sum is rounded from 128 bits on the host
    Fixture f(EVQL_T_UINT64, fns, types, false, 2);
    f.by({{1, false}, {3, false}});
    EXPECT(f.decide(&p) == OSORT_UNREADABLE);
    OrderKeyArgs k{};
    EXPECT(classify_order_key(f.kp, f.select, f.agg_index, f.passthrough, f.order[1], false, &k) ==
           OKEY_EXACT_SUM);
    EXPECT(classify_order_key(f.kp, f.select, f.agg_index, f.passthrough, f.order[0], true, &k) ==
           OKEY_RECORD && k.descending == 1);
  }
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
