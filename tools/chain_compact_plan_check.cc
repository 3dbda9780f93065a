// chain_compact_plan_check.cc -- the host-only part of evql_lsm_chain_compact (column rules,
// output sizes: eventql_amd/csrc/chain_compact_plan.cc) exercised on its own, so that it can
// run under AddressSanitizer / UBSan without a device or the HIP runtime:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I eventql_amd/csrc tools/chain_compact_plan_check.cc \
//       eventql_amd/csrc/chain_compact_plan.cc -o /tmp/chain_compact_plan_check
//
// Exit status 0 and "ok" when every expectation holds.
#include <cstdio>
#include <cstdlib>
#include "chain_compact_plan.h"

using namespace evql;

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      ++failures;                                                 \
    }                                                             \
  } while (0)

static ColumnLayout col(const char* name, ColumnType t, uint32_t r = 0, uint32_t d = 0) {
  ColumnLayout c;
  c.name = name;
  c.logical_type = t;
  c.storage_type = t == ColumnType::STRING ? ColumnEncoding::STRING_PLAIN : ColumnEncoding::UINT64_PLAIN;
  c.column_id = 1;
  c.rlevel_max = r;
  c.dlevel_max = d;
  return c;
}

static ColumnSpec spec(const char* name, ColumnType t, uint32_t r = 0, uint32_t d = 0) {
  ColumnSpec s;
  s.name = name;
  s.logical_type = t;
  s.storage_type = t == ColumnType::STRING ? ColumnEncoding::STRING_PLAIN : ColumnEncoding::UINT64_LEB128;
  s.column_id = 1;
  s.rlevel_max = r;
  s.dlevel_max = d;
  s.bitpack_max_value = 0;
  return s;
}

int main() {
  const ColumnType U = ColumnType::UNSIGNED_INT, S = ColumnType::STRING, B = ColumnType::BOOLEAN;
  TableLayout newest{}, middle{}, oldest{};
  newest.num_rows = 4097;
  newest.columns = {col("x", U), col("late", U, 0, 1), col("items.v", U, 1, 2), col("s", S),
                    col("__lsm_is_update", B)};
  middle.num_rows = 0;
  middle.columns = {col("x", U), col("items.v", U, 1, 2), col("s", S), col("__lsm_is_update", B)};
  oldest.num_rows = 2048;
  oldest.columns = {col("s", S), col("x", U), col("__lsm_skip", B), col("__lsm_is_update", B)};
  const std::vector<const TableLayout*> tabs = {&newest, &middle, &oldest};
  const std::vector<uint64_t> kept = {4000, 0, 1};
  CompactPlan p;

  std::vector<ColumnSpec> specs = {spec("x", U), spec("late", U, 0, 1), spec("items.v", U, 1, 2),
                                   spec("s", S), spec("__lsm_is_update", B)};
  std::string err = plan_chain_compact(tabs, kept, specs, false, &p);
  EXPECT(err.empty());
  EXPECT(p.columns.size() == 5);
  EXPECT(p.columns[0].source == (std::vector<int>{0, 0, 1}));
  EXPECT(p.columns[1].source == (std::vector<int>{1, -1, -1}) && !p.columns[1].nested);
  EXPECT(p.columns[2].source == (std::vector<int>{2, 1, -1}) && p.columns[2].nested);
  EXPECT(p.columns[3].is_string && p.columns[3].source == (std::vector<int>{3, 2, 0}));
  EXPECT(p.columns[4].constant_false && p.columns[4].source == (std::vector<int>{-1, -1, -1}));
  EXPECT(p.rows_in == 6145 && p.rows_out == 4001 && p.tiles == 3 + 0 + 1);
  EXPECT(p.row_base == (std::vector<uint64_t>{0, 4000, 4000}));
  EXPECT(p.tile_base == (std::vector<uint64_t>{0, 3, 3}));
  EXPECT(p.position == (std::vector<uint32_t>{0, 1, 2}));

  // oldest first
  err = plan_chain_compact(tabs, kept, specs, true, &p);
  EXPECT(err.empty());
  EXPECT(p.row_base == (std::vector<uint64_t>{1, 1, 0}));
  EXPECT(p.tile_base == (std::vector<uint64_t>{1, 1, 0}));
  EXPECT(p.position == (std::vector<uint32_t>{2, 1, 0}));
  EXPECT(p.rows_out == 4001 && p.tiles == 4);

  // the refusals
  auto refused = [&](std::vector<ColumnSpec> sp, const std::vector<uint64_t>& k) {
    return !plan_chain_compact(tabs, k, sp, false, &p).empty();
  };
  EXPECT(refused({spec("late", U, 0, 0)}, kept));          // levels differ / required and absent
  EXPECT(refused({spec("nowhere", U)}, kept));             // required, absent everywhere
  EXPECT(!refused({spec("nowhere", U, 0, 1)}, kept));      // optional, absent everywhere: NULLs
  EXPECT(refused({spec("x", S)}, kept));                   // type
  EXPECT(refused({spec("x", U, 1, 1)}, kept));             // levels
  EXPECT(refused({spec("__lsm_skip", B)}, kept));
  EXPECT(refused({spec("__lsm_is_update", B, 1, 1)}, kept));
  EXPECT(refused({spec("x", U), spec("x", U)}, kept));     // named twice
  EXPECT(refused({}, kept));
  EXPECT(refused({spec("x", U)}, {4098, 0, 0}));           // more kept than rows
  EXPECT(refused({spec("x", U)}, {1, 2}));                 // counts of another chain
  EXPECT(!plan_chain_compact({}, {}, specs, false, &p).empty());

  if (failures) return 1;
  puts("ok");
  return 0;
}
