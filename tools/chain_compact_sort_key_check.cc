// chain_compact_sort_key_check.cc -- the key rule of evql_lsm_chain_compact_sorted
// (plan_compact_sort_key / plan_compact_sort_rows, eventql_amd/csrc/chain_compact_plan.cc)
// exercised on its own, so that it can run under AddressSanitizer / UBSan without a device or
// the HIP runtime:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I eventql_amd/csrc tools/chain_compact_sort_key_check.cc \
//       eventql_amd/csrc/chain_compact_plan.cc -o /tmp/chain_compact_sort_key_check
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

enum Answer { ACCEPTED, BAD_ARGUMENT, NOT_SUPPORTED };

static Answer ask(const std::vector<ColumnSpec>& specs, const char* key, size_t* index = nullptr,
                  std::string* msg = nullptr) {
  size_t k = 99;
  bool notsup = false;
  const std::string err = plan_compact_sort_key(specs, key, &k, &notsup);
  if (index) *index = k;
  if (msg) *msg = err;
  if (err.empty()) {
    EXPECT(!notsup);
    return ACCEPTED;
  }
  return notsup ? NOT_SUPPORTED : BAD_ARGUMENT;
}

int main() {
  const ColumnType U = ColumnType::UNSIGNED_INT, S = ColumnType::STRING, B = ColumnType::BOOLEAN,
                   F = ColumnType::FLOAT, I = ColumnType::SIGNED_INT, D = ColumnType::DATETIME;
  const std::vector<ColumnSpec> flat = {spec("x", U), spec("opt", U, 0, 1), spec("f", F), spec("s", S),
                                        spec("i", I), spec("t", D), spec("__lsm_is_update", B)};
  size_t k = 0;
  std::string msg;
  EXPECT(ask(flat, "x", &k) == ACCEPTED && k == 0);
  EXPECT(ask(flat, "t", &k) == ACCEPTED && k == 5);
  EXPECT(ask(flat, nullptr) == BAD_ARGUMENT);
  EXPECT(ask(flat, "nowhere") == BAD_ARGUMENT);
  EXPECT(ask(flat, "") == BAD_ARGUMENT);
  EXPECT(ask(flat, "opt", nullptr, &msg) == NOT_SUPPORTED && msg.find("optional") != std::string::npos);
  EXPECT(ask(flat, "f", nullptr, &msg) == NOT_SUPPORTED && msg.find("float") != std::string::npos);
  EXPECT(ask(flat, "s", nullptr, &msg) == NOT_SUPPORTED && msg.find("string") != std::string::npos);
  EXPECT(ask(flat, "i", nullptr, &msg) == NOT_SUPPORTED && msg.find("signed") != std::string::npos);
  EXPECT(ask(flat, "__lsm_is_update", nullptr, &msg) == NOT_SUPPORTED && msg.find("boolean") != std::string::npos);

  // a repeated / nested key is a bad argument; a repeated / nested OTHER column is not supported
  const std::vector<ColumnSpec> nested = {spec("x", U), spec("items.v", U, 1, 2), spec("deep", U, 0, 2)};
  EXPECT(ask(nested, "items.v") == BAD_ARGUMENT);
  EXPECT(ask(nested, "deep") == BAD_ARGUMENT);
  EXPECT(ask(nested, "x", nullptr, &msg) == NOT_SUPPORTED && msg.find("items.v") != std::string::npos);
  EXPECT(ask({spec("x", U), spec("deep", U, 0, 2)}, "x") == NOT_SUPPORTED);
  EXPECT(ask({spec("x", U), spec("opt", U, 0, 1)}, "x") == ACCEPTED);
  EXPECT(ask({}, "x") == BAD_ARGUMENT);

  bool notsup = true;
  EXPECT(plan_compact_sort_rows(0, &notsup).empty() && !notsup);
  EXPECT(plan_compact_sort_rows(0xffffffffull, &notsup).empty() && !notsup);
  EXPECT(!plan_compact_sort_rows(0x100000000ull, &notsup).empty() && notsup);

  if (failures) return 1;
  puts("ok");
  return 0;
}
