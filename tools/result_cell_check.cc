// result_cell_check.cc -- where a select cell lives in a group record and how it is read
// (eventql_amd/csrc/result_cell.h, result_cell.cc) exercised on its own, so that it can run
// under AddressSanitizer / UBSan without a device or the HIP runtime:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I eventql_amd/csrc tools/result_cell_check.cc eventql_amd/csrc/result_cell.cc \
//       -o /tmp/result_cell_check
//
// Exit status 0 and "ok" when every expectation holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "codegen.h"
#include "result_cell.h"

using namespace evql;

static int failures = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      ++failures;                                                 \
    }                                                             \
  } while (0)

static LoweredProgram input_prog(uint32_t i, uint32_t type) {
  LoweredProgram p;
  p.call = std::make_shared<Expr>();
  p.call->kind = Expr::INPUT;
  p.call->input = i;
  p.call->type = type;
  p.return_type = type;
  return p;
}

static uint64_t f64_bits(double v) {
  uint64_t b;
  memcpy(&b, &v, 8);
  return b;
}

// ---- the classifier -------------------------------------------------------------------------
// every aggregate function: does a count word follow the state word, is the value a mean
struct FnRow {
  uint32_t fn;
  bool counted, mean;
};
static const FnRow kFns[] = {
    {EVQL_AGG_COUNT, false, false},        {EVQL_AGG_SUM_UINT64, false, false},
    {EVQL_AGG_SUM_INT64, false, false},    {EVQL_AGG_SUM_FLOAT64, false, false},
    {EVQL_AGG_MIN_UINT64, true, false},    {EVQL_AGG_MAX_UINT64, true, false},
    {EVQL_AGG_MIN_INT64, true, false},     {EVQL_AGG_MAX_INT64, true, false},
    {EVQL_AGG_MIN_FLOAT64, true, false},   {EVQL_AGG_MAX_FLOAT64, true, false},
    {EVQL_AGG_MEAN_UINT64, true, true},    {EVQL_AGG_MEAN_INT64, true, true},
    {EVQL_AGG_MEAN_FLOAT64, true, true},   {EVQL_AGG_COUNT_DISTINCT_UINT64, false, false}};

static void check_aggregates() {
  EXPECT(sizeof(kFns) / sizeof(kFns[0]) == EVQL_AGG_COUNT_DISTINCT_UINT64);  // 1 .. 14, all of them
  for (int hashed = 0; hashed < 2; ++hashed) {
    // an exact key: [kind][identity][states]; a hashed key with first rows:
    // [kind][identity][identity 2][first row][states]
    KernelPlan kp;
    kp.key_mode = hashed ? KEY_HASHED : KEY_EXACT;
    kp.need_first_row = hashed != 0;
    const uint32_t base = hashed ? 4 : 2;
    for (const FnRow& r : kFns) {
      AggPlan a;
      a.fn = r.fn;
      a.first_word = int(kp.states.size());
      a.nwords = r.counted ? 2 : 1;
      a.exact_index = r.fn == EVQL_AGG_SUM_FLOAT64 ? 0 : -1;
      for (int w = 0; w < a.nwords; ++w) kp.states.push_back(StateWord{0});
      kp.aggs.push_back(a);
    }
    uint32_t word = base;
    for (size_t i = 0; i < kp.aggs.size(); ++i) {
      const FnRow& r = kFns[i];
      ResultCell c;
      c.count_word = 77;  // (whatever the caller left there)
      c.is_mean = 1;
      const AggPlan* a = nullptr;
      EXPECT(aggregate_cell(kp, int(i), &c, &a));
      EXPECT(a == &kp.aggs[i] && a->fn == r.fn);
      EXPECT((a->exact_index >= 0) == (r.fn == EVQL_AGG_SUM_FLOAT64));
      EXPECT(c.kind == 1 && c.word == word);
      EXPECT(c.count_word == (r.counted ? int32_t(word + 1) : -1));
      EXPECT(c.is_mean == (r.mean ? 1u : 0u));
      word += r.counted ? 2 : 1;
    }
    ResultCell c;
    EXPECT(aggregate_cell(kp, 0, &c));  // (the aggregate is not asked for)
    EXPECT(!aggregate_cell(kp, -1, &c) && !aggregate_cell(kp, int(kp.aggs.size()), &c));
  }
}

static void check_first_rows() {
  // scan columns 0 u (UINT64), 1 s (STRING), 2 b (BOOL), 3 f (FLOAT64 over a uint column),
  // 4 g (a real FLOAT64); the scan select list reads them one to one, entry 5 is computed
  KernelPlan kp;
  std::vector<LoweredProgram> scan_select;
  const uint32_t types[5] = {EVQL_T_UINT64, EVQL_T_STRING, EVQL_T_BOOL, EVQL_T_FLOAT64, EVQL_T_FLOAT64};
  for (uint32_t i = 0; i < 5; ++i) {
    ColAccess c;
    c.stype = types[i];
    c.string_hash = types[i] == EVQL_T_STRING;
    c.from_uint_to_float = i == 3;
    kp.cols.push_back(c);
    scan_select.push_back(input_prog(i, types[i]));
  }
  LoweredProgram computed = input_prog(0, EVQL_T_UINT64);
  computed.call->kind = Expr::CALL;
  scan_select.push_back(computed);

  uint32_t col = 99;
  EXPECT(bare_column(kp, scan_select, input_prog(3, EVQL_T_FLOAT64), &col) && col == 3);
  EXPECT(!bare_column(kp, scan_select, input_prog(5, EVQL_T_UINT64), &col));  // computed below
  EXPECT(!bare_column(kp, scan_select, input_prog(6, EVQL_T_UINT64), &col));  // no such entry
  EXPECT(!bare_column(kp, scan_select, computed, &col));                      // computed above
  LoweredProgram none;
  EXPECT(!bare_column(kp, scan_select, none, &col));
  {
    std::vector<LoweredProgram> far{input_prog(5, EVQL_T_UINT64)};  // a column the plan has not
    EXPECT(!bare_column(kp, far, input_prog(0, EVQL_T_UINT64), &col));
  }

  ResultCell c;
  EXPECT(first_row_cell(kp, scan_select, input_prog(3, EVQL_T_FLOAT64), &c));  // uint read as FLOAT64
  EXPECT(c.kind == 2 && c.src == 3 && c.stype == EVQL_T_FLOAT64 && c.to_float == 1 && !c.is_string &&
         !c.is_bool && c.count_word == -1);
  c = ResultCell();
  EXPECT(first_row_cell(kp, scan_select, input_prog(4, EVQL_T_FLOAT64), &c) && c.src == 4 && !c.to_float);
  c = ResultCell();
  EXPECT(first_row_cell(kp, scan_select, input_prog(1, EVQL_T_STRING), &c));
  EXPECT(c.kind == 2 && c.src == 1 && c.stype == EVQL_T_STRING && c.is_string == 1 && !c.is_bool && !c.to_float);
  c = ResultCell();
  EXPECT(first_row_cell(kp, scan_select, input_prog(2, EVQL_T_BOOL), &c));
  EXPECT(c.kind == 2 && c.src == 2 && c.is_bool == 1 && !c.is_string);
  c = ResultCell();
  EXPECT(first_row_cell(kp, scan_select, input_prog(0, EVQL_T_UINT64), &c) && c.src == 0 && !c.to_float);
  // the column's type is not the expression's: nothing is filled in
  c = ResultCell();
  EXPECT(!first_row_cell(kp, scan_select, input_prog(0, EVQL_T_FLOAT64), &c) && c.kind == 0 && c.src == 0);
  EXPECT(!first_row_cell(kp, scan_select, input_prog(1, EVQL_T_UINT64), &c) && !c.is_string);
  EXPECT(!first_row_cell(kp, scan_select, input_prog(5, EVQL_T_UINT64), &c));
}

// ---- the read -------------------------------------------------------------------------------
static void check_cell_bits() {
  bool null = false;
  // the key
  ResultCell key;
  const uint64_t rec_key[2] = {1, 0xdeadbeefcafef00dull};
  EXPECT(cell_bits(key, rec_key, nullptr, nullptr, 0, 0, &null) == 0xdeadbeefcafef00dull && !null);
  const uint64_t rec_null[2] = {2, 0xdeadbeefcafef00dull};  // kind word 2: the NULL key
  null = false;
  EXPECT(cell_bits(key, rec_null, nullptr, nullptr, 0, 0, &null) == 0 && null);

  // states: [kind][identity][state][count]
  ResultCell plain;
  plain.kind = 1;
  plain.word = 2;
  const uint64_t rec_plain[4] = {1, 5, 1234567, 0};  // (a count or sum: no count word is read)
  null = true;
  EXPECT(cell_bits(plain, rec_plain, nullptr, nullptr, 0, 0, &null) == 1234567 && !null);

  ResultCell minmax = plain;
  minmax.count_word = 3;
  const uint64_t rec_min0[4] = {1, 5, ~0ull, 0};  // min's identity, no non-NULL input
  null = false;
  EXPECT(cell_bits(minmax, rec_min0, nullptr, nullptr, 0, 0, &null) == 0 && null);
  const uint64_t rec_max0[4] = {1, 5, 0x8000000000000000ull, 0};  // max#int64's identity
  null = false;
  EXPECT(cell_bits(minmax, rec_max0, nullptr, nullptr, 0, 0, &null) == 0 && null);
  const uint64_t rec_min[4] = {1, 5, 42, 7};
  EXPECT(cell_bits(minmax, rec_min, nullptr, nullptr, 0, 0, &null) == 42 && !null);

  ResultCell mean = minmax;
  mean.is_mean = 1;
  const uint64_t rec_mean0[4] = {1, 5, f64_bits(3.5), 0};
  null = false;
  EXPECT(cell_bits(mean, rec_mean0, nullptr, nullptr, 0, 0, &null) == 0 && null);
  const uint64_t rec_mean[4] = {1, 5, f64_bits(7.0), 2};
  EXPECT(cell_bits(mean, rec_mean, nullptr, nullptr, 0, 0, &null) == f64_bits(3.5) && !null);
  // the smallest subnormal over 3: rounds to +0.0, and is no NULL
  const uint64_t rec_tiny[4] = {1, 5, f64_bits(0x1p-1074), 3};
  null = true;
  EXPECT(cell_bits(mean, rec_tiny, nullptr, nullptr, 0, 0, &null) == 0 && !null);
  // a count of 2^53 + 1 is 2^53 as a double (ties to even): 2^53 / that = 1.0 exactly
  const uint64_t rec_big[4] = {1, 5, f64_bits(0x1p53), (1ull << 53) + 1};
  EXPECT(cell_bits(mean, rec_big, nullptr, nullptr, 0, 0, &null) == 0x3ff0000000000000ull && !null);
  const uint64_t rec_neg[4] = {1, 5, f64_bits(-1.0), 3};  // one division, rounded once
  EXPECT(cell_bits(mean, rec_neg, nullptr, nullptr, 0, 0, &null) == 0xbfd5555555555555ull && !null);

  // first rows: [src][n] arrays, n = 3
  const uint64_t n = 3;
  const uint64_t vals[2 * 3] = {10, 11, 12, (1ull << 63) + 1, ~0ull, 77};
  const uint8_t tags[2 * 3] = {0, 1, 0, 0, 0, 3};
  ResultCell first;
  first.kind = 2;
  first.src = 0;
  EXPECT(cell_bits(first, nullptr, vals, tags, n, 0, &null) == 10 && !null);
  EXPECT(cell_bits(first, nullptr, vals, tags, n, 1, &null) == 11 && null);  // the tag is set
  EXPECT(cell_bits(first, nullptr, vals, tags, n, 2, &null) == 12 && !null);
  first.src = 1;
  first.to_float = 1;
  EXPECT(cell_bits(first, nullptr, vals, tags, n, 0, &null) == 0x43e0000000000000ull && !null);  // 2^63
  EXPECT(cell_bits(first, nullptr, vals, tags, n, 1, &null) == 0x43f0000000000000ull && !null);  // 2^64
  EXPECT(cell_bits(first, nullptr, vals, tags, n, 2, &null) == f64_bits(77.0) && null);  // (bit 0 alone)

  // a BOOL is 0 | 1 whatever the word holds
  ResultCell b = first;
  b.to_float = 0;
  b.is_bool = 1;
  EXPECT(cell_bits(b, nullptr, vals, tags, n, 1, &null) == 1 && !null);
  ResultCell bkey;
  bkey.is_bool = 1;
  EXPECT(cell_bits(bkey, rec_key, nullptr, nullptr, 0, 0, &null) == 1);
  const uint64_t rec_false[2] = {1, 0};
  EXPECT(cell_bits(bkey, rec_false, nullptr, nullptr, 0, 0, &null) == 0 && !null);
}

static void check_string_elem() {
  const char* src = "0123456789abcdef";
  auto from = [&](uint32_t at) { return [=](uint32_t k) { return uint8_t(src[at + k]); }; };
  uint8_t buf[32];
  memset(buf, 0xee, sizeof(buf));
  EXPECT(put_string_elem(buf, 11, 0x80, from(2)) == 16);
  const uint8_t want[16] = {11, 0, 0, 0, '2', '3', '4', '5', '6', '7', '8', '9', 'a', 'b', 'c', 0x80};
  EXPECT(memcmp(buf, want, 16) == 0 && buf[16] == 0xee);
  memset(buf, 0xee, sizeof(buf));
  EXPECT(put_string_elem(buf, 0, 1, from(0)) == 5);  // a NULL / an empty string: no byte is read
  const uint8_t empty[5] = {0, 0, 0, 0, 1};
  EXPECT(memcmp(buf, empty, 5) == 0 && buf[5] == 0xee);
}

int main() {
  check_aggregates();
  check_first_rows();
  check_cell_bits();
  check_string_elem();
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
