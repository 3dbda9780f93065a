// result_cell.h -- where a select cell lives in a group record, and how its value is read
// there.  Every route a GROUP BY result leaves the device by -- FINAL rows,
// PARTIAL rows, a resident cstable, the ORDER BY sort, the host's direct pack -- describes a
// cell with the one ResultCell and reads it with the one cell_bits.  The classifier half
// (result_cell.cc) is host-only; the read compiles for the host and for the device.
#pragma once
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define EVQL_CELL_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define EVQL_CELL_FN inline __attribute__((always_inline))
#endif

namespace evql {

struct KernelPlan;
struct LoweredProgram;
struct AggPlan;

// A group record is [kind word][identity][second identity][first row][state words ..]
// (KernelPlan: the bracketed words where the plan has them).  Plain data: it travels in kernel
// arguments, and the route structs (EmitCol, MatCol, PartialCell, OrderKeyArgs) derive from it.
struct ResultCell {
  uint32_t kind = 0;        // 0 the exact key (record word 1; NULL when the kind word is 2),
                            // 1 an aggregate's state, 2 scan column `src` at the group's first row
  uint32_t stype = 0;       // evql_stype of the value
  uint32_t word = 0;        // kind 1: record word of the state
  int32_t count_word = -1;  // kind 1, min / max / mean: record word of the non-NULL count
  uint32_t is_mean = 0;     // kind 1: state word = float sum, value = sum / double(count)
  uint32_t src = 0;         // kind 2: scan column index
  uint32_t to_float = 0;    // kind 2: (double) of the unsigned raw value (readFloat on a uint column)
  uint32_t is_string = 0;   // kind 2: the value word is (len << 40 | position) in the column's pages
  uint32_t is_bool = 0;     // the value is 0 | 1
};

// The one `fn` switch: kind 1, the state's word, the count's word for min / max / mean, the
// mean flag.  false: `agg_index` names no aggregate of the plan.  *agg (where asked for) is the
// aggregate, so that a route can refuse its function or an exact sum by its own rule.
bool aggregate_cell(const KernelPlan& kp, int agg_index, ResultCell* cell, const AggPlan** agg = nullptr);

// a bare column: `lp` = X_INPUT(j) of the scan select list, whose expression j = X_INPUT(c) of
// the scan columns
bool bare_column(const KernelPlan& kp, const std::vector<LoweredProgram>& scan_select,
                 const LoweredProgram& lp, uint32_t* col);

// ... read from the group's first row: kind 2.  false: no bare column, or the column's type is
// not the expression's.  Whether first rows exist at all (need_first_row, a merged result, a
// nested scan) and whether a STRING must be a hashed string column is the route's to ask.
bool first_row_cell(const KernelPlan& kp, const std::vector<LoweredProgram>& scan_select,
                    const LoweredProgram& lp, ResultCell* cell);

// The one read: the value bits of cell `c` of group i, whose record is `rec`; first_vals /
// first_tags are the [src][n] arrays of the first-row gather (kind 2 only).  A NULL key and a
// min / max / mean without a non-NULL input read 0; a NULL first-row value keeps the gathered
// word.  The mean is one double division.
EVQL_CELL_FN uint64_t cell_bits(const ResultCell& c, const uint64_t* rec, const uint64_t* first_vals,
                                const uint8_t* first_tags, uint64_t n, uint64_t i, bool* null) {
  uint64_t bits = 0;
  *null = false;
  if (c.kind == 0) {
    if (rec[0] == 2) *null = true; else bits = rec[1];
  } else if (c.kind == 1) {
    bits = rec[c.word];
    if (c.count_word >= 0) {
      const uint64_t cnt = rec[c.count_word];
      if (cnt == 0) {
        bits = 0;
        *null = true;
      } else if (c.is_mean) {
        double sum;
        __builtin_memcpy(&sum, &bits, 8);
        const double mean = sum / (double) cnt;
        __builtin_memcpy(&bits, &mean, 8);
      }
    }
  } else {
    const uint64_t raw = first_vals[(uint64_t) c.src * n + i];
    *null = first_tags[(uint64_t) c.src * n + i] & 1;
    bits = raw;
    if (c.to_float) {
      const double f = (double) raw;
      __builtin_memcpy(&bits, &f, 8);
    }
  }
  return c.is_bool ? (uint64_t) (bits != 0) : bits;
}

// The SVector element of a STRING at p: u32 length, the bytes, the tag.  byte_at(k) is byte k of
// the string: out of a column's paged image, or out of an arena.  Returns the element's size.
template <class ByteAt>
EVQL_CELL_FN uint32_t put_string_elem(uint8_t* p, uint32_t len, uint8_t tag, ByteAt byte_at) {
  p[0] = (uint8_t) len; p[1] = (uint8_t) (len >> 8); p[2] = (uint8_t) (len >> 16); p[3] = (uint8_t) (len >> 24);
  for (uint32_t k = 0; k < len; ++k) p[4 + k] = byte_at(k);
  p[4 + len] = tag;
  return 5 + len;
}

}  // namespace evql
