// merge_frame_index.h -- the host-only part of the device merge of PARTIAL aggregate rows
// (merge_device.cc): every byte of a frame is validated here, once, and the
// kernels get the offset of every row.  No HIP call and no device state: it builds and runs on
// its own (tools/merge_frame_index_check.cc).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace evql {

struct LoweredProgram;

// how one select expression travels in a row (results.cc save_state / SValue::encode)
enum MergeCellClass : uint8_t {
  MCELL_VARUINT = 0,     // count / integer sum: LEB128 of the state word
  MCELL_RAW8 = 1,        // sum(float64): the 8 bytes of the state word
  MCELL_COUNT_RAW8 = 2,  // min / max / mean: LEB128 of the non-NULL count, then the 8 bytes
  // non-aggregates: u8 wire type, lenenc(value bytes || tag); the class is the return type's
  MCELL_STRING = 3,
  MCELL_BOOL = 4,
  MCELL_NUM8 = 5,        // UINT64, INT64, FLOAT64, TIMESTAMP64
  MCELL_NIL = 6          // a NIL-typed expression: only NIL arrives
};

// the fold of one aggregate's state words (k_mrg_fold)
enum MergeFoldOp : uint8_t {
  MFOLD_ADD_U64 = 0,  // count, sum(uint64 / int64): one word
  MFOLD_ADD_F64 = 1,  // sum(float64): one word
  MFOLD_MEAN = 2,     // float sum + count
  MFOLD_MIN_U64 = 3, MFOLD_MAX_U64 = 4, MFOLD_MIN_I64 = 5, MFOLD_MAX_I64 = 6,
  MFOLD_MIN_F64 = 7, MFOLD_MAX_F64 = 8,  // value + count
  MFOLD_LAST = 9      // non-aggregate: value word + (wire type | tag << 8) of the last row
};

// evql_stype values the decode kernel tells apart (it is built without evql_gpu.h)
static const uint32_t kMergeWireNil = 0, kMergeWireBool = 4, kMergeWireString = 5;

static const uint32_t kMaxMergeCols = 64;
static const uint32_t kMergeKeyBytes = 20;
static const uint32_t kMergeKeyWords = 3;
// a string word is (len << 40 | arena position)
static const uint64_t kMergeMaxStringLen = (1ull << 24) - 1;

// the fixed-width record of a select list: [3 key words][cell words...]
struct MergeRecordLayout {
  uint32_t ncols = 0;
  uint32_t rw = 0;  // words per record
  uint8_t cls[kMaxMergeCols];
  uint8_t op[kMaxMergeCols];
  uint16_t word[kMaxMergeCols];  // first record word of the cell
};

enum MergeLayoutResult {
  MLAYOUT_OK = 0,
  MLAYOUT_AGGREGATE = 1,  // count_distinct: the saved state is a set
  MLAYOUT_TOO_WIDE = 2    // more than kMaxMergeCols select expressions
};
MergeLayoutResult merge_record_layout(const std::vector<LoweredProgram>& select, MergeRecordLayout* out);

enum MergeIndexResult {
  MINDEX_OK = 0,
  MINDEX_MALFORMED = 1,   // EVQL_EIO
  MINDEX_CELL_CLASS = 2,  // EVQL_ENOTSUP: a cell of another size class than the program's return type
  MINDEX_TOO_LARGE = 3    // EVQL_ENOTSUP: offsets are u32, string lengths 24 bits
};

// Payload of one QUERY_PARTIALAGGR_RESULT frame: varuint flags, varuint count, count rows of
// (20-byte key, cells).  On MINDEX_OK row_off holds count + 1 offsets into the payload: row i is
// [row_off[i], row_off[i + 1]), its key the first 20 bytes.  Anything else leaves row_off empty.
// Stricter than the host merge's reader in one point: a varuint of more than ten bytes is
// malformed (the host stops reading after ten and goes on).
MergeIndexResult index_merge_frame(const MergeRecordLayout& L, const uint8_t* p, size_t len,
                                   std::vector<uint32_t>* row_off);

// The two STRING SVectors of a PartialGroupBy nextBatch (u32 length, bytes, tag per element).
// nrows entries each: the 20 key bytes of row i start at keys[key_off[i]], its cells are
// data[data_off[i], data_end[i]) and fill that range exactly.
MergeIndexResult index_merge_rows(const MergeRecordLayout& L, const uint8_t* keys, size_t keys_len,
                                  const uint8_t* data, size_t data_len, size_t nrows,
                                  std::vector<uint32_t>* key_off, std::vector<uint32_t>* data_off,
                                  std::vector<uint32_t>* data_end);

}  // namespace evql
