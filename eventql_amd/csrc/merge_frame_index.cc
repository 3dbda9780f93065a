// merge_frame_index.cc -- see merge_frame_index.h
#include "merge_frame_index.h"
#include <cstring>
#include "plan_ir.h"

namespace evql {

static_assert(kMergeWireNil == EVQL_T_NIL && kMergeWireBool == EVQL_T_BOOL &&
                  kMergeWireString == EVQL_T_STRING, "evql_stype (evql_gpu.h)");

MergeLayoutResult merge_record_layout(const std::vector<LoweredProgram>& select, MergeRecordLayout* out) {
  *out = MergeRecordLayout();
  if (select.size() > kMaxMergeCols) return MLAYOUT_TOO_WIDE;
  uint32_t w = kMergeKeyWords;
  for (size_t i = 0; i < select.size(); ++i) {
    const LoweredProgram& lp = select[i];
    uint8_t cls, op;
    uint32_t words = 2;
    if (lp.is_aggregate) {
      switch (lp.aggregate_fn) {
        case EVQL_AGG_COUNT: case EVQL_AGG_SUM_UINT64: case EVQL_AGG_SUM_INT64:
          cls = MCELL_VARUINT; op = MFOLD_ADD_U64; words = 1; break;
        case EVQL_AGG_SUM_FLOAT64: cls = MCELL_RAW8; op = MFOLD_ADD_F64; words = 1; break;
        case EVQL_AGG_MEAN_UINT64: case EVQL_AGG_MEAN_INT64: case EVQL_AGG_MEAN_FLOAT64:
          cls = MCELL_COUNT_RAW8; op = MFOLD_MEAN; break;
        case EVQL_AGG_MIN_UINT64: cls = MCELL_COUNT_RAW8; op = MFOLD_MIN_U64; break;
        case EVQL_AGG_MAX_UINT64: cls = MCELL_COUNT_RAW8; op = MFOLD_MAX_U64; break;
        case EVQL_AGG_MIN_INT64: cls = MCELL_COUNT_RAW8; op = MFOLD_MIN_I64; break;
        case EVQL_AGG_MAX_INT64: cls = MCELL_COUNT_RAW8; op = MFOLD_MAX_I64; break;
        case EVQL_AGG_MIN_FLOAT64: cls = MCELL_COUNT_RAW8; op = MFOLD_MIN_F64; break;
        case EVQL_AGG_MAX_FLOAT64: cls = MCELL_COUNT_RAW8; op = MFOLD_MAX_F64; break;
        default: return MLAYOUT_AGGREGATE;
      }
    } else {
      op = MFOLD_LAST;
      switch (lp.return_type) {
        case EVQL_T_STRING: cls = MCELL_STRING; break;
        case EVQL_T_BOOL: cls = MCELL_BOOL; break;
        case EVQL_T_NIL: cls = MCELL_NIL; break;
        default: cls = MCELL_NUM8;
      }
    }
    out->cls[i] = cls;
    out->op[i] = op;
    out->word[i] = uint16_t(w);
    w += words;
  }
  out->ncols = uint32_t(select.size());
  out->rw = w;
  return MLAYOUT_OK;
}

namespace {

struct Cursor {
  const uint8_t* p;
  size_t len, pos;
  // util/io/inputstream.cc readVarUInt: 7 bits per byte, LSB group first; at most ten bytes
  bool varuint(uint64_t* v) {
    *v = 0;
    for (int i = 0; i < 10; ++i) {
      if (pos >= len) return false;
      const uint8_t b = p[pos++];
      *v |= uint64_t(b & 0x7f) << (7 * i);
      if (!(b & 0x80)) return true;
    }
    return false;
  }
  bool skip(size_t n) {
    if (n > len - pos) return false;
    pos += n;
    return true;
  }
};

// the cells of one row from c->pos on; the same rules as merge.cc load_state / decode_svalue
MergeIndexResult walk_cells(const MergeRecordLayout& L, Cursor* c) {
  uint64_t v;
  for (uint32_t i = 0; i < L.ncols; ++i) {
    switch (L.cls[i]) {
      case MCELL_VARUINT:
        if (!c->varuint(&v)) return MINDEX_MALFORMED;
        break;
      case MCELL_RAW8:
        if (!c->skip(8)) return MINDEX_MALFORMED;
        break;
      case MCELL_COUNT_RAW8:
        if (!c->varuint(&v) || !c->skip(8)) return MINDEX_MALFORMED;
        break;
      default: {
        if (c->pos >= c->len) return MINDEX_MALFORMED;
        const uint8_t type = c->p[c->pos++];
        uint64_t n;
        if (!c->varuint(&n) || n > c->len - c->pos) return MINDEX_MALFORMED;
        const uint8_t* d = c->p + c->pos;
        uint8_t cls;
        switch (type) {
          case EVQL_T_NIL: cls = MCELL_NIL; break;
          case EVQL_T_BOOL:
            if (n != 2) return MINDEX_MALFORMED;
            cls = MCELL_BOOL;
            break;
          case EVQL_T_STRING: {
            if (n < 5) return MINDEX_MALFORMED;
            uint32_t sl;
            memcpy(&sl, d, 4);
            if (uint64_t(sl) + 5 != n) return MINDEX_MALFORMED;
            if (sl > kMergeMaxStringLen) return MINDEX_TOO_LARGE;
            cls = MCELL_STRING;
            break;
          }
          case EVQL_T_UINT64: case EVQL_T_INT64: case EVQL_T_FLOAT64: case EVQL_T_TIMESTAMP64:
            if (n != 9) return MINDEX_MALFORMED;
            cls = MCELL_NUM8;
            break;
          default: return MINDEX_MALFORMED;
        }
        if (cls != MCELL_NIL && cls != L.cls[i]) return MINDEX_CELL_CLASS;
        c->pos += size_t(n);
      }
    }
  }
  return MINDEX_OK;
}

}  // namespace

MergeIndexResult index_merge_frame(const MergeRecordLayout& L, const uint8_t* p, size_t len,
                                   std::vector<uint32_t>* row_off) {
  row_off->clear();
  Cursor c{p, len, 0};
  uint64_t flags, count;
  if (!c.varuint(&flags) || !c.varuint(&count)) return MINDEX_MALFORMED;
  // (a row is at least its key: a count the payload cannot hold is refused before any reserve)
  if (count > (len - c.pos) / kMergeKeyBytes) return MINDEX_MALFORMED;
  if (len > 0xffffffffull) return MINDEX_TOO_LARGE;
  row_off->reserve(size_t(count) + 1);
  for (uint64_t j = 0; j < count; ++j) {
    row_off->push_back(uint32_t(c.pos));
    MergeIndexResult r = c.skip(kMergeKeyBytes) ? walk_cells(L, &c) : MINDEX_MALFORMED;
    if (r != MINDEX_OK) {
      row_off->clear();
      return r;
    }
  }
  row_off->push_back(uint32_t(c.pos));
  return MINDEX_OK;
}

MergeIndexResult index_merge_rows(const MergeRecordLayout& L, const uint8_t* keys, size_t keys_len,
                                  const uint8_t* data, size_t data_len, size_t nrows,
                                  std::vector<uint32_t>* key_off, std::vector<uint32_t>* data_off,
                                  std::vector<uint32_t>* data_end) {
  key_off->clear();
  data_off->clear();
  data_end->clear();
  auto bad = [&](MergeIndexResult r) {
    key_off->clear();
    data_off->clear();
    data_end->clear();
    return r;
  };
  // (an element is at least its length and its tag)
  if (nrows > keys_len / 5 || nrows > data_len / 5) return MINDEX_MALFORMED;
  if (keys_len > 0xffffffffull || data_len > 0xffffffffull) return MINDEX_TOO_LARGE;
  Cursor kc{keys, keys_len, 0}, dc{data, data_len, 0};
  key_off->reserve(nrows);
  data_off->reserve(nrows);
  data_end->reserve(nrows);
  for (size_t i = 0; i < nrows; ++i) {
    uint32_t kn, dn;
    if (kc.len - kc.pos < 4 || dc.len - dc.pos < 4) return bad(MINDEX_MALFORMED);
    memcpy(&kn, keys + kc.pos, 4);
    memcpy(&dn, data + dc.pos, 4);
    kc.pos += 4;
    dc.pos += 4;
    key_off->push_back(uint32_t(kc.pos));
    data_off->push_back(uint32_t(dc.pos));
    if (!kc.skip(size_t(kn) + 1) || size_t(dn) + 1 > dc.len - dc.pos || kn != kMergeKeyBytes) {
      return bad(MINDEX_MALFORMED);
    }
    // the cells fill the element exactly
    Cursor row{data, dc.pos + dn, dc.pos};
    MergeIndexResult r = walk_cells(L, &row);
    if (r == MINDEX_OK && row.pos != row.len) r = MINDEX_MALFORMED;
    if (r != MINDEX_OK) return bad(r);
    data_end->push_back(uint32_t(row.len));
    dc.pos += size_t(dn) + 1;
  }
  return MINDEX_OK;
}

}  // namespace evql
