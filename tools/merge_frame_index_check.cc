// merge_frame_index_check.cc -- csrc/merge_frame_index.cc on its own, for a sanitizer build:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I eventql_amd/csrc tools/merge_frame_index_check.cc eventql_amd/csrc/merge_frame_index.cc
// Every input is copied into a heap block of exactly its size, so that a read behind the end
// of a payload is a report and not a lucky zero.  Prints "ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "merge_frame_index.h"
#include "plan_ir.h"

using namespace evql;

namespace {

typedef std::vector<uint8_t> Bytes;

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                           \
    }                                                                    \
  } while (0)

void put_varuint(Bytes* b, uint64_t v) {
  do {
    uint8_t x = v & 0x7f;
    v >>= 7;
    b->push_back(x | (v ? 0x80 : 0));
  } while (v);
}
void put_raw(Bytes* b, const void* p, size_t n) {
  const uint8_t* c = static_cast<const uint8_t*>(p);
  b->insert(b->end(), c, c + n);
}
void put_u64(Bytes* b, uint64_t v) { put_raw(b, &v, 8); }
void put_svalue(Bytes* b, uint8_t type, const Bytes& body) {
  b->push_back(type);
  put_varuint(b, body.size());
  put_raw(b, body.data(), body.size());
}
Bytes str_body(const std::string& s, uint8_t tag) {
  Bytes b;
  uint32_t l = uint32_t(s.size());
  put_raw(&b, &l, 4);
  put_raw(&b, s.data(), s.size());
  b.push_back(tag);
  return b;
}
Bytes num_body(uint64_t v, uint8_t tag) {
  Bytes b;
  put_u64(&b, v);
  b.push_back(tag);
  return b;
}

// count, sum(float), min, string cell, numeric cell, bool cell, NIL cell
std::vector<LoweredProgram> select_list() {
  std::vector<LoweredProgram> s(7);
  s[0].is_aggregate = true; s[0].aggregate_fn = EVQL_AGG_COUNT; s[0].return_type = EVQL_T_UINT64;
  s[1].is_aggregate = true; s[1].aggregate_fn = EVQL_AGG_SUM_FLOAT64; s[1].return_type = EVQL_T_FLOAT64;
  s[2].is_aggregate = true; s[2].aggregate_fn = EVQL_AGG_MIN_INT64; s[2].return_type = EVQL_T_INT64;
  s[3].return_type = EVQL_T_STRING;
  s[4].return_type = EVQL_T_TIMESTAMP64;
  s[5].return_type = EVQL_T_BOOL;
  s[6].return_type = EVQL_T_NIL;
  return s;
}

Bytes row_cells(uint64_t i, uint8_t cell4_type = EVQL_T_UINT64) {
  Bytes b;
  put_varuint(&b, i * 300);            // count
  put_u64(&b, 0x3ff0000000000000ull);  // sum
  put_varuint(&b, i);                  // min: count, value
  put_u64(&b, uint64_t(-5));
  if (i == 1) {
    put_svalue(&b, EVQL_T_NIL, Bytes());  // a NULL string travels as NIL
  } else {
    put_svalue(&b, EVQL_T_STRING, str_body(std::string(size_t(i) * 70, 'x'), 0x80));
  }
  put_svalue(&b, cell4_type, cell4_type == EVQL_T_BOOL ? Bytes{1, 0} : num_body(77, 0));
  put_svalue(&b, EVQL_T_BOOL, Bytes{1, 0});
  put_svalue(&b, EVQL_T_NIL, Bytes{1});
  return b;
}

Bytes key(uint8_t seed) { return Bytes(20, seed); }

Bytes frame(uint64_t count, const std::vector<Bytes>& rows) {
  Bytes f;
  put_varuint(&f, 1);  // flags
  put_varuint(&f, count);
  for (size_t i = 0; i < rows.size(); ++i) {
    put_raw(&f, key(uint8_t(i)).data(), 20);
    put_raw(&f, rows[i].data(), rows[i].size());
  }
  return f;
}

MergeIndexResult index_exact(const MergeRecordLayout& L, const Bytes& f, size_t len, std::vector<uint32_t>* off) {
  std::unique_ptr<uint8_t[]> exact(new uint8_t[len ? len : 1]);
  if (len) memcpy(exact.get(), f.data(), len);
  return index_merge_frame(L, len ? exact.get() : nullptr, len, off);
}

}  // namespace

int main() {
  MergeRecordLayout L;
  CHECK(merge_record_layout(select_list(), &L) == MLAYOUT_OK);
  CHECK(L.ncols == 7 && L.rw == 3 + 1 + 1 + 2 + 2 + 2 + 2 + 2);
  CHECK(L.cls[2] == MCELL_COUNT_RAW8 && L.op[2] == MFOLD_MIN_I64 && L.word[2] == 5);
  {
    std::vector<LoweredProgram> s = select_list();
    s[0].aggregate_fn = EVQL_AGG_COUNT_DISTINCT_UINT64;
    MergeRecordLayout X;
    CHECK(merge_record_layout(s, &X) == MLAYOUT_AGGREGATE);
    CHECK(merge_record_layout(std::vector<LoweredProgram>(kMaxMergeCols + 1), &X) == MLAYOUT_TOO_WIDE);
  }
  std::vector<uint32_t> off;

  // a well-formed frame of three rows, and every truncation of it
  const std::vector<Bytes> rows = {row_cells(0), row_cells(1), row_cells(2)};
  const Bytes good = frame(3, rows);
  CHECK(index_exact(L, good, good.size(), &off) == MINDEX_OK);
  CHECK(off.size() == 4 && off[0] == 2 && off[3] == good.size());
  for (size_t i = 0; i < 3; ++i) CHECK(off[i + 1] - off[i] == 20 + rows[i].size());
  for (size_t len = 0; len < good.size(); ++len) {
    CHECK(index_exact(L, good, len, &off) == MINDEX_MALFORMED);
    CHECK(off.empty());
  }
  // (bytes behind the last row are not the frame's rows: the host merge ignores them too)
  Bytes trailing = good;
  trailing.push_back(0xff);
  CHECK(index_exact(L, trailing, trailing.size(), &off) == MINDEX_OK && off.size() == 4);

  // zero rows
  CHECK(index_exact(L, frame(0, {}), 2, &off) == MINDEX_OK);
  CHECK(off.size() == 1 && off[0] == 2);
  CHECK(index_exact(L, Bytes(), 0, &off) == MINDEX_MALFORMED);
  CHECK(index_exact(L, Bytes{0}, 1, &off) == MINDEX_MALFORMED);

  // a count the payload cannot hold: refused before anything is reserved
  {
    Bytes f;
    put_varuint(&f, 0);
    put_varuint(&f, 1ull << 60);
    put_raw(&f, key(1).data(), 20);
    CHECK(index_exact(L, f, f.size(), &off) == MINDEX_MALFORMED);
    CHECK(index_exact(L, frame(4, rows), frame(4, rows).size(), &off) == MINDEX_MALFORMED);
  }

  // over-long varuints: the count, a state, an SValue length
  {
    Bytes f{0};
    f.insert(f.end(), 10, 0x80);
    f.push_back(0x01);
    f.insert(f.end(), 64, 0);
    CHECK(index_exact(L, f, f.size(), &off) == MINDEX_MALFORMED);
    Bytes cells(11, 0x80);  // the count state of row 0
    cells.push_back(0);
    cells.insert(cells.end(), rows[0].begin() + 1, rows[0].end());
    const Bytes g = frame(1, {cells});
    CHECK(index_exact(L, g, g.size(), &off) == MINDEX_MALFORMED);
    // ten bytes are the longest varuint there is
    Bytes ten(9, 0x80);
    ten.push_back(0x01);
    ten.insert(ten.end(), rows[0].begin() + 1, rows[0].end());
    const Bytes h = frame(1, {ten});
    CHECK(index_exact(L, h, h.size(), &off) == MINDEX_OK && off.size() == 2);
    Bytes sv;
    put_varuint(&sv, 0);
    put_u64(&sv, 0);
    put_varuint(&sv, 0);
    put_u64(&sv, 0);
    sv.push_back(EVQL_T_STRING);
    sv.insert(sv.end(), 12, 0xff);
    sv.insert(sv.end(), 64, 0);
    const Bytes k = frame(1, {sv});
    CHECK(index_exact(L, k, k.size(), &off) == MINDEX_MALFORMED);
  }

  // length fields that point behind the end, or disagree with each other
  {
    Bytes head;
    put_varuint(&head, 0);
    put_u64(&head, 0);
    put_varuint(&head, 0);
    put_u64(&head, 0);
    Bytes a = head;  // SValue length far behind the payload
    a.push_back(EVQL_T_STRING);
    put_varuint(&a, 1ull << 40);
    a.insert(a.end(), 16, 0);
    CHECK(index_exact(L, frame(1, {a}), frame(1, {a}).size(), &off) == MINDEX_MALFORMED);
    Bytes b = head;  // the string's own length says more than the SValue holds
    Bytes body = str_body("abc", 0);
    body[0] = 200;
    put_svalue(&b, EVQL_T_STRING, body);
    b.insert(b.end(), 300, 0);
    CHECK(index_exact(L, frame(1, {b}), frame(1, {b}).size(), &off) == MINDEX_MALFORMED);
    Bytes c = head;  // ... and 2^32 - 1: no wrap-around
    body[0] = body[1] = body[2] = body[3] = 0xff;
    put_svalue(&c, EVQL_T_STRING, body);
    CHECK(index_exact(L, frame(1, {c}), frame(1, {c}).size(), &off) == MINDEX_MALFORMED);
    Bytes e = head;  // a numeric of the wrong width, an unknown type
    put_svalue(&e, EVQL_T_STRING, str_body("", 0));
    put_svalue(&e, EVQL_T_UINT64, Bytes(8, 0));
    CHECK(index_exact(L, frame(1, {e}), frame(1, {e}).size(), &off) == MINDEX_MALFORMED);
    Bytes u = head;
    put_svalue(&u, 99, Bytes(9, 0));
    CHECK(index_exact(L, frame(1, {u}), frame(1, {u}).size(), &off) == MINDEX_MALFORMED);
  }

  // a cell of another size class than the program's return type
  {
    const Bytes f = frame(1, {row_cells(2, EVQL_T_BOOL)});
    CHECK(index_exact(L, f, f.size(), &off) == MINDEX_CELL_CLASS && off.empty());
    const Bytes g = frame(1, {row_cells(2, EVQL_T_FLOAT64)});  // the same class: any 8-byte numeric
    CHECK(index_exact(L, g, g.size(), &off) == MINDEX_OK);
  }

  // the two SVectors of add_rows
  {
    Bytes keys, data;
    for (size_t i = 0; i < 3; ++i) {
      uint32_t kn = 20, dn = uint32_t(rows[i].size());
      put_raw(&keys, &kn, 4);
      put_raw(&keys, key(uint8_t(i)).data(), 20);
      keys.push_back(0);
      put_raw(&data, &dn, 4);
      put_raw(&data, rows[i].data(), rows[i].size());
      data.push_back(0);
    }
    std::vector<uint32_t> ko, d0, d1;
    auto run = [&](const Bytes& k, size_t klen, const Bytes& d, size_t dlen, size_t n) {
      std::unique_ptr<uint8_t[]> ke(new uint8_t[klen ? klen : 1]), de(new uint8_t[dlen ? dlen : 1]);
      if (klen) memcpy(ke.get(), k.data(), klen);
      if (dlen) memcpy(de.get(), d.data(), dlen);
      return index_merge_rows(L, ke.get(), klen, de.get(), dlen, n, &ko, &d0, &d1);
    };
    CHECK(run(keys, keys.size(), data, data.size(), 3) == MINDEX_OK);
    CHECK(ko.size() == 3 && ko[0] == 4 && ko[1] == 29 && d0[0] == 4 && d1[0] == 4 + rows[0].size());
    CHECK(d1[2] + 1 == data.size());
    CHECK(run(keys, keys.size(), data, data.size(), 0) == MINDEX_OK && ko.empty());
    for (size_t len = 0; len < data.size(); ++len) {
      CHECK(run(keys, keys.size(), data, len, 3) == MINDEX_MALFORMED && ko.empty() && d0.empty());
    }
    for (size_t len = 0; len < keys.size(); ++len) {
      CHECK(run(keys, len, data, data.size(), 3) == MINDEX_MALFORMED);
    }
    CHECK(run(keys, keys.size(), data, data.size(), 4) == MINDEX_MALFORMED);
    Bytes k19 = keys;  // kn != 20
    k19[0] = 19;
    k19.erase(k19.begin() + 4);
    CHECK(run(k19, k19.size(), data, data.size(), 3) == MINDEX_MALFORMED);
    Bytes longer = data;  // an element longer than its cells
    longer[0] += 1;
    longer.insert(longer.begin() + 4 + rows[0].size(), 0);
    CHECK(run(keys, keys.size(), longer, longer.size(), 3) == MINDEX_MALFORMED);
    Bytes past = data;  // an element length behind the end
    past[2] = 0xff;
    CHECK(run(keys, keys.size(), past, past.size(), 3) == MINDEX_MALFORMED);
  }
  printf("ok\n");
  return 0;
}
