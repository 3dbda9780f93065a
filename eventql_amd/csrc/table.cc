// table.cc -- a table's residency in HBM: the image and its page tables, and the decoded
// ("materialised") forms of columns the fused kernel cannot read in place.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include "runtime.h"

namespace evql {

// ---------------------------------------------------------------------------
// tables
// ---------------------------------------------------------------------------
static uint64_t stream_payload_bytes(const std::vector<uint8_t>& img, const ColumnLayout& c,
                                     uint64_t nrows) {
  // encoded bytes actually holding values
  uint64_t total = 0;
  auto bitpacked = [&](const std::vector<PageRef>& pages) -> uint64_t {
    if (pages.empty()) return 0;
    uint32_t maxv;
    memcpy(&maxv, &img[pages[0].offset], 4);
    return 4 + 16ull * bitpack_width(maxv) * ((nrows + 127) / 128);
  };
  auto bytes_used = [&](const std::vector<PageRef>& pages) -> uint64_t {
    if (pages.empty()) return 0;
    uint64_t full = 0;
    for (size_t i = 0; i + 1 < pages.size(); ++i) full += pages[i].size;
    const PageRef& last = pages.back();
    uint64_t used = last.size;
    while (used > 0 && img[last.offset + used - 1] == 0) --used;
    return full + used;
  };
  switch (c.storage_type) {
    case ColumnEncoding::UINT64_PLAIN:
    case ColumnEncoding::FLOAT_IEEE754:
      total += c.dlevel_max == 0 ? 8 * nrows : bytes_used(c.data_pages);
      break;
    case ColumnEncoding::UINT32_PLAIN:
      total += c.dlevel_max == 0 ? 4 * nrows : bytes_used(c.data_pages);
      break;
    case ColumnEncoding::UINT32_BITPACKED:
    case ColumnEncoding::BOOLEAN_BITPACKED:
      total += c.dlevel_max == 0 ? bitpacked(c.data_pages) : bytes_used(c.data_pages);
      break;
    default:
      total += bytes_used(c.data_pages);
  }
  if (c.dlevel_max > 0) total += bitpacked(c.dlevel_pages);
  if (c.rlevel_max > 0) total += bitpacked(c.rlevel_pages);
  return total;
}

Status upload_page_tables(evql_table* t) {
  t->d_pages.assign(t->layout.columns.size(), std::vector<uint64_t*>(3, nullptr));
  for (size_t i = 0; i < t->layout.columns.size(); ++i) {
    const ColumnLayout& c = t->layout.columns[i];
    const std::vector<PageRef>* lists[3] = {&c.data_pages, &c.rlevel_pages, &c.dlevel_pages};
    for (int k = 0; k < 3; ++k) {
      std::vector<uint64_t> offs;
      for (const auto& p : *lists[k]) offs.push_back(p.offset);
      if (offs.empty()) offs.push_back(0);
      // one extra entry so that a tile index one past the end stays in bounds
      offs.push_back(offs.back());
      uint64_t* d = nullptr;
      HIP_TRY(hipMalloc(&d, offs.size() * 8));
      HIP_TRY(hipMemcpyAsync(d, offs.data(), offs.size() * 8, hipMemcpyHostToDevice,
                             t->ctx->stream));
      HIP_TRY(hipStreamSynchronize(t->ctx->stream));
      t->d_pages[i][k] = d;
    }
  }
  return Status();
}

Status table_from_image(evql_ctx* ctx, const void* image, size_t len, bool keep_host,
                        evql_table** out) {
  std::unique_ptr<evql_table> t(new evql_table());
  t->ctx = ctx;
  std::vector<uint8_t> transcoded;
  {
    // v0.1.0 files are re-encoded into the v0.2.0 page layout first (cstable_v1.cc)
    const uint8_t* b = static_cast<const uint8_t*>(image);
    if (len >= 6 && b[0] == 0x23 && b[1] == 0x17 && b[2] == 0x23 && b[3] == 0x17 &&
        (uint32_t(b[4]) | (uint32_t(b[5]) << 8)) == 1) {
      std::string verr = transcode_v1_to_v2(b, len, &transcoded);
      if (!verr.empty()) return Status::error(EVQL_EIO, verr);
      image = transcoded.data();
      len = transcoded.size();
    }
  }
  std::string err = parse_cstable(static_cast<const uint8_t*>(image), len, &t->layout);
  if (!err.empty()) return Status::error(EVQL_EIO, err);
  t->image_len = len;
  const uint8_t* img = static_cast<const uint8_t*>(image);
  std::vector<uint8_t> tmp(img, img + len);
  for (const auto& c : t->layout.columns) {
    t->payload_bytes.push_back(stream_payload_bytes(tmp, c, t->layout.num_rows));
  }
  // 1 MiB of zero slack behind the image keeps speculative vector loads legal
  const size_t slack = 1 << 20;
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&t->d_image), len + slack));
  HIP_TRY(hipMemsetAsync(t->d_image + len, 0, slack, ctx->stream));
  HIP_TRY(hipMemcpyAsync(t->d_image, image, len, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  (void) keep_host;  // nothing of the file is kept on the host
  Status st = upload_page_tables(t.get());
  if (!st.ok()) return st;
  *out = t.release();
  return Status();
}

}  // namespace evql

evql_table::evql_table()
    : narrow_min_rows(evql::narrow_plain_min_rows()),
      narrow_float_min_rows(evql::narrow_float_min_rows()) {}

evql_table::~evql_table() {
  if (d_image) hipFree(d_image);
  for (auto& v : d_pages) {
    for (auto* p : v) {
      if (p) hipFree(p);
    }
  }
  // (the cached decodes -- materialized, dicts, nested_cache, leaf_cache -- free their
  // device arrays themselves)
}

namespace evql {

// ---------------------------------------------------------------------------
// decode-to-SoA ("materialise") of columns the fused kernel cannot read in place
// ---------------------------------------------------------------------------
Status stream_bits(evql_table* t, const std::vector<PageRef>& pages, uint32_t* bits) {
  uint32_t maxv = 0;
  if (!pages.empty()) {
    HIP_TRY(hipMemcpy(&maxv, t->d_image + pages[0].offset, 4, hipMemcpyDeviceToHost));
  }
  *bits = pages.empty() ? 0 : bitpack_width(maxv);
  return Status();
}

// Value boundaries of a STRING_PLAIN column, on the device (aot_kernels.h
// "STRING_PLAIN value boundaries"): d_strval[i] = (len << 40) | position of value i's
// first byte in the virtual byte stream over the column's 512 KiB data pages.
static Status locate_string_values(evql_table* t, const ColumnLayout& c, int li, uint64_t nvalues,
                                   uint64_t* d_strval) {
  hipStream_t s = t->ctx->stream;
  if (nvalues == 0) return Status();
  StrScanArgs a{};
  a.image = t->d_image;
  a.pages = t->d_pages[li][0];
  a.nbytes = uint64_t(c.data_pages.size()) * kPlainPageSize;
  a.nchunks = a.nbytes / kStrChunk;
  a.nvalues = nvalues;
  a.strval = d_strval;
  if (a.nchunks == 0) return Status::error(EVQL_EIO, "end of column reached: " + c.name);
  const uint64_t ngroups = (a.nchunks + kStrGroup - 1) / kStrGroup;
  DevBuf<uint16_t> d_exits, d_hops, d_centry;
  DevBuf<uint32_t> d_gexit, d_ghops, d_status;
  DevBuf<uint64_t> d_gentry, d_gbase, d_cbase;
  HIP_TRY(d_exits.alloc(a.nchunks * kStrEntries * 2));
  HIP_TRY(d_hops.alloc(a.nchunks * kStrEntries * 2));
  HIP_TRY(d_gexit.alloc(ngroups * kStrEntries * 4));
  HIP_TRY(d_ghops.alloc(ngroups * kStrEntries * 4));
  HIP_TRY(d_gentry.alloc(ngroups * 8));
  HIP_TRY(d_gbase.alloc(ngroups * 8));
  HIP_TRY(d_centry.alloc(a.nchunks * 2));
  HIP_TRY(d_cbase.alloc(a.nchunks * 8));
  HIP_TRY(d_status.alloc(16));
  HIP_TRY(hipMemsetAsync(d_status, 0, 16, s));
  a.exits = d_exits;
  a.hops = d_hops;
  a.gexit = d_gexit;
  a.ghops = d_ghops;
  a.gentry = d_gentry;
  a.gbase = d_gbase;
  a.centry = d_centry;
  a.cbase = d_cbase;
  a.status = d_status;
  HIP_TRY(launch_str_chunk_tables(a, s));
  HIP_TRY(launch_str_group_compose(a, s));
  HIP_TRY(launch_str_chain(a, s));
  HIP_TRY(launch_str_chunk_entries(a, s));
  uint32_t status[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(status, d_status, 16, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (status[0] & 1u) {
    // a value outran the chunk tables: locate the chunk entries with the serial walk
    HIP_TRY(hipMemsetAsync(d_status, 0, 16, s));
    HIP_TRY(launch_str_walk_serial(a, s));
    HIP_TRY(hipMemcpyAsync(status, d_status, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  uint64_t found;
  memcpy(&found, &status[2], 8);
  if ((status[0] & 2u) || found < nvalues) {
    return Status::error(EVQL_EIO, "end of column reached: " + c.name);
  }
  HIP_TRY(launch_str_emit(a, s));
  HIP_TRY(hipMemcpyAsync(status, d_status, 16, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (status[0] & 2u) return Status::error(EVQL_EIO, "end of column reached: " + c.name);
  return Status();
}

// values the data pages of a fixed-width encoding can hold (byte streams: no bound,
// their decoders stop at the end of the stream)
static uint64_t fixed_width_capacity(const ColumnLayout& c) {
  switch (c.storage_type) {
    case ColumnEncoding::UINT64_PLAIN:
    case ColumnEncoding::FLOAT_IEEE754:
      return uint64_t(c.data_pages.size()) * (kPlainPageSize / 8);
    case ColumnEncoding::UINT32_PLAIN:
      return uint64_t(c.data_pages.size()) * (kPlainPageSize / 4);
    case ColumnEncoding::UINT32_BITPACKED:
    case ColumnEncoding::BOOLEAN_BITPACKED:
      return c.data_pages.empty() ? ~0ull
                                  : uint64_t(c.data_pages.size()) * kBitpackBlocksPerPage * 128;
    default:
      return ~0ull;
  }
}

// the buffer of a narrow copy of `n` values of `bits` bits (runtime.h narrow_copy_bytes):
// everything behind the value pairs that the caller's launch_narrow_flat writes is zeroed,
// the maximum word stored
static Status alloc_narrow_copy(hipStream_t s, uint64_t n, uint32_t bits, DevBuf<uint8_t>* d_packed) {
  const uint64_t bytes = narrow_copy_bytes(n, bits);
  HIP_TRY(d_packed->alloc(bytes));
  const uint64_t written = (n + 1) / 2 * 2 * (bits / 8);
  HIP_TRY(hipMemsetAsync(d_packed->p + written, 0, bytes - written, s));
  const uint32_t maxw = bits >= 32 ? 0xffffffffu : ((1u << bits) - 1u);
  HIP_TRY(hipMemcpyAsync(d_packed->p + narrow_copy_max_word_at(n, bits), &maxw, 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));  // (maxw lives until here)
  return Status();
}

// `n` u64 values as a narrow copy of the narrowest of 8 / 16 / 32 bits that holds their
// maximum; *bits = 0 when it does not fit 32 bits.
Status pack_narrow(hipStream_t s, const uint64_t* d_values, uint64_t n, DevBuf<uint8_t>* d_packed,
                   uint32_t* bits_out) {
  *bits_out = 0;
  if (n == 0) return Status();
  DevBuf<uint64_t> d_max;
  HIP_TRY(d_max.alloc(8));
  HIP_TRY(hipMemsetAsync(d_max, 0, 8, s));
  HIP_TRY(launch_max_u64(d_values, n, d_max, s));
  uint64_t maxv = 0;
  HIP_TRY(hipMemcpyAsync(&maxv, d_max, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (maxv > 0xffffffffull) return Status();
  const uint32_t bits = maxv <= 0xffu ? 8 : (maxv <= 0xffffu ? 16 : 32);
  Status st = alloc_narrow_copy(s, n, bits, d_packed);
  if (!st.ok()) return st;
  HIP_TRY(launch_narrow_flat(nullptr, nullptr, d_values, d_packed->p, n, bits, s));
  HIP_TRY(hipStreamSynchronize(s));
  *bits_out = bits;
  return Status();
}

// EVQL_NARROW_PLAIN: 0 = PLAIN columns are never kept narrow, N = in tables of at least N rows
uint64_t narrow_plain_min_rows() {
  if (const char* e = getenv("EVQL_NARROW_PLAIN")) {
    char* end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    if (end != e) return v == 0 ? ~0ull : v;  // 0 = off
  }
  return kNarrowMinRows;
}

// Required UINT64_PLAIN column `li`, whose maximum is `maxv`, once more as a narrow copy
// of the narrowest of 8 / 16 / 32 bits -- t->materialized[name] with packed_bits set and no
// 8-byte words, what a required LEB128 column leaves there.  The file's own pages stay
// (download_image, the LSM paths and table_rt_column read them).  No entry when the
// maximum does not fit 32 bits.
Status narrow_plain_column(evql_table* t, int li, uint64_t maxv) {
  static_assert(kPlain64PageValues == kPlainPageSize / 8, "k_narrow_flat's source page size");
  const ColumnLayout& c = t->layout.columns[li];
  const uint64_t n = t->layout.num_rows;
  if (t->materialized.count(c.name) || maxv > 0xffffffffull || n == 0) return Status();
  if (n > uint64_t(c.data_pages.size()) * (kPlainPageSize / 8)) return Status();  // (short file)
  hipStream_t s = t->ctx->stream;
  const uint32_t bits = maxv <= 0xffu ? 8 : (maxv <= 0xffffu ? 16 : 32);
  MaterializedColumn m;
  DevBuf<uint8_t> d_packed;
  Status st = alloc_narrow_copy(s, n, bits, &d_packed);
  if (!st.ok()) return st;
  HIP_TRY(launch_narrow_flat(t->d_image, t->d_pages[li][0], nullptr, d_packed.p, n, bits, s));
  HIP_TRY(hipStreamSynchronize(s));
  m.d_packed = d_packed.release();
  m.packed_bits = bits;
  t->materialized[c.name] = std::move(m);
  return Status();
}

// EVQL_NARROW_FLOAT: 0 = FLOAT_IEEE754 columns are never kept as float32, N = in tables of at
// least N rows.  EVQL_NARROW_PLAIN=0 ("the file's own pages") turns these copies off as
// well; any other value of it leaves this threshold alone.
uint64_t narrow_float_min_rows() {
  if (narrow_plain_min_rows() == ~0ull) return ~0ull;
  if (const char* e = getenv("EVQL_NARROW_FLOAT")) {
    char* end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    if (end != e) return v == 0 ? ~0ull : v;  // 0 = off
  }
  return kNarrowMinRows;
}

// Required FLOAT_IEEE754 column `li` once more as float32 -- t->materialized[name] with
// packed_bits = 32 and packed_f32 -- when every value is exactly a float32 zero, normal
// number, infinity or quiet NaN (k_narrow_f32): widening gives back the file's 64 bits, so
// the fused kernel streams 4 bytes per row for the same result.  One pass, one host wait.
// A column with any other value is remembered in t->narrow_float_refused and keeps its
// pages.  The file's own pages stay either way (row-addressed readers use them).
Status narrow_float_column(evql_table* t, int li) {
  const ColumnLayout& c = t->layout.columns[li];
  const uint64_t n = t->layout.num_rows;
  if (t->materialized.count(c.name) || t->narrow_float_refused.count(c.name) || n == 0) return Status();
  if (n > uint64_t(c.data_pages.size()) * (kPlainPageSize / 8)) return Status();  // (short file)
  hipStream_t s = t->ctx->stream;
  const uint64_t bytes = narrow_copy_bytes(n, 32);
  DevBuf<uint8_t> d_packed;
  DevBuf<uint32_t> d_refused;
  HIP_TRY(d_packed.alloc(bytes));
  HIP_TRY(d_refused.alloc(4));
  // zero behind the value pairs the kernel writes, then the maximum word of a 32-bit copy
  const uint64_t written = (n + 1) / 2 * 8;
  HIP_TRY(hipMemsetAsync(d_packed.p + written, 0, bytes - written, s));
  HIP_TRY(hipMemsetAsync(d_packed.p + narrow_copy_max_word_at(n, 32), 0xff, 4, s));
  HIP_TRY(hipMemsetAsync(d_refused.p, 0, 4, s));
  HIP_TRY(launch_narrow_f32(t->d_image, t->d_pages[li][0], d_packed.p, n, d_refused.p, s));
  uint32_t refused = 0;
  HIP_TRY(hipMemcpyAsync(&refused, d_refused.p, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  ++t->narrow_float_passes;
  if (refused) {
    t->narrow_float_refused.insert(c.name);
    return Status();  // (d_packed is freed here)
  }
  MaterializedColumn m;
  m.d_packed = d_packed.release();
  m.packed_bits = 32;
  m.packed_f32 = true;
  t->materialized[c.name] = std::move(m);
  return Status();
}

Status defined_value_source(evql_table* t, int li, uint64_t nvalues, uint64_t* dst, RtColumn* src,
                            DevBuf<uint64_t>* owned) {
  const ColumnLayout& c = t->layout.columns[li];
  hipStream_t s = t->ctx->stream;
  if (nvalues > fixed_width_capacity(c)) {
    // fewer data pages than defined values (column_reader_uint.cc raises
    // "end of column reached" when it gets there)
    return Status::error(EVQL_EIO, "end of column reached: " + c.name);
  }
  *src = RtColumn{};
  src->pages = t->d_pages[li][0];
  switch (c.storage_type) {
    case ColumnEncoding::UINT64_PLAIN:
    case ColumnEncoding::FLOAT_IEEE754:
      src->mode = ColAccess::PLAIN64;
      return Status();
    case ColumnEncoding::UINT32_PLAIN:
      src->mode = ColAccess::PLAIN32;
      return Status();
    case ColumnEncoding::UINT32_BITPACKED:
    case ColumnEncoding::BOOLEAN_BITPACKED:
      src->mode = ColAccess::BITPACKED;
      return stream_bits(t, c.data_pages, &src->bits);
    case ColumnEncoding::UINT64_LEB128: {
      const uint64_t nbytes = uint64_t(c.data_pages.size()) * kPlainPageSize;
      const uint64_t nchunks = (nbytes + kLebChunk - 1) / kLebChunk;
      DevBuf<uint64_t> d_chunks;
      HIP_TRY(d_chunks.alloc((nchunks + 1) * 8));
      if (!dst) {
        HIP_TRY(owned->alloc(nvalues * 8));
        dst = *owned;
      }
      if (nchunks) {
        HIP_TRY(launch_leb128_count(t->d_image, t->d_pages[li][0], nbytes, d_chunks, s));
        HIP_TRY(launch_exclusive_scan(d_chunks, nchunks, nullptr, s));
        HIP_TRY(launch_leb128_decode(t->d_image, t->d_pages[li][0], nbytes, d_chunks, nvalues, dst,
                                     s));
      }
      HIP_TRY(hipStreamSynchronize(s));
      src->mode = ColAccess::SOA;
      src->soa = dst;
      return Status();
    }
    case ColumnEncoding::STRING_PLAIN: {
      // a string slot's "value" is where its bytes are: (len << 40) | position
      HIP_TRY(owned->alloc(std::max<uint64_t>(nvalues, 1) * 8));
      Status st = locate_string_values(t, c, li, nvalues, *owned);
      if (!st.ok()) return st;
      src->mode = ColAccess::SOA;
      src->soa = *owned;
      return Status();
    }
    default:
      return Status::error(EVQL_ENOTSUP, "unsupported column encoding");
  }
}

Status materialize_column(evql_table* t, const ColAccess& ca) {
  evql_ctx* ctx = t->ctx;
  const ColumnLayout& c = t->layout.columns[ca.layout_index];
  if (t->materialized.count(c.name)) return Status();
  MaterializedColumn m;
  const uint64_t n = t->layout.num_rows;
  const uint64_t np = padded_rows(n);
  hipStream_t s = ctx->stream;
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&m.d_values), np * 8));
  HIP_TRY(hipMemsetAsync(m.d_values, 0, np * 8, s));
  const int li = ca.layout_index;

  if (c.logical_type == ColumnType::STRING) {
    // per row: tag, (len << 40 | position) and a 64-bit hash of the bytes -- all
    // computed on the device from the pages in HBM (no host copy of the file)
    m.string_hash = true;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&m.d_tags), np));
    HIP_TRY(hipMemsetAsync(m.d_tags, 0, np, s));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&m.d_strpos), np * 8));
    HIP_TRY(hipMemsetAsync(m.d_strpos, 0, np * 8, s));
    uint64_t nvalues = n;
    DevBuf<uint64_t> d_tiles;
    const uint64_t ntiles = (n + kDecodeTile - 1) / kDecodeTile;
    if (c.dlevel_max > 0) {
      HIP_TRY(hipMemsetAsync(m.d_tags, 1, np, s));
      HIP_TRY(d_tiles.alloc((ntiles + 1) * 8));
      uint32_t dbits = 0;
      Status st = stream_bits(t, c.dlevel_pages, &dbits);
      if (!st.ok()) return st;
      HIP_TRY(launch_dlevel_tags(t->d_image, t->d_pages[li][2], dbits, c.dlevel_max, n, m.d_tags,
                                 d_tiles, s));
      uint64_t* d_total = d_tiles.p + ntiles;
      HIP_TRY(launch_exclusive_scan(d_tiles, ntiles, d_total, s));
      HIP_TRY(hipMemcpyAsync(&nvalues, d_total, 8, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      DevBuf<uint64_t> d_strval;
      HIP_TRY(d_strval.alloc(nvalues * 8));
      Status st2 = locate_string_values(t, c, li, nvalues, d_strval);
      if (!st2.ok()) return st2;
      RtColumn src{};
      src.mode = ColAccess::SOA;
      src.soa = d_strval;
      HIP_TRY(launch_expand_nullable(t->d_image, src, m.d_tags, d_tiles, n, m.d_strpos, s));
      HIP_TRY(hipStreamSynchronize(s));
    } else {
      Status st2 = locate_string_values(t, c, li, n, m.d_strpos);
      if (!st2.ok()) return st2;
    }
    HIP_TRY(launch_string_hash(t->d_image, t->d_pages[li][0], m.d_strpos, n, m.d_values, s));
    HIP_TRY(hipStreamSynchronize(s));
    t->materialized[c.name] = std::move(m);
    return Status();
  }

  uint64_t nvalues = n;
  DevBuf<uint64_t> d_tiles;
  const uint64_t ntiles = (n + kDecodeTile - 1) / kDecodeTile;

  if (c.dlevel_max > 0) {
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&m.d_tags), np));
    HIP_TRY(hipMemsetAsync(m.d_tags, 1, np, s));
    HIP_TRY(d_tiles.alloc((ntiles + 1) * 8));
    uint32_t dbits = 0;
    Status st = stream_bits(t, c.dlevel_pages, &dbits);
    if (!st.ok()) return st;
    HIP_TRY(launch_dlevel_tags(t->d_image, t->d_pages[li][2], dbits, c.dlevel_max, n, m.d_tags,
                               d_tiles, s));
    uint64_t* d_total = d_tiles.p + ntiles;
    HIP_TRY(launch_exclusive_scan(d_tiles, ntiles, d_total, s));
    HIP_TRY(hipMemcpyAsync(&nvalues, d_total, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }

  if (c.storage_type == ColumnEncoding::STRING_PLAIN) {  // (not as a STRING column: above)
    return Status::error(EVQL_ENOTSUP, "unsupported column encoding");
  }
  // a non-nullable LEB128 column decodes straight into its SoA array; a nullable one
  // into a dense array that the expansion below reads by value index
  RtColumn src{};
  DevBuf<uint64_t> d_dense;
  Status sts = defined_value_source(t, li, nvalues, c.dlevel_max > 0 ? nullptr : m.d_values, &src,
                                    &d_dense);
  if (!sts.ok()) return sts;

  if (c.dlevel_max > 0) {
    HIP_TRY(launch_expand_nullable(t->d_image, src, m.d_tags, d_tiles, n, m.d_values, s));
    HIP_TRY(hipStreamSynchronize(s));
  } else if (c.storage_type == ColumnEncoding::UINT64_LEB128 && n > 0) {
    // Required LEB128 column (the reference's default integer encoding,
    // TableSchema.cc:290-316): keep it in HBM as a flat array of the narrowest of
    // 8 / 16 / 32 bits per value that holds its maximum instead of 8-byte words.  The
    // fused kernel then streams fewer bytes than the LEB128 stream itself holds for
    // multi-byte values, with no decode but a zero extension.  Decoding LEB128 inside the fused kernel instead would
    // cost ~10 lane-operations per stream byte (terminator scan + extraction) against
    // the ~12 the chip has per HBM byte at 6.3 TB/s for the whole query.
    uint32_t bits = 0;
    DevBuf<uint8_t> d_packed;
    Status stp = pack_narrow(s, m.d_values, n, &d_packed, &bits);
    if (!stp.ok()) return stp;
    m.d_packed = d_packed.release();
    if (bits) {
      m.packed_bits = bits;
      hipFree(m.d_values);  // the 8-byte words are not needed any more
      m.d_values = nullptr;
    }
  }
  t->materialized[c.name] = std::move(m);
  return Status();
}

// Row-addressable view of one flat column for the AOT kernels (lsm.cc): direct
// page access where the encoding allows it, the cached SoA decode otherwise.
// For STRING columns *strpos receives the device array of (len << 40 | position).
Status table_rt_column(evql_table* t, const std::string& name, RtColumn* out,
                       const uint64_t** strpos) {
  int li = -1;
  for (size_t k = 0; k < t->layout.columns.size(); ++k) {
    if (t->layout.columns[k].name == name) li = int(k);
  }
  if (li < 0) return Status::error(EVQL_EARG, "column not found: " + name);
  const ColumnLayout& cl = t->layout.columns[li];
  if (cl.rlevel_max > 0) return Status::error(EVQL_ENOTSUP, "repeated column: " + name);
  ColAccess c;
  c.name = name;
  c.layout_index = li;
  c.stype = EVQL_T_UINT64;
  *out = RtColumn{};
  out->pages = t->d_pages[li][0];
  if (cl.logical_type == ColumnType::STRING) {
    c.stype = EVQL_T_STRING;
    c.mode = ColAccess::SOA;
    c.string_hash = c.string_bytes = c.has_tags = true;
  } else {
    switch (cl.storage_type) {
      case ColumnEncoding::UINT64_PLAIN:
      case ColumnEncoding::FLOAT_IEEE754: c.mode = ColAccess::PLAIN64; break;
      case ColumnEncoding::UINT32_PLAIN: c.mode = ColAccess::PLAIN32; break;
      case ColumnEncoding::UINT32_BITPACKED:
      case ColumnEncoding::BOOLEAN_BITPACKED: c.mode = ColAccess::BITPACKED; break;
      default: c.mode = ColAccess::SOA;
    }
    if (cl.dlevel_max > 0) {
      c.mode = ColAccess::SOA;
      c.has_tags = true;
    }
  }
  if (c.mode == ColAccess::BITPACKED) {
    Status st = stream_bits(t, cl.data_pages, &out->bits);
    if (!st.ok()) return st;
  } else if (c.mode == ColAccess::SOA) {
    Status st = materialize_column(t, c);
    if (!st.ok()) return st;
    const MaterializedColumn& m = t->materialized[name];
    out->soa = m.d_values;
    out->tags = m.d_tags;
    if (strpos) *strpos = m.d_strpos;
    if (m.packed_bits) {
      c.mode = ColAccess::NARROW;
      out->bits = m.packed_bits;
      out->pages = nullptr;
      out->base = m.d_packed;
    }
  }
  out->mode = uint32_t(c.mode);
  return Status();
}

}  // namespace evql
