// nested.cc -- the Dremel flatteners: repeated / optional columns decoded to one value per
// output row of a nested scan.
#include <algorithm>
#include <cstring>
#include "runtime.h"

namespace evql {

// ---------------------------------------------------------------------------
// nested (Dremel) scans: CSTableScan::fetchNext with NO_AGGREGATION
// (sql/CSTableScan.cc:187-541) as data-parallel passes.
//
// One output row per slot of the deepest referenced column (the "leaf").  A
// column X at a shallower repetition depth repeats its current value, i.e. row j
// reads X's slot  #{ i <= j : r_leaf[i] <= rlevel_max(X) } - 1.  Undefined slots
// (d < dlevel_max) read as value 0 with tag 0 (an all-zero `SValue()`,
// svalue.cc:154-160 -- NOT a NULL tag).  The number of real slots is where record
// number `num_rows` would start (bit-packed streams are zero-padded).
// ---------------------------------------------------------------------------
static uint64_t level_stream_capacity(const std::vector<PageRef>& pages, uint32_t bits) {
  if (bits == 0) return 0;
  uint64_t blocks = 0;
  for (size_t i = 0; i < pages.size(); ++i) {
    uint64_t bytes = pages[i].size - (i == 0 ? 4 : 0);
    blocks += bytes / (16ull * bits);
  }
  return blocks * 128;
}

// Decodes the `nslots` levels of stream `which` (1 repetition, 2 definition) of column
// `li` to one byte per slot and leaves in counts[k], k < n, the scanned per-tile counts of
// the slots at level <= thr[k].
static Status decode_levels(evql_table* t, int li, int which, uint32_t bits, uint64_t nslots,
                            uint8_t* levels, size_t n, const uint32_t* thr,
                            const DevBuf<uint64_t>* counts) {
  hipStream_t s = t->ctx->stream;
  LevelDecodeArgs la{};
  la.image = t->d_image;
  la.pages = t->d_pages[li][which];
  la.bits = bits;
  la.nslots = nslots;
  la.levels = levels;
  for (int k = 0; k < 4; ++k) la.thr[k] = 255;
  for (size_t k = 0; k < n; ++k) {
    la.counts[k] = counts[k];
    la.thr[k] = thr[k];
  }
  HIP_TRY(launch_level_decode(la, s));
  const uint64_t ntiles = (nslots + kDecodeTile - 1) / kDecodeTile;
  for (size_t k = 0; k < n; ++k) HIP_TRY(launch_exclusive_scan(counts[k], ntiles, nullptr, s));
  return Status();
}

// slot values of one (possibly repeated / optional) column: vals[slot] = defined
// ? data value : 0, for every slot of its level streams (or `nslots` when the
// column has no definition levels)
static Status nested_slot_values(evql_table* t, int li, uint64_t nslots_flat,
                                 DevBuf<uint64_t>* out_vals, uint64_t* out_cap) {
  evql_ctx* ctx = t->ctx;
  hipStream_t s = ctx->stream;
  const ColumnLayout& c = t->layout.columns[li];
  // a column without definition levels is required and top-level: one slot per record
  if (c.dlevel_max == 0) nslots_flat = t->layout.num_rows;
  uint64_t cap = nslots_flat;
  DevBuf<uint8_t> d_tags;
  DevBuf<uint64_t> d_tiles;
  uint64_t nvalues = nslots_flat;
  uint32_t dbits = 0;
  if (c.dlevel_max > 0) {
    Status st = stream_bits(t, c.dlevel_pages, &dbits);
    if (!st.ok()) return st;
    cap = dbits ? level_stream_capacity(c.dlevel_pages, dbits) : nslots_flat;
  }
  const uint64_t capp = padded_rows(cap);
  const uint64_t ntiles = (cap + kDecodeTile - 1) / kDecodeTile;
  HIP_TRY(d_tags.alloc(capp));
  HIP_TRY(d_tiles.alloc((ntiles + 2) * 8));
  if (c.dlevel_max > 0) {
    DevBuf<uint8_t> d_lv;
    HIP_TRY(d_lv.alloc(capp));
    HIP_TRY(hipMemsetAsync(d_lv, 0xff, capp, s));
    if (dbits == 0) {
      // every slot has definition level 0
      HIP_TRY(hipMemsetAsync(d_lv, 0, capp, s));
    } else {
      Status st = decode_levels(t, li, 2, dbits, cap, d_lv, 0, nullptr, nullptr);
      if (!st.ok()) return st;
    }
    HIP_TRY(launch_defined_from_levels(d_lv, c.dlevel_max, cap, d_tags, d_tiles, s));
    uint64_t* d_total = d_tiles.p + ntiles;
    HIP_TRY(launch_exclusive_scan(d_tiles, ntiles, d_total, s));
    HIP_TRY(hipMemcpyAsync(&nvalues, d_total, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  } else {
    HIP_TRY(hipMemsetAsync(d_tags, 0, capp, s));
    std::vector<uint64_t> offs(ntiles + 1);
    for (uint64_t i = 0; i <= ntiles; ++i) offs[i] = i * kDecodeTile;
    HIP_TRY(hipMemcpyAsync(d_tiles, offs.data(), (ntiles + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  RtColumn src{};
  DevBuf<uint64_t> d_dense;
  Status st = defined_value_source(t, li, nvalues, nullptr, &src, &d_dense);
  if (!st.ok()) return st;
  DevBuf<uint64_t> d_vals;
  HIP_TRY(d_vals.alloc(capp * 8));
  HIP_TRY(hipMemsetAsync(d_vals, 0, capp * 8, s));
  HIP_TRY(launch_expand_nullable(t->d_image, src, d_tags, d_tiles, cap, d_vals, s));
  HIP_TRY(hipStreamSynchronize(s));
  *out_vals = std::move(d_vals);
  *out_cap = cap;
  return Status();
}

// number of (r, d, value) slots a repeated column holds for the table's records:
// where record number `num_rows` would start in its (zero-padded) repetition levels
static Status exact_slot_count(evql_table* t, int li, uint64_t* out) {
  const ColumnLayout& c = t->layout.columns[li];
  const uint64_t nrec = t->layout.num_rows;
  if (c.rlevel_max == 0) {
    *out = nrec;
    return Status();
  }
  hipStream_t s = t->ctx->stream;
  uint32_t rbits = 0;
  Status st = stream_bits(t, c.rlevel_pages, &rbits);
  if (!st.ok()) return st;
  if (rbits == 0) return Status::error(EVQL_ENOTSUP, "repeated column without repetition levels");
  const uint64_t cap = level_stream_capacity(c.rlevel_pages, rbits);
  const uint64_t capp = padded_rows(cap);
  const uint64_t ntiles = (cap + kDecodeTile - 1) / kDecodeTile;
  DevBuf<uint8_t> d_lv;
  DevBuf<uint64_t> d_cnt, d_n;
  HIP_TRY(d_lv.alloc(capp));
  HIP_TRY(hipMemsetAsync(d_lv, 0xff, capp, s));
  HIP_TRY(d_cnt.alloc((ntiles + 2) * 8));
  HIP_TRY(d_n.alloc(8));
  const uint32_t thr0 = 0;
  st = decode_levels(t, li, 1, rbits, cap, d_lv, 1, &thr0, &d_cnt);
  if (!st.ok()) return st;
  uint64_t n = cap;
  HIP_TRY(hipMemcpyAsync(d_n, &n, 8, hipMemcpyHostToDevice, s));
  HIP_TRY(launch_find_nth(d_lv, d_cnt, cap, 0, nrec, d_n, s));
  HIP_TRY(hipMemcpyAsync(&n, d_n, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *out = n;
  return Status();
}

Status nested_column_slots(evql_table* t, int li, ColumnSlots* out) {
  const ColumnLayout& c = t->layout.columns[li];
  hipStream_t s = t->ctx->stream;
  const uint64_t nrec = t->layout.num_rows;
  *out = ColumnSlots();
  out->nslots = nrec;
  if (c.rlevel_max > 0) {
    uint32_t rbits = 0;
    Status st = stream_bits(t, c.rlevel_pages, &rbits);
    if (!st.ok()) return st;
    if (rbits == 0) return Status::error(EVQL_ENOTSUP, "repeated column without repetition levels");
    const uint64_t cap = level_stream_capacity(c.rlevel_pages, rbits);
    auto hit = t->leaf_cache.find(li);
    if (hit != t->leaf_cache.end()) {
      out->rlevels = hit->second.levels;
      out->rec_offsets = hit->second.rec_offsets;
    } else {
      const uint64_t capp = padded_rows(cap);
      const uint64_t ntiles = (cap + kDecodeTile - 1) / kDecodeTile;
      HIP_TRY(out->rlevels_owned.alloc(capp));
      HIP_TRY(hipMemsetAsync(out->rlevels_owned, 0xff, capp, s));
      HIP_TRY(out->rec_offsets_owned.alloc((ntiles + 2) * 8));
      const uint32_t thr0 = 0;
      st = decode_levels(t, li, 1, rbits, cap, out->rlevels_owned, 1, &thr0, &out->rec_offsets_owned);
      if (!st.ok()) return st;
      out->rlevels = out->rlevels_owned;
      out->rec_offsets = out->rec_offsets_owned;
    }
    // number of real slots = start of record number `nrec` (the stream is zero-padded)
    DevBuf<uint64_t> d_n;
    HIP_TRY(d_n.alloc(8));
    uint64_t n = cap;
    HIP_TRY(hipMemcpyAsync(d_n, &n, 8, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_find_nth(out->rlevels, out->rec_offsets, cap, 0, nrec, d_n, s));
    HIP_TRY(hipMemcpyAsync(&n, d_n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    out->nslots = n;
  }
  if (c.dlevel_max > 0) {
    uint32_t dbits = 0;
    Status st = stream_bits(t, c.dlevel_pages, &dbits);
    if (!st.ok()) return st;
    const uint64_t cap = dbits ? level_stream_capacity(c.dlevel_pages, dbits) : out->nslots;
    if (cap < out->nslots) return Status::error(EVQL_EIO, "end of column reached: " + c.name);
    const uint64_t capp = padded_rows(cap);
    HIP_TRY(out->dlevels_owned.alloc(capp));
    HIP_TRY(hipMemsetAsync(out->dlevels_owned, dbits ? 0xff : 0, capp, s));
    if (dbits) {
      st = decode_levels(t, li, 2, dbits, cap, out->dlevels_owned, 0, nullptr, nullptr);
      if (!st.ok()) return st;
    }
    out->dlevels = out->dlevels_owned;
  }
  uint64_t vcap = 0;
  Status st = nested_slot_values(t, li, out->nslots, &out->values_owned, &vcap);
  if (!st.ok()) return st;
  if (vcap < out->nslots) return Status::error(EVQL_EIO, "end of column reached: " + c.name);
  out->values = out->values_owned;
  return Status();
}

// flattens `cols` (all of one ancestor chain) to one value per leaf slot:
// (*flat)[i] is borrowed from the table's nested cache
Status materialize_nested(evql_query* q, const std::vector<ColAccess>& cols,
                          std::vector<uint64_t*>* flat_out, uint64_t* nrows_out,
                          const LeafLevels** keep, std::vector<uint64_t*>* strpos_out) {
  evql_table* t = q->table;
  evql_ctx* ctx = q->ctx;
  hipStream_t s = ctx->stream;
  struct {
    const std::vector<ColAccess>& cols;
  } kp{cols};
  std::vector<uint64_t*>& nested_flat = *flat_out;
  const uint64_t nrec = t->layout.num_rows;
  nested_flat.assign(kp.cols.size(), nullptr);
  if (strpos_out) strpos_out->assign(kp.cols.size(), nullptr);
  // a string column's row value is (len << 40 | position); the kernels group and
  // compare on its hash (`flat`) and read the bytes through the position (`strpos`)
  auto publish = [&](size_t i, const evql_table::NestedFlat& e) {
    if (kp.cols[i].string_hash) {
      nested_flat[i] = e.d_hash;
      if (strpos_out) (*strpos_out)[i] = e.d_values;
    } else {
      nested_flat[i] = e.d_values;
    }
  };
  if (kp.cols.empty()) {
    *nrows_out = nrec;  // fetchNextWithoutColumns: one row per record
    return Status();
  }
  // leaf = deepest referenced column
  int leaf = 0;
  for (size_t i = 0; i < kp.cols.size(); ++i) {
    if (t->layout.columns[kp.cols[i].layout_index].rlevel_max >
        t->layout.columns[kp.cols[leaf].layout_index].rlevel_max) {
      leaf = int(i);
    }
  }
  const ColumnLayout& lc = t->layout.columns[kp.cols[leaf].layout_index];
  const int leaf_li = kp.cols[leaf].layout_index;
  q->nested_leaf = leaf_li;
  {
    // every column already flattened for this leaf by an earlier operator?
    bool all = keep == nullptr || lc.rlevel_max == 0 || t->leaf_cache.count(leaf_li);
    for (const auto& c : kp.cols) all = all && t->nested_cache.count({c.layout_index, leaf_li});
    if (all) {
      if (keep && lc.rlevel_max > 0) *keep = &t->leaf_cache[leaf_li];
      for (size_t i = 0; i < kp.cols.size(); ++i) {
        const auto& e = t->nested_cache[{kp.cols[i].layout_index, leaf_li}];
        publish(i, e);
        *nrows_out = e.nflat;
      }
      return Status();
    }
  }
  uint64_t nflat = nrec;
  uint64_t leaf_cap = 0;
  DevBuf<uint8_t> d_leaf_levels;
  std::vector<uint32_t> thr_levels;            // distinct parent rlevel_max values
  std::vector<DevBuf<uint64_t>> thr_offsets;   // scanned per-tile counts per threshold
  if (lc.rlevel_max > 0) {
    uint32_t rbits = 0;
    Status st = stream_bits(t, lc.rlevel_pages, &rbits);
    if (!st.ok()) return st;
    const uint64_t cap = level_stream_capacity(lc.rlevel_pages, rbits);
    leaf_cap = cap;
    const uint64_t capp = padded_rows(cap);
    const uint64_t ntiles = (cap + kDecodeTile - 1) / kDecodeTile;
    thr_levels.push_back(0);
    for (const auto& c : kp.cols) {
      uint32_t rm = t->layout.columns[c.layout_index].rlevel_max;
      if (rm >= lc.rlevel_max) continue;
      bool seen = false;
      for (auto x : thr_levels) seen = seen || x == rm;
      if (!seen) thr_levels.push_back(rm);
    }
    if (thr_levels.size() > 4) {
      return Status::error(EVQL_ENOTSUP, "more than four repetition depths in one nested scan");
    }
    HIP_TRY(d_leaf_levels.alloc(capp));
    HIP_TRY(hipMemsetAsync(d_leaf_levels, 0xff, capp, s));
    thr_offsets.resize(thr_levels.size());
    for (auto& d : thr_offsets) HIP_TRY(d.alloc((ntiles + 2) * 8));
    if (rbits == 0) {
      return Status::error(EVQL_ENOTSUP, "repeated column without repetition levels");
    }
    st = decode_levels(t, leaf_li, 1, rbits, cap, d_leaf_levels, thr_levels.size(),
                       thr_levels.data(), thr_offsets.data());
    if (!st.ok()) return st;
    // number of real slots = start of record number `nrec`
    DevBuf<uint64_t> d_n;
    HIP_TRY(d_n.alloc(8));
    HIP_TRY(hipMemcpyAsync(d_n, &cap, 8, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_find_nth(d_leaf_levels, thr_offsets[0], cap, 0, nrec, d_n, s));
    HIP_TRY(hipMemcpyAsync(&nflat, d_n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  *nrows_out = nflat;
  const uint8_t* leaf_levels = d_leaf_levels.p;
  const uint64_t flatp = padded_rows(nflat);
  for (size_t i = 0; i < kp.cols.size(); ++i) {
    // the same column referenced twice shares one buffer
    const int li = kp.cols[i].layout_index;
    {
      // (the same column referenced twice, or flattened by an earlier operator)
      auto hit = t->nested_cache.find({li, leaf_li});
      if (hit != t->nested_cache.end()) {
        publish(i, hit->second);
        continue;
      }
    }
    const ColumnLayout& c = t->layout.columns[li];
    DevBuf<uint64_t> d_vals;
    uint64_t cap = 0;
    Status st = nested_slot_values(t, li, nflat, &d_vals, &cap);
    if (!st.ok()) return st;
    if (c.rlevel_max > 0 && li != leaf_li) {
      // exact ancestor-chain check (the planner's is on names only): a column on the
      // leaf's chain has one slot per leaf slot whose repetition level does not
      // exceed the column's depth.  A sibling repeated group passes only by
      // coincidence of every count.
      uint64_t own = 0;
      st = exact_slot_count(t, li, &own);
      if (!st.ok()) return st;
      bool chain = false;
      if (c.rlevel_max >= lc.rlevel_max) {
        chain = own == nflat;
      } else {
        size_t k = 0;
        while (thr_levels[k] != c.rlevel_max) ++k;
        // the own-th (0-based) leaf slot with r <= depth must be the first padding slot
        DevBuf<uint64_t> d_n;
        HIP_TRY(d_n.alloc(8));
        uint64_t at = ~0ull;
        HIP_TRY(hipMemcpyAsync(d_n, &at, 8, hipMemcpyHostToDevice, s));
        HIP_TRY(launch_find_nth(leaf_levels, thr_offsets[k], leaf_cap, c.rlevel_max, own, d_n, s));
        HIP_TRY(hipMemcpyAsync(&at, d_n, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        // (a leaf stream without a padding slot cannot be probed this way)
        chain = at == nflat || nflat == leaf_cap;
      }
      if (!chain) {
        return Status::error(EVQL_ENOTSUP, "nested columns from different repeated groups");
      }
    }
    // (built completely, then cached: a failure leaves no half-made entry behind)
    evql_table::NestedFlat e;
    e.nflat = nflat;
    if (c.rlevel_max >= lc.rlevel_max) {
      if (padded_rows(cap) < flatp) {
        // level streams shorter than the leaf's: not the same ancestor chain
        return Status::error(EVQL_ENOTSUP, "nested columns from different repeated groups");
      }
      e.d_values = std::move(d_vals);
    } else {
      size_t k = 0;
      while (thr_levels[k] != c.rlevel_max) ++k;
      DevBuf<uint64_t> d_flat;
      HIP_TRY(d_flat.alloc(flatp * 8));
      HIP_TRY(hipMemsetAsync(d_flat, 0, flatp * 8, s));
      HIP_TRY(launch_flatten_parent(leaf_levels, thr_offsets[k], c.rlevel_max, nflat, d_vals,
                                    d_flat, s));
      HIP_TRY(hipStreamSynchronize(s));
      e.d_values = std::move(d_flat);
    }
    if (kp.cols[i].string_hash) {
      // undefined slots carry strpos 0: the empty string (an all-zero SValue read as
      // a STRING, CSTableScan.cc:224-246)
      HIP_TRY(e.d_hash.alloc(flatp * 8));
      HIP_TRY(hipMemsetAsync(e.d_hash, 0, flatp * 8, s));
      HIP_TRY(launch_string_hash(t->d_image, t->d_pages[li][0], e.d_values, nflat, e.d_hash, s));
      HIP_TRY(hipStreamSynchronize(s));
    }
    publish(i, t->nested_cache.emplace(std::make_pair(li, leaf_li), std::move(e)).first->second);
  }
  if (keep && lc.rlevel_max > 0) {
    auto hit = t->leaf_cache.find(leaf_li);
    if (hit == t->leaf_cache.end()) {
      LeafLevels ll;
      ll.levels = std::move(d_leaf_levels);
      ll.rec_offsets = std::move(thr_offsets[0]);  // threshold 0 comes first
      hit = t->leaf_cache.emplace(leaf_li, std::move(ll)).first;
    }
    *keep = &hit->second;
  }
  return Status();
}

// Columns of SIBLING repeated groups (or of groups at different depths that share no
// chain): CSTableScan::fetchNext zips them level by level (CSTableScan.cc:187-541) -- a row
// per step of its column automaton; a group that has run out of slots reads the all-zero
// SValue from then on (:511-515), columns above the fetch level keep their value.  One
// thread replays that automaton per record (k_zip_rows), first counting the record's rows,
// then writing the slot every (column, row) reads; the flattened columns are gathered from
// the per-slot values.  Owned by the operator (not cached on the table).
Status materialize_nested_zip(evql_query* q, const std::vector<ColAccess>& cols,
                              std::vector<uint64_t*>* flat_out, uint64_t* nrows_out,
                              std::vector<uint64_t*>* strpos_out) {
  evql_table* t = q->table;
  hipStream_t s = q->ctx->stream;
  const uint64_t nrec = t->layout.num_rows;
  const size_t nc = cols.size();
  if (nc > kMaxZipCols) return Status::error(EVQL_ENOTSUP, "too many columns in a zipped nested scan");
  flat_out->assign(nc, nullptr);
  if (strpos_out) strpos_out->assign(nc, nullptr);
  q->nested_leaf = -1;
  if (nrec == 0) {
    *nrows_out = 0;
    return Status();
  }
  ZipArgs za{};
  za.nrec = nrec;
  za.ncols = uint32_t(nc);
  std::vector<DevBuf<uint64_t>> d_vals(nc), d_starts(nc), d_idx(nc);
  std::vector<DevBuf<uint8_t>> d_levels(nc);
  std::map<int, size_t> first_use;  // layout index -> first scan column that decoded it
  for (size_t i = 0; i < nc; ++i) {
    const int li = cols[i].layout_index;
    const ColumnLayout& c = t->layout.columns[li];
    za.rmax[i] = c.rlevel_max;
    auto seen = first_use.find(li);
    if (seen != first_use.end()) {
      const size_t j = seen->second;
      za.levels[i] = za.levels[j];
      za.starts[i] = za.starts[j];
      continue;
    }
    first_use[li] = i;
    uint64_t cap = 0;
    Status st = nested_slot_values(t, li, nrec, &d_vals[i], &cap);
    if (!st.ok()) return st;
    if (c.rlevel_max == 0) continue;  // one slot per record: levels / starts stay NULL
    uint32_t rbits = 0;
    st = stream_bits(t, c.rlevel_pages, &rbits);
    if (!st.ok()) return st;
    if (rbits == 0) return Status::error(EVQL_ENOTSUP, "repeated column without repetition levels");
    const uint64_t lcap = level_stream_capacity(c.rlevel_pages, rbits);
    const uint64_t lcapp = padded_rows(lcap);
    const uint64_t ntiles = (lcap + kDecodeTile - 1) / kDecodeTile;
    DevBuf<uint64_t> d_cnt;
    HIP_TRY(d_levels[i].alloc(lcapp));
    HIP_TRY(hipMemsetAsync(d_levels[i], 0xff, lcapp, s));
    HIP_TRY(d_cnt.alloc((ntiles + 2) * 8));
    const uint32_t thr0 = 0;
    st = decode_levels(t, li, 1, rbits, lcap, d_levels[i], 1, &thr0, &d_cnt);
    if (!st.ok()) return st;
    HIP_TRY(d_starts[i].alloc((nrec + 2) * 8));
    // (a level stream without zero padding: record `nrec` would start at its end)
    HIP_TRY(hipMemcpyAsync(d_starts[i].p + nrec, &lcap, 8, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_record_starts(d_levels[i], d_cnt, lcap, d_starts[i], nrec + 1, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (cap < lcap && c.dlevel_max > 0) {
      return Status::error(EVQL_EIO, "level streams of different length: " + c.name);
    }
    za.levels[i] = d_levels[i];
    za.starts[i] = d_starts[i];
  }
  DevBuf<uint64_t> d_rows;
  DevBuf<ZipArgs> d_args;
  HIP_TRY(d_rows.alloc((nrec + 2) * 8));
  HIP_TRY(d_args.alloc(sizeof(ZipArgs)));
  za.rows = d_rows;
  HIP_TRY(hipMemcpyAsync(d_args, &za, sizeof(ZipArgs), hipMemcpyHostToDevice, s));
  HIP_TRY(launch_zip_rows(d_args, nrec, 0, s));
  uint64_t nflat = 0;
  HIP_TRY(launch_exclusive_scan(d_rows, nrec, d_rows.p + nrec, s));
  HIP_TRY(hipMemcpyAsync(&nflat, d_rows.p + nrec, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *nrows_out = nflat;
  const uint64_t flatp = padded_rows(nflat);
  for (size_t i = 0; i < nc; ++i) {
    HIP_TRY(d_idx[i].alloc(std::max<uint64_t>(nflat, 1) * 8));
    za.idx[i] = d_idx[i];
  }
  HIP_TRY(hipMemcpyAsync(d_args, &za, sizeof(ZipArgs), hipMemcpyHostToDevice, s));
  HIP_TRY(launch_zip_rows(d_args, nrec, 1, s));
  for (size_t i = 0; i < nc; ++i) {
    const int li = cols[i].layout_index;
    const size_t src = first_use[li];
    DevBuf<uint64_t> d_flat;
    HIP_TRY(d_flat.alloc(flatp * 8));
    HIP_TRY(hipMemsetAsync(d_flat, 0, flatp * 8, s));
    HIP_TRY(launch_zip_gather(d_vals[src], d_idx[i], nflat, d_flat, s));
    if (cols[i].string_hash) {
      // the flattened words are (len << 40 | position); a reset slot reads strpos 0: ""
      DevBuf<uint64_t> d_hash;
      HIP_TRY(d_hash.alloc(flatp * 8));
      HIP_TRY(hipMemsetAsync(d_hash, 0, flatp * 8, s));
      HIP_TRY(launch_string_hash(t->d_image, t->d_pages[li][0], d_flat, nflat, d_hash, s));
      (*flat_out)[i] = d_hash;
      if (strpos_out) (*strpos_out)[i] = d_flat;
      q->nested_owned.push_back(d_hash.release());
      q->nested_owned.push_back(d_flat.release());
    } else {
      (*flat_out)[i] = d_flat;
      q->nested_owned.push_back(d_flat.release());
    }
  }
  HIP_TRY(hipStreamSynchronize(s));
  return Status();
}

// CSTableScan with AGGREGATE_WITHIN_RECORD_FLAT (CSTableScan.cc:440-487): one
// output row per record holding the scan select list's aggregates over the
// record's flattened rows.  select_list_[i] accumulates on the rows whose fetch
// level is <= its rep_level (:442); with every column on one ancestor chain the
// fetch level of a row is the leaf's repetition level of that slot.
Status materialize_within_record(evql_query* q) {
  evql_table* t = q->table;
  hipStream_t s = q->ctx->stream;
  const uint64_t nrec = t->layout.num_rows;
  if (q->wr_aggs.size() > kMaxWithinAggs) {
    return Status::error(EVQL_ENOTSUP, "too many WITHIN RECORD aggregates");
  }
  std::vector<uint64_t*> flat;
  uint64_t nflat = 0;
  const LeafLevels* leaf = nullptr;  // (stays null where the leaf is not repeated)
  Status st = materialize_nested(q, q->wr_cols, &flat, &nflat, &leaf);
  if (!st.ok()) return st;
  WithinRecordArgs a{};
  a.leaf_levels = leaf ? leaf->levels.p : nullptr;
  a.rec_offsets = leaf ? leaf->rec_offsets.p : nullptr;
  a.nflat = nflat;
  a.nrec = nrec;
  a.n = uint32_t(q->wr_aggs.size());
  const uint64_t recp = padded_rows(nrec);
  q->nested_flat.assign(q->wr_aggs.size(), nullptr);
  for (size_t e = 0; e < q->wr_aggs.size(); ++e) {
    const evql_query::WithinAgg& w = q->wr_aggs[e];
    DevBuf<uint64_t> d_out;
    HIP_TRY(d_out.alloc(recp * 8));
    // (every record is stored by the kernel: only the padding behind them is cleared)
    if (recp > nrec) HIP_TRY(hipMemsetAsync(d_out.p + nrec, 0, (recp - nrec) * 8, s));
    if (leaf) {
      const uint64_t ntiles = (nflat + kDecodeTile - 1) / kDecodeTile;
      DevBuf<uint64_t> d_head;
      HIP_TRY(d_head.alloc(std::max<uint64_t>(ntiles, 1) * 8));
      a.tile_head[e] = d_head;
      q->nested_owned.push_back(d_head.release());
    }
    a.src[e] = w.col >= 0 ? flat[w.col] : nullptr;
    a.lit[e] = w.lit;
    a.level[e] = w.level;
    a.is_count[e] = w.is_count ? 1 : 0;
    a.out[e] = d_out;
    q->nested_flat[e] = d_out;
    q->nested_owned.push_back(d_out.release());
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  HIP_TRY(hipEventRecord(e0, s));
  HIP_TRY(launch_within_record(a, s));
  HIP_TRY(hipEventRecord(e1, s));
  HIP_TRY(hipStreamSynchronize(s));
  float wms = 0;
  hipEventElapsedTime(&wms, e0, e1);
  q->within_record_ms = wms;
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  q->nested_rows = nrec;
  // (the reference counts the flattened rows it read, not the records it emitted)
  q->reported_rows_scanned = nflat;
  return Status();
}

// Row filter of a nested scan.  CSTableScan reads filter_[record] when a record starts and
// every flattened row of a rejected record fails where_pred (CSTableScan.cc:426, 642-645):
// a record mask.  The fused kernel tests one bit per row of ITS input:
//  * WITHIN RECORD, scans without columns, leaves that are not repeated: a row is a
//    record, the caller's bits are the row filter as they are;
//  * otherwise the record bits are expanded once, here, to one bit per leaf slot
//    (k_filter_expand); the expansion belongs to the query and replaces d_row_filter.
// The statistics follow the reference's counters: its nested loop counts every flattened
// row as scanned, its column-less loop only the records the filter keeps.
Status expand_record_filter(evql_query* q, const LeafLevels* leaf) {
  hipStream_t s = q->ctx->stream;
  const uint64_t nrec = q->table->layout.num_rows;
  if (q->kp.cols.empty() && !q->within_record) {
    std::vector<uint8_t> bits = q->row_filter_host;
    const uint64_t len = std::min<uint64_t>(q->row_filter_len, nrec);
    if (bits.empty()) {  // a chain's filter lives on the device
      bits.resize((len + 7) / 8);
      if (len) HIP_TRY(hipMemcpy(bits.data(), q->d_row_filter, bits.size(), hipMemcpyDeviceToHost));
    }
    uint64_t kept = 0;
    for (uint64_t r = 0; r < len; ++r) kept += (bits[r >> 3] >> (r & 7)) & 1;
    q->reported_rows_scanned = kept;
  }
  if (q->within_record || !leaf) return Status();
  const uint64_t nflat = q->nested_rows;
  const uint64_t ntiles = (nflat + kDecodeTile - 1) / kDecodeTile;
  DevBuf<uint64_t> d_rows;
  HIP_TRY(d_rows.alloc((ntiles * (kDecodeTile / 64) + 2) * 8));
  HIP_TRY(launch_filter_expand(leaf->levels, leaf->rec_offsets, nflat, q->d_row_filter,
                               std::min<uint64_t>(q->row_filter_len, nrec), d_rows, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (q->row_filter_owned) hipFree(q->d_row_filter);
  q->d_row_filter = reinterpret_cast<uint8_t*>(d_rows.release());
  q->row_filter_owned = true;
  q->row_filter_len = nflat;
  return Status();
}

// CSTableScan::fetchNext keeps the values of shallower columns across the rows of one
// slot, but after a row that WHERE rejects it resets every column at or below the
// running select level without re-reading it (CSTableScan.cc:501-512).  Worked out per
// column C of repetition depth c: the rows of a slot of C read C's value, except that
// they read 0 from the second row on when the slot's FIRST row was rejected (the first
// row itself always sees the freshly fetched value).  Whether a first row is rejected
// depends only on fresh values and on columns shallower than c, so the depths are
// settled one after the other, shallowest first: predicate of every row over the
// columns as they stand (evql_where_rows), verdict of every slot's first row
// (k_slot_keep), masked copy of the depth's columns (k_mask_parent).  Pinned by the
// reference's own engine on tests/golden/ref_csql_nested.json.
Status apply_where_resets(evql_query* q, const LeafLevels* leaf) {
  evql_table* t = q->table;
  hipStream_t s = q->ctx->stream;
  const KernelPlan& kp = q->kp;
  const uint64_t n = q->nested_rows;
  if (n == 0 || !leaf || !q->module.fn_where) return Status();
  uint32_t leaf_depth = 0;
  std::vector<uint32_t> depths;
  for (const auto& c : kp.cols) {
    leaf_depth = std::max(leaf_depth, t->layout.columns[c.layout_index].rlevel_max);
  }
  for (const auto& c : kp.cols) {
    const uint32_t d = t->layout.columns[c.layout_index].rlevel_max;
    if (d < leaf_depth && std::find(depths.begin(), depths.end(), d) == depths.end()) depths.push_back(d);
  }
  std::sort(depths.begin(), depths.end());
  const uint64_t np = padded_rows(n);
  const uint64_t ntiles = (n + kDecodeTile - 1) / kDecodeTile;
  DevBuf<uint8_t> d_acc, d_keep;
  DevBuf<uint64_t> d_off;
  HIP_TRY(d_acc.alloc(np));
  HIP_TRY(d_keep.alloc(np));
  HIP_TRY(d_off.alloc((ntiles + 2) * 8));
  HIP_TRY(hipMemsetAsync(d_acc, 0, np, s));
  struct WhereArgs {
    HostArgs a;
    uint8_t* acc;
  };
  for (uint32_t d : depths) {
    WhereArgs wa{};
    fill_host_args(q, &wa.a);
    wa.acc = d_acc;
    size_t sz = sizeof(WhereArgs);
    void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &wa, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz,
                      HIP_LAUNCH_PARAM_END};
    int grid = q->grid;
    if (uint64_t(grid) > wa.a.ntiles) grid = int(wa.a.ntiles);
    if (grid > 0) {
      HIP_TRY(hipModuleLaunchKernel(q->module.fn_where, grid, 1, 1, kp.block, 1, 1, 0, s, nullptr,
                                    config));
    }
    HIP_TRY(launch_level_tile_counts(leaf->levels, d, n, d_off, s));
    HIP_TRY(launch_exclusive_scan(d_off, ntiles, nullptr, s));
    HIP_TRY(hipMemsetAsync(d_keep, 0, np, s));
    HIP_TRY(launch_slot_keep(leaf->levels, d_off, d, n, d_acc, d_keep, s));
    std::map<uint64_t*, uint64_t*> done;  // (a column referenced twice shares one buffer)
    for (size_t i = 0; i < kp.cols.size(); ++i) {
      if (t->layout.columns[kp.cols[i].layout_index].rlevel_max != d) continue;
      auto hit = done.find(q->nested_flat[i]);
      if (hit != done.end()) {
        q->nested_flat[i] = hit->second;
        continue;
      }
      DevBuf<uint64_t> d_out;
      HIP_TRY(d_out.alloc(np * 8));
      HIP_TRY(hipMemsetAsync(d_out, 0, np * 8, s));
      if (kp.cols[i].string_hash) {
        // a reset string reads "" (an all-zero SValue): mask the positions, hash again
        DevBuf<uint64_t> d_sp;
        HIP_TRY(d_sp.alloc(np * 8));
        HIP_TRY(hipMemsetAsync(d_sp, 0, np * 8, s));
        HIP_TRY(launch_mask_parent(leaf->levels, d_off, d, n, d_keep, q->nested_strpos[i], d_sp, s));
        HIP_TRY(launch_string_hash(t->d_image, t->d_pages[kp.cols[i].layout_index][0], d_sp, n,
                                   d_out, s));
        q->nested_strpos[i] = d_sp;
        q->nested_owned.push_back(d_sp.release());
      } else {
        HIP_TRY(launch_mask_parent(leaf->levels, d_off, d, n, d_keep, q->nested_flat[i], d_out, s));
      }
      done[q->nested_flat[i]] = d_out;
      q->nested_flat[i] = d_out;
      q->nested_owned.push_back(d_out.release());
    }
    HIP_TRY(hipStreamSynchronize(s));
  }
  return Status();
}

}  // namespace evql
