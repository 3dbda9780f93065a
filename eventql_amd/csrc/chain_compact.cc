// chain_compact.cc -- a partition's file chain compacted into one cstable on the device
// (evql_lsm_chain_compact).
//
// SimpleCompactionStrategy::compact (db/compaction_strategy.cc:44-222) reads every input
// table column by column on one CPU thread and appends the rows it keeps to a CSTableWriter.
// Here the inputs are resident tables, the rows to keep are the chain's filter bits in HBM
// (lsm.cc) and the writer is table_from_device_columns (device_writer.cc); what joins them
// is a streaming gather of the kept rows into SoA columns:
//
//   1. resolve   which column of which table feeds an output column (chain_compact_plan.cc),
//                and a row- / slot-addressable device form of each (the tables' caches)
//   2. rank      kept rows per 2048-row tile of every table (k_cmp_ranks), kept slots per
//                tile of every repeated column (k_cmp_slot_counts); ONE scan per array over
//                the tiles of all tables in output order = the destination of every tile
//   3. fixed     value word + NULL byte of the kept rows (k_cmp_fixed, one launch per table)
//   4. strings   sizes of the gathered (len << 40 | position) words per output tile, one scan
//                per column across all tables, bytes into one heap per column
//                (k_cmp_str_sizes / k_cmp_str_bytes)
//   5. repeated  (r, d, value) of the slots of kept records (k_cmp_slots)
//   6. encode    table_from_device_columns, as it is
//   7. stats
//
// evql_lsm_chain_compact_sorted is the same call with three more steps; by 5b every flat
// column is vals (+ nulls) over rows_out dense rows and a string's word is (len << 40) | heap
// offset, so reordering the words reorders the strings without touching the heap:
//
//   3b. key statistics  min, max and descents of the gathered key words (k_sort_key_stats);
//                       read back with step 4's wait, or with one of its own when no STRING
//                       column is written
//   5b. sort            no descent: nothing more.  Otherwise (key, u32 row) pairs through
//                       ceil(bit_length(max - min) / 8) stable 8-bit passes over key - min
//                       (k_sort_hist, k_sort_digit_scan, k_sort_scatter), ping-pong
//   5c. permute         dst[i] = src[perm[i]] for the words and NULL bytes of the other
//                       columns, in groups that share one read of perm (k_cmp_permute); the
//                       key column takes the last pass's sorted words
//
// Output positions are fixed by the scans: no atomic decides where a row lands and no
// workgroup waits for another.  Host waits of steps 2 - 5: one for the sizes that the host
// must know (the flat total as a check against the chain's own counts, the slot totals of
// repeated columns) and, when there is a string column, one for the heap sizes.
#include "chain_compact_plan.h"
#include "radix_sort.h"
#include "runtime.h"

namespace evql {
namespace {

// the part of an output column that one table fills
struct Segment {
  size_t table = 0;  // chain index
  int li = -1;       // layout index in that table, -1: absent
  uint64_t base = 0, len = 0;
};

struct OutColumn {
  DevBuf<uint64_t> vals;
  DevBuf<uint8_t> nulls, rlevels, dlevels, heap;
  uint64_t n = 0;              // value words: output rows, or slots of a repeated column
  std::vector<Segment> segs;   // in output order
  // repeated columns: the source slots per table (chain order), kept slots per tile
  std::vector<ColumnSlots> slots;
  std::vector<uint64_t> slot_tile_base;  // per table (chain order)
  uint64_t slot_tiles = 0;
  DevBuf<uint64_t> d_slot_tiles;
  // strings: bytes per output tile, scanned
  std::vector<uint64_t> str_tile_base;  // per segment
  uint64_t str_tiles = 0, heap_bytes = 0;
  DevBuf<uint64_t> d_str_tiles;
};

// columns that one k_cmp_permute launch moves: its destinations are staging beyond the table
static const size_t kPermuteGroup = 4;

// steps 3b, 5b, 5c of the sorted form
struct SortJob {
  size_t key = 0;                 // output column
  bool own_wait = false;          // no STRING column: the statistics need a wait of their own
  DevBuf<uint64_t> d_stats;       // [0..2] k_sort_key_stats, [3] k_cmp_permute's status
  uint64_t* h_stats = nullptr;    // their four words of the pinned block
  RadixPassScratch pass;          // the pairs, ping-pong
  std::vector<DevBuf<uint64_t>> free_vals;  // retired value / NULL buffers: the next
  std::vector<DevBuf<uint8_t>> free_nulls;  // group's destinations
  std::vector<CmpPermuteCol> h_cols;        // (lives until the stream has been synchronised)
  DevBuf<CmpPermuteCol> d_cols;
  evql_compact_sort_stats_t st{};
};

struct Job {
  evql_ctx* ctx = nullptr;
  hipStream_t s = nullptr;
  std::vector<evql_table*> tables;          // chain order
  std::vector<const uint8_t*> d_filters;    // NULL: every row is kept
  std::vector<uint64_t> kept;
  std::vector<size_t> order;                // output position -> chain index
  const std::vector<ColumnSpec>* specs = nullptr;
  CompactPlan plan;
  std::vector<OutColumn> cols;
  std::vector<std::vector<RtColumn>> flat;  // [column][table] row-addressable sources
  DevBuf<uint64_t> d_row_tiles;             // scanned kept rows per tile, all tables
  uint64_t* h_pinned = nullptr;             // the sizes the host reads back
  uint32_t launches = 0, waits = 0;
  SortJob* sort = nullptr;                  // the sorted form
  const uint64_t* bits(size_t k) const { return reinterpret_cast<const uint64_t*>(d_filters[k]); }
};

uint64_t tiles_of(uint64_t n) { return (n + kCompactTile - 1) / kCompactTile; }

// values a fixed-width data stream holds: direct page reads stay below it
bool pages_hold_rows(const ColumnLayout& c, uint32_t mode, uint32_t bits, uint64_t n) {
  const uint64_t np = c.data_pages.size();
  switch (mode) {
    case ColAccess::PLAIN64: return n <= np * (kPlainPageSize / 8);
    case ColAccess::PLAIN32: return n <= np * (kPlainPageSize / 4);
    case ColAccess::BITPACKED: return bits == 0 || n <= np * kBitpackBlocksPerPage * 128;
    default: return true;
  }
}

// ---- 1. resolve ------------------------------------------------------------------------
Status resolve_columns(Job& j) {
  const std::vector<ColumnSpec>& specs = *j.specs;
  const size_t nt = j.tables.size();
  std::vector<const TableLayout*> layouts;
  for (evql_table* t : j.tables) layouts.push_back(&t->layout);
  const std::string err = plan_chain_compact(layouts, j.kept, specs, j.order[0] != 0, &j.plan);
  if (!err.empty()) return Status::error(EVQL_EARG, err);
  j.cols.resize(specs.size());
  j.flat.assign(specs.size(), std::vector<RtColumn>(nt));
  for (size_t c = 0; c < specs.size(); ++c) {
    const CompactColumn& pc = j.plan.columns[c];
    OutColumn& oc = j.cols[c];
    if (pc.nested) oc.slots.resize(nt);
    for (size_t k = 0; k < nt; ++k) {
      const int li = pc.source[k];
      if (li < 0) continue;
      evql_table* t = j.tables[k];
      if (pc.nested) {
        Status st = nested_column_slots(t, li, &oc.slots[k]);
        if (!st.ok()) return st;
        continue;
      }
      RtColumn rc{};
      const uint64_t* strpos = nullptr;
      Status st = table_rt_column(t, specs[c].name, &rc, &strpos);
      if (!st.ok()) return st;
      if (pc.is_string) {
        // a string's value word is where its bytes are: (len << 40) | stream position
        if (!strpos) return Status::error(EVQL_EARG, "not a string column: " + specs[c].name);
        const uint8_t* tags = rc.tags;
        rc = RtColumn{};
        rc.mode = ColAccess::SOA;
        rc.soa = strpos;
        rc.tags = tags;
      }
      if (!pages_hold_rows(t->layout.columns[li], rc.mode, rc.bits, t->layout.num_rows)) {
        return Status::error(EVQL_EIO, "end of column reached: " + specs[c].name);
      }
      j.flat[c][k] = rc;
    }
  }
  return Status();
}

// ---- 2. rank ---------------------------------------------------------------------------
Status rank_kept(Job& j) {
  const size_t nt = j.tables.size();
  HIP_TRY(j.d_row_tiles.alloc((j.plan.tiles + 2) * 8));
  for (size_t k : j.order) {
    const uint64_t n = j.tables[k]->layout.num_rows;
    if (!n) continue;
    HIP_TRY(launch_cmp_ranks(j.bits(k), n, j.d_row_tiles.p + j.plan.tile_base[k], j.s));
    ++j.launches;
  }
  HIP_TRY(launch_exclusive_scan(j.d_row_tiles, j.plan.tiles, j.d_row_tiles.p + j.plan.tiles, j.s));
  ++j.launches;
  // what the host reads back: [0] kept rows; per repeated column its segment bases and total
  size_t nread = 1;
  HIP_TRY(hipMemcpyAsync(j.h_pinned, j.d_row_tiles.p + j.plan.tiles, 8, hipMemcpyDeviceToHost, j.s));
  for (size_t c = 0; c < j.cols.size(); ++c) {
    if (!j.plan.columns[c].nested) continue;
    OutColumn& oc = j.cols[c];
    oc.slot_tile_base.assign(nt, 0);
    for (size_t k : j.order) {
      oc.slot_tile_base[k] = oc.slot_tiles;
      // an absent column has one (0, 0) slot per record
      const uint64_t ns = j.plan.columns[c].source[k] < 0 ? j.tables[k]->layout.num_rows
                                                          : oc.slots[k].nslots;
      oc.slot_tiles += tiles_of(ns);
    }
    HIP_TRY(oc.d_slot_tiles.alloc((oc.slot_tiles + 2) * 8));
    for (size_t k : j.order) {
      CmpSlotArgs a{};
      const ColumnSlots& cs = oc.slots[k];
      const bool present = j.plan.columns[c].source[k] >= 0;
      a.rlevels = present ? cs.rlevels : nullptr;
      a.rec_offsets = present ? cs.rec_offsets : nullptr;
      a.bits = j.bits(k);
      a.nrec = j.tables[k]->layout.num_rows;
      a.nslots = present ? cs.nslots : a.nrec;
      a.tile_counts = oc.d_slot_tiles.p + oc.slot_tile_base[k];
      if (!a.nslots) continue;
      HIP_TRY(launch_cmp_slot_counts(a, j.s));
      ++j.launches;
    }
    HIP_TRY(launch_exclusive_scan(oc.d_slot_tiles, oc.slot_tiles, oc.d_slot_tiles.p + oc.slot_tiles, j.s));
    ++j.launches;
    if ((nread + nt + 1) * 8 > kTailBlockBytes) {
      return Status::error(EVQL_ENOTSUP, "too many repeated columns x tables in one compaction");
    }
    for (size_t p = 0; p < nt; ++p) {
      HIP_TRY(hipMemcpyAsync(j.h_pinned + nread + p, oc.d_slot_tiles.p + oc.slot_tile_base[j.order[p]], 8,
                             hipMemcpyDeviceToHost, j.s));
    }
    HIP_TRY(hipMemcpyAsync(j.h_pinned + nread + nt, oc.d_slot_tiles.p + oc.slot_tiles, 8,
                           hipMemcpyDeviceToHost, j.s));
    nread += nt + 1;
  }
  HIP_TRY(hipStreamSynchronize(j.s));
  ++j.waits;
  if (j.h_pinned[0] != j.plan.rows_out) {
    return Status::error(EVQL_ERUNTIME, "the chain's filters keep other rows than its build counted");
  }
  // the segments of every column
  nread = 1;
  for (size_t c = 0; c < j.cols.size(); ++c) {
    OutColumn& oc = j.cols[c];
    const CompactColumn& pc = j.plan.columns[c];
    for (size_t p = 0; p < nt; ++p) {
      Segment sg;
      sg.table = j.order[p];
      sg.li = pc.source[sg.table];
      if (pc.nested) {
        sg.base = j.h_pinned[nread + p];
        sg.len = j.h_pinned[nread + p + 1] - sg.base;
      } else {
        sg.base = j.plan.row_base[sg.table];
        sg.len = j.kept[sg.table];
      }
      oc.segs.push_back(sg);
    }
    oc.n = pc.nested ? j.h_pinned[nread + nt] : j.plan.rows_out;
    if (pc.nested) nread += nt + 1;
  }
  return Status();
}

// ---- 3. fixed-width columns (and the value words of flat strings) -------------------------
Status gather_fixed(Job& j, DevBuf<CmpFixedCol>* d_cols, std::vector<CmpFixedCol>* h_cols) {
  const std::vector<ColumnSpec>& specs = *j.specs;
  const size_t nt = j.tables.size();
  size_t nflat = 0;
  for (size_t c = 0; c < specs.size(); ++c) {
    if (j.plan.columns[c].nested) continue;
    ++nflat;
    OutColumn& oc = j.cols[c];
    HIP_TRY(oc.vals.alloc(oc.n * 8));
    if (specs[c].dlevel_max > 0) HIP_TRY(oc.nulls.alloc(oc.n));
    if (j.plan.columns[c].constant_false) {
      HIP_TRY(hipMemsetAsync(oc.vals, 0, oc.n * 8, j.s));
      if (oc.nulls.p) HIP_TRY(hipMemsetAsync(oc.nulls, 0, oc.n, j.s));
      continue;
    }
    for (const Segment& sg : oc.segs) {
      if (sg.li >= 0 || !sg.len) continue;
      // absent from this table: one NULL per kept row (writeNull, compaction_strategy.cc:171-173)
      HIP_TRY(hipMemsetAsync(oc.vals.p + sg.base, 0, sg.len * 8, j.s));
      HIP_TRY(hipMemsetAsync(oc.nulls.p + sg.base, 1, sg.len, j.s));
    }
  }
  // one launch per table over the columns it holds
  h_cols->assign(nt * nflat, CmpFixedCol{});
  HIP_TRY(d_cols->alloc(h_cols->size() * sizeof(CmpFixedCol)));
  std::vector<uint32_t> ncols(nt, 0);
  for (size_t k = 0; k < nt; ++k) {
    for (size_t c = 0; c < specs.size(); ++c) {
      const CompactColumn& pc = j.plan.columns[c];
      if (pc.nested || pc.constant_false || pc.source[k] < 0) continue;
      CmpFixedCol& fc = (*h_cols)[k * nflat + ncols[k]++];
      fc.src = j.flat[c][k];
      fc.out_vals = j.cols[c].vals;
      fc.out_nulls = j.cols[c].nulls;
    }
  }
  if (!h_cols->empty()) {
    HIP_TRY(hipMemcpyAsync(d_cols->p, h_cols->data(), h_cols->size() * sizeof(CmpFixedCol),
                           hipMemcpyHostToDevice, j.s));
  }
  for (size_t k : j.order) {
    if (!ncols[k] || !j.kept[k]) continue;
    CmpFixedArgs a{};
    a.image = j.tables[k]->d_image;
    a.cols = d_cols->p + k * nflat;
    a.ncols = ncols[k];
    a.bits = j.bits(k);
    a.nrows = j.tables[k]->layout.num_rows;
    a.tile_off = j.d_row_tiles.p + j.plan.tile_base[k];
    a.out_cap = j.plan.rows_out;
    HIP_TRY(launch_cmp_fixed(a, j.s));
    ++j.launches;
  }
  return Status();
}

// ---- 5. repeated / nested columns ---------------------------------------------------------
Status gather_slots(Job& j) {
  const std::vector<ColumnSpec>& specs = *j.specs;
  for (size_t c = 0; c < specs.size(); ++c) {
    const CompactColumn& pc = j.plan.columns[c];
    if (!pc.nested) continue;
    OutColumn& oc = j.cols[c];
    HIP_TRY(oc.vals.alloc(oc.n * 8));
    HIP_TRY(oc.dlevels.alloc(oc.n));
    if (specs[c].rlevel_max > 0) HIP_TRY(oc.rlevels.alloc(oc.n));
    for (const Segment& sg : oc.segs) {
      if (!sg.len) continue;
      const size_t k = sg.table;
      const ColumnSlots& cs = oc.slots[k];
      CmpSlotArgs a{};
      a.bits = j.bits(k);
      a.nrec = j.tables[k]->layout.num_rows;
      if (sg.li >= 0) {
        a.rlevels = cs.rlevels;
        a.rec_offsets = cs.rec_offsets;
        a.dlevels = cs.dlevels;
        a.values = cs.values;
        a.nslots = cs.nslots;
      } else {
        a.nslots = a.nrec;  // one slot (r = 0, d = 0) per kept record
      }
      a.tile_off = oc.d_slot_tiles.p + oc.slot_tile_base[k];
      a.out_r = oc.rlevels;
      a.out_d = oc.dlevels;
      a.out_vals = oc.vals;
      a.out_cap = oc.n;
      HIP_TRY(launch_cmp_slots(a, j.s));
      ++j.launches;
    }
  }
  return Status();
}

// ---- 4. strings ---------------------------------------------------------------------------
// The gathered value words of a string column name bytes of the table they came from.  Per
// column: bytes per 2048-word tile of every segment, one scan across the segments, then the
// bytes into one heap; the words become (len << 40) | heap offset.
Status gather_strings(Job& j, uint64_t* string_bytes) {
  const std::vector<ColumnSpec>& specs = *j.specs;
  std::vector<size_t> str_cols;
  for (size_t c = 0; c < specs.size(); ++c) {
    if (j.plan.columns[c].is_string) str_cols.push_back(c);
  }
  *string_bytes = 0;
  if (str_cols.empty()) return Status();
  if ((str_cols.size() + 4) * 8 > kTailBlockBytes) return Status::error(EVQL_ENOTSUP, "too many string columns");
  auto str_args = [&](const OutColumn& oc, size_t si) {
    const Segment& sg = oc.segs[si];
    evql_table* t = j.tables[sg.table];
    CmpStrArgs a{};
    a.image = t->d_image;
    a.pages = t->d_pages[sg.li][0];
    a.src_bytes = uint64_t(t->layout.columns[sg.li].data_pages.size()) * kPlainPageSize;
    a.words = oc.vals.p + sg.base;
    a.n = sg.len;
    return a;
  };
  for (size_t x = 0; x < str_cols.size(); ++x) {
    OutColumn& oc = j.cols[str_cols[x]];
    for (const Segment& sg : oc.segs) {
      oc.str_tile_base.push_back(oc.str_tiles);
      oc.str_tiles += tiles_of(sg.len);
    }
    HIP_TRY(oc.d_str_tiles.alloc((oc.str_tiles + 2) * 8));
    // (the words of a segment whose table lacks the column are zero: no bytes)
    HIP_TRY(hipMemsetAsync(oc.d_str_tiles, 0, (oc.str_tiles + 2) * 8, j.s));
    for (size_t si = 0; si < oc.segs.size(); ++si) {
      if (oc.segs[si].li < 0 || !oc.segs[si].len) continue;
      CmpStrArgs a = str_args(oc, si);
      a.tile_sums = oc.d_str_tiles.p + oc.str_tile_base[si];
      HIP_TRY(launch_cmp_str_sizes(a, j.s));
      ++j.launches;
    }
    HIP_TRY(launch_exclusive_scan(oc.d_str_tiles, oc.str_tiles, oc.d_str_tiles.p + oc.str_tiles, j.s));
    ++j.launches;
    HIP_TRY(hipMemcpyAsync(j.h_pinned + x, oc.d_str_tiles.p + oc.str_tiles, 8, hipMemcpyDeviceToHost, j.s));
  }
  HIP_TRY(hipStreamSynchronize(j.s));
  ++j.waits;
  for (size_t x = 0; x < str_cols.size(); ++x) {
    OutColumn& oc = j.cols[str_cols[x]];
    oc.heap_bytes = j.h_pinned[x];
    *string_bytes += oc.heap_bytes;
    HIP_TRY(oc.heap.alloc(oc.heap_bytes));
    for (size_t si = 0; si < oc.segs.size(); ++si) {
      if (oc.segs[si].li < 0 || !oc.segs[si].len) continue;
      CmpStrArgs a = str_args(oc, si);
      a.tile_off = oc.d_str_tiles.p + oc.str_tile_base[si];
      a.heap = oc.heap;
      a.heap_cap = oc.heap_bytes;
      HIP_TRY(launch_cmp_str_bytes(a, j.s));
      ++j.launches;
    }
  }
  return Status();
}

// ---- 3b. key statistics ---------------------------------------------------------------------
Status sort_key_stats(Job& j, hipEvent_t begin, hipEvent_t end) {
  SortJob& sj = *j.sort;
  const uint64_t n = j.plan.rows_out;
  sj.own_wait = true;
  for (const CompactColumn& pc : j.plan.columns) sj.own_wait = sj.own_wait && !pc.is_string;
  sj.h_stats = j.h_pinned + kTailBlockBytes / 8 - 4;  // (the sizes of steps 2 and 4 lie in front)
  HIP_TRY(sj.d_stats.alloc(4 * 8));
  HIP_TRY(hipMemsetAsync(sj.d_stats, 0, 4 * 8, j.s));
  HIP_TRY(hipEventRecord(begin, j.s));
  if (n) {
    HIP_TRY(launch_sort_key_stats(j.cols[sj.key].vals, n, sj.d_stats, j.s));
    ++sj.st.n_kernel_launches;
  }
  HIP_TRY(hipEventRecord(end, j.s));
  HIP_TRY(hipMemcpyAsync(sj.h_stats, sj.d_stats.p, 3 * 8, hipMemcpyDeviceToHost, j.s));
  if (sj.own_wait) {
    HIP_TRY(hipStreamSynchronize(j.s));
    ++sj.st.n_host_waits;
  }
  return Status();
}

// ---- 5b. sort -------------------------------------------------------------------------------
Status sort_rows(Job& j) {
  SortJob& sj = *j.sort;
  const uint64_t n = j.plan.rows_out;
  sj.st.rows = n;
  sj.st.key_min = n ? ~sj.h_stats[0] : 0;
  sj.st.key_max = n ? sj.h_stats[1] : 0;
  sj.st.presorted = sj.h_stats[2] == 0 || n <= 1;
  if (sj.st.presorted) return Status();
  uint32_t bits = 0;
  for (uint64_t range = sj.st.key_max - sj.st.key_min; range; range >>= 1) ++bits;
  sj.st.passes = (bits + 7) / 8;
  // the first pass reads the gathered column; its rows are the identity
  Status st = radix_sort_passes(j.cols[sj.key].vals, nullptr, n, sj.st.key_min, sj.st.passes, &sj.pass, j.s);
  if (!st.ok()) return st;
  sj.st.n_kernel_launches += 3 * sj.st.passes;
  return Status();
}

// ---- 5c. permute ----------------------------------------------------------------------------
Status permute_columns(Job& j) {
  SortJob& sj = *j.sort;
  const std::vector<ColumnSpec>& specs = *j.specs;
  const uint64_t n = j.plan.rows_out;
  const uint32_t last = (sj.st.passes - 1) & 1;
  // the key column's sorted words are the last pass's; its gathered words and the other pair
  // buffer are the first destinations
  OutColumn& kc = j.cols[sj.key];
  sj.free_vals.push_back(std::move(kc.vals));
  kc.vals = std::move(sj.pass.keys[last]);
  if (sj.pass.keys[last ^ 1].p) sj.free_vals.push_back(std::move(sj.pass.keys[last ^ 1]));
  std::vector<size_t> todo;
  for (size_t c = 0; c < specs.size(); ++c) {
    // (a constant column is the same in every order)
    if (c != sj.key && !j.plan.columns[c].constant_false) todo.push_back(c);
  }
  if (todo.empty()) return Status();
  sj.h_cols.resize(todo.size());
  HIP_TRY(sj.d_cols.alloc(todo.size() * sizeof(CmpPermuteCol)));
  std::vector<DevBuf<uint64_t>> dst_vals(todo.size());
  std::vector<DevBuf<uint8_t>> dst_nulls(todo.size());
  for (size_t g = 0; g < todo.size(); g += kPermuteGroup) {
    const size_t ge = std::min(todo.size(), g + kPermuteGroup);
    for (size_t x = g; x < ge; ++x) {
      OutColumn& oc = j.cols[todo[x]];
      if (!sj.free_vals.empty()) {
        dst_vals[x] = std::move(sj.free_vals.back());
        sj.free_vals.pop_back();
      } else {
        HIP_TRY(dst_vals[x].alloc(n * 8));
      }
      if (oc.nulls.p) {
        if (!sj.free_nulls.empty()) {
          dst_nulls[x] = std::move(sj.free_nulls.back());
          sj.free_nulls.pop_back();
        } else {
          HIP_TRY(dst_nulls[x].alloc(n));
        }
      }
      sj.h_cols[x] = CmpPermuteCol{oc.vals.p, dst_vals[x].p, oc.nulls.p, dst_nulls[x].p};
    }
    HIP_TRY(hipMemcpyAsync(sj.d_cols.p + g, sj.h_cols.data() + g, (ge - g) * sizeof(CmpPermuteCol),
                           hipMemcpyHostToDevice, j.s));
    CmpPermuteArgs a{};
    a.perm = sj.pass.idx[last];
    a.n = n;
    a.cols = sj.d_cols.p + g;
    a.ncols = uint32_t(ge - g);
    a.status = sj.d_stats.p + 3;
    HIP_TRY(launch_cmp_permute(a, j.s));
    ++sj.st.n_kernel_launches;
    // the sources retire: the stream runs the next group behind this one
    for (size_t x = g; x < ge; ++x) {
      OutColumn& oc = j.cols[todo[x]];
      sj.free_vals.push_back(std::move(oc.vals));
      oc.vals = std::move(dst_vals[x]);
      if (oc.nulls.p) {
        sj.free_nulls.push_back(std::move(oc.nulls));
        oc.nulls = std::move(dst_nulls[x]);
      }
    }
  }
  HIP_TRY(hipMemcpyAsync(sj.h_stats + 3, sj.d_stats.p + 3, 8, hipMemcpyDeviceToHost, j.s));
  return Status();
}

}  // namespace

Status chain_compact(evql_lsm_chain* ch, const std::vector<ColumnSpec>& specs, int row_order,
                     int page_order, evql_table** out, evql_compact_stats_t* stats,
                     const CompactSort* sort) {
  Job j;
  SortJob sj;
  j.ctx = lsm_chain_ctx(ch);
  j.s = j.ctx->stream;
  j.specs = &specs;
  if (lsm_chain_parts(ch, &j.tables, &j.d_filters) == 0) return Status::error(EVQL_EARG, "chain was not built");
  lsm_chain_rows_kept(ch, &j.kept);
  const size_t nt = j.tables.size();
  for (size_t p = 0; p < nt; ++p) j.order.push_back(row_order == EVQL_COMPACT_FILE_ORDER ? nt - 1 - p : p);

  if (sort) {
    bool notsup = false;
    const std::string err = plan_compact_sort_key(specs, sort->key_column, &sj.key, &notsup);
    if (!err.empty()) return Status::error(notsup ? EVQL_ENOTSUP : EVQL_EARG, err);
    j.sort = &sj;
  }
  Status st = resolve_columns(j);
  if (!st.ok()) return st;
  if (sort) {
    bool notsup = false;
    const std::string err = plan_compact_sort_rows(j.plan.rows_out, &notsup);
    if (!err.empty()) return Status::error(EVQL_ENOTSUP, err);
  }

  // the pinned block of the read-backs goes back to the pool on every path
  struct PinnedBlock {
    std::shared_ptr<PinnedPool> pool;
    void* p = nullptr;
    ~PinnedBlock() {
      if (p) pool->give(p);
    }
  } pinned;
  pinned.pool = j.ctx->pinned;
  HIP_TRY(pinned.pool->take(&pinned.p));
  j.h_pinned = static_cast<uint64_t*>(pinned.p);
  struct Events {
    // [0..2] gather, encode; the sorted form: [3..4] key statistics, [5] passes, [6] permutes
    hipEvent_t e[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ~Events() {
      for (hipEvent_t x : e) {
        if (x) hipEventDestroy(x);
      }
    }
  } ev;
  for (int i = 0; i < (sort ? 7 : 3); ++i) HIP_TRY(hipEventCreate(&ev.e[i]));

  HIP_TRY(hipEventRecord(ev.e[0], j.s));
  st = rank_kept(j);
  if (!st.ok()) return st;
  DevBuf<CmpFixedCol> d_fixed_cols;
  std::vector<CmpFixedCol> h_fixed_cols;  // (lives until the stream has been synchronised)
  st = gather_fixed(j, &d_fixed_cols, &h_fixed_cols);
  if (st.ok() && sort) st = sort_key_stats(j, ev.e[3], ev.e[4]);
  if (st.ok()) st = gather_slots(j);
  uint64_t string_bytes = 0;
  if (st.ok()) st = gather_strings(j, &string_bytes);
  if (!st.ok()) return st;
  HIP_TRY(hipEventRecord(ev.e[1], j.s));
  hipEvent_t encode_begin = ev.e[1];
  // ---- 5b. sort, 5c. permute (the sorted form only) -------------------------------------------
  if (sort) {
    st = sort_rows(j);
    if (!st.ok()) return st;
    if (!sj.st.presorted) {
      HIP_TRY(hipEventRecord(ev.e[5], j.s));
      st = permute_columns(j);
      if (!st.ok()) return st;
      HIP_TRY(hipEventRecord(ev.e[6], j.s));
      encode_begin = ev.e[6];
    }
  }

  // ---- 6. encode ----------------------------------------------------------------------------
  std::vector<DeviceColumnIn> in;
  for (size_t c = 0; c < specs.size(); ++c) {
    const OutColumn& oc = j.cols[c];
    const bool nested = j.plan.columns[c].nested;
    in.push_back({oc.vals, oc.nulls, oc.heap, oc.rlevels, oc.dlevels, nested ? oc.n : 0});
  }
  evql_table* t = nullptr;
  st = table_from_device_columns(j.ctx, specs, in, j.plan.rows_out, page_order, &t);
  if (!st.ok()) return st;
  std::unique_ptr<evql_table> owned(t);
  HIP_TRY(hipEventRecord(ev.e[2], j.s));
  HIP_TRY(hipEventSynchronize(ev.e[2]));
  if (sort && !sj.st.presorted && sj.h_stats[3] != 0) {
    return Status::error(EVQL_ERUNTIME, "the sort's permutation names a row behind the last");
  }

  // ---- 7. stats -----------------------------------------------------------------------------
  if (stats) {
    *stats = evql_compact_stats_t{};
    stats->rows_in = j.plan.rows_in;
    stats->rows_written = j.plan.rows_out;
    stats->string_bytes = string_bytes;
    stats->n_tables = uint32_t(nt);
    stats->n_kernel_launches = j.launches;
    stats->n_host_waits = j.waits;
    HIP_TRY(hipEventElapsedTime(&stats->gather_ms, ev.e[0], ev.e[1]));
    HIP_TRY(hipEventElapsedTime(&stats->encode_ms, encode_begin, ev.e[2]));
  }
  if (sort) {
    // the key statistics ran inside the gather's span: their time is the sort's
    float key_stats_ms = 0, passes_ms = 0;
    HIP_TRY(hipEventElapsedTime(&key_stats_ms, ev.e[3], ev.e[4]));
    if (stats) stats->gather_ms = std::max(0.0f, stats->gather_ms - key_stats_ms);
    if (!sj.st.presorted) {
      HIP_TRY(hipEventElapsedTime(&passes_ms, ev.e[1], ev.e[5]));
      HIP_TRY(hipEventElapsedTime(&sj.st.permute_ms, ev.e[5], ev.e[6]));
    }
    sj.st.sort_ms = key_stats_ms + passes_ms;
    if (sort->stats) *sort->stats = sj.st;
  }
  *out = owned.release();
  return Status();
}

}  // namespace evql
