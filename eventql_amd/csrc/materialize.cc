// materialize.cc -- evql_table_from_query: the groups of an executed GROUP BY as a resident
// cstable, without leaving the device.
//
//   1. plan        plan_materialize (materialize_plan.cc): one MatCell per output column
//   2. records     collect_records (results.cc): the dense records [kind, slot words...]
//   3. gather      k_mat_first_rows + k_gather_rows (first-row cells), k_mat_fixed (value words,
//                  NULL bytes), per string column k_mat_str_sizes, a scan, k_mat_str_bytes
//   4. sort        with a sort column: key statistics, the LSD radix passes of sorted
//                  compaction over key - key_min, one k_cmp_permute over every other column
//                  (strings move their words only: the heap stays where it is)
//   5. encode      table_from_device_columns (device_writer.cc)
//
// Host waits: one for the heap sizes and the key statistics together (only with a STRING or a
// sort column), and the writer's.  The query is read, never changed.
#include <memory>
#include "radix_sort.h"
#include "runtime.h"

namespace evql {

MatInput materialize_input(const evql_query* q, const std::vector<MatSpec>* specs, int sort_column) {
  MatInput in;
  in.group_mode = q->group_mode;
  in.n = q->stats.num_groups;
  in.merged = q->merged;
  in.nested = q->nested;
  in.ordered = !q->order.empty() || q->has_limit;
  in.kp = &q->rplan();
  in.scan_select = &q->scan_select;
  in.select = &q->select;
  in.select_agg_index = &q->select_agg_index;
  in.select_passthrough = &q->select_passthrough;
  in.specs = specs;
  in.sort_column = sort_column;
  return in;
}

namespace {

struct Events {
  // [0] begin, [1] fixed cells and string sizes done, [2] key statistics done, [3] string bytes
  // done, [4] sorted and permuted, [5] encoded
  hipEvent_t e[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  ~Events() {
    for (hipEvent_t x : e) {
      if (x) hipEventDestroy(x);
    }
  }
};

struct OutCol {
  DevBuf<uint64_t> vals;
  DevBuf<uint8_t> nulls;
  DevBuf<uint8_t> heap;
  DevBuf<uint64_t> offsets;  // strings: sizes -> scanned offsets, [n] the total
  uint64_t heap_bytes = 0;
  const uint64_t* pages = nullptr;
  uint64_t src_bytes = 0;
};

}  // namespace

Status table_from_query(evql_query* q, const std::vector<ColumnSpec>& specs, int sort_column,
                        int page_order, evql_table** out, evql_materialize_stats_t* stats) {
  std::vector<MatSpec> mspecs;
  for (const ColumnSpec& c : specs) {
    mspecs.push_back(MatSpec{c.name, uint32_t(c.logical_type), c.rlevel_max, c.dlevel_max});
  }
  MatPlan plan;
  MatDecision dec = plan_materialize(materialize_input(q, &mspecs, sort_column), &plan);
  if (dec != MAT_DEVICE) return Status::error(mat_decision_code(dec), plan.reason);
  if (!q->executed) return Status::error(EVQL_EARG, "materialise: the query has not executed");

  evql_table* t = q->table;
  const KernelPlan& kp = q->rplan();
  hipStream_t s = q->ctx->stream;
  const uint32_t ncols = uint32_t(specs.size());
  const bool sorted = sort_column >= 0;
  evql_materialize_stats_t ms{};

  Events ev;
  for (hipEvent_t& e : ev.e) HIP_TRY(hipEventCreate(&e));
  HIP_TRY(hipEventRecord(ev.e[0], s));

  // ---- 2. records (their collection is part of the gather's time) -----------------------------
  FetchedRecords r;
  Status st = collect_records(q, &r);
  if (!st.ok()) return st;
  const uint64_t n = r.n;
  if (sorted && n > 0xffffffffull) {
    return Status::error(EVQL_ENOTSUP, "materialise: a sort of more than 2^32 - 1 rows");
  }
  ms.rows = n;

  // ---- 3. gather ------------------------------------------------------------------------------
  // status words: [0] NULL bits, [1] an index outside its array, [2] k_cmp_permute's
  DevBuf<uint64_t> d_status;
  uint64_t h_status[3] = {0, 0, 0};
  HIP_TRY(d_status.alloc(3 * 8));
  HIP_TRY(hipMemsetAsync(d_status, 0, 3 * 8, s));
  MatArgs ma{};
  ma.records = r.d_rec;
  ma.n = n;
  ma.rw = r.nwords + 1;
  ma.ncols = ncols;
  ma.status = d_status;
  FirstRows fr;
  if (plan.need_first && n) {
    // (this route bounds the recorded first rows by the table's rows: the emit routes do not)
    st = gather_first_rows(q, r.d_rec, n, ma.rw, t->layout.num_rows, d_status, &fr);
    if (!st.ok()) return st;
    ms.n_kernel_launches += 2;
    ma.first_vals = fr.vals;
    ma.first_tags = fr.tags;
  }
  std::vector<OutCol> cols(ncols);
  bool strings = false;
  for (uint32_t c = 0; c < ncols; ++c) {
    const MatCell& cell = plan.cells[c];
    OutCol& oc = cols[c];
    HIP_TRY(oc.vals.alloc(n * 8));
    if (cell.optional) HIP_TRY(oc.nulls.alloc(n));
    MatCol& mc = ma.col[c];
    static_cast<ResultCell&>(mc) = cell;
    mc.values = oc.vals;
    mc.nulls = oc.nulls;
    if (cell.is_string) {
      const int li = kp.cols[cell.src].layout_index;
      if (li < 0 || size_t(li) >= t->d_pages.size() || t->d_pages[li].empty()) {
        return Status::error(EVQL_ERUNTIME, "materialise: no pages behind string column " + specs[c].name);
      }
      oc.pages = t->d_pages[li][0];
      oc.src_bytes = uint64_t(t->layout.columns[li].data_pages.size()) * kPlainPageSize;
      strings = strings || n > 0;
    }
  }
  DevBuf<MatArgs> d_args;
  HIP_TRY(d_args.alloc(sizeof(MatArgs)));
  HIP_TRY(hipMemcpyAsync(d_args, &ma, sizeof(MatArgs), hipMemcpyHostToDevice, s));
  HIP_TRY(launch_mat_fixed(d_args, n, s));
  if (n) ++ms.n_kernel_launches;
  if (strings) {
    for (uint32_t c = 0; c < ncols; ++c) {
      if (!plan.cells[c].is_string) continue;
      OutCol& oc = cols[c];
      HIP_TRY(oc.offsets.alloc((n + 2) * 8));
      HIP_TRY(launch_mat_str_sizes(d_args, c, n, oc.src_bytes, oc.offsets, s));
      HIP_TRY(launch_exclusive_scan(oc.offsets, n, oc.offsets.p + n, s));
      HIP_TRY(hipMemcpyAsync(&oc.heap_bytes, oc.offsets.p + n, 8, hipMemcpyDeviceToHost, s));
      ms.n_kernel_launches += 2;
    }
  }
  HIP_TRY(hipEventRecord(ev.e[1], s));
  // ---- 4a. key statistics: they ride on the wait for the heap sizes ---------------------------
  DevBuf<uint64_t> d_kstats;
  uint64_t h_kstats[3] = {0, 0, 0};
  if (sorted && n) {
    HIP_TRY(d_kstats.alloc(3 * 8));
    HIP_TRY(hipMemsetAsync(d_kstats, 0, 3 * 8, s));
    HIP_TRY(launch_sort_key_stats(cols[sort_column].vals, n, d_kstats, s));
    HIP_TRY(hipMemcpyAsync(h_kstats, d_kstats.p, 3 * 8, hipMemcpyDeviceToHost, s));
    ++ms.n_kernel_launches;
  }
  HIP_TRY(hipEventRecord(ev.e[2], s));
  if (strings || (sorted && n)) {
    HIP_TRY(hipStreamSynchronize(s));
    ++ms.n_host_waits;
  }
  if (strings) {
    for (uint32_t c = 0; c < ncols; ++c) {
      if (!plan.cells[c].is_string) continue;
      OutCol& oc = cols[c];
      HIP_TRY(oc.heap.alloc(oc.heap_bytes));
      HIP_TRY(launch_mat_str_bytes(d_args, c, n, t->d_image, oc.pages, oc.src_bytes, oc.offsets, oc.heap,
                                   oc.heap_bytes, s));
      ++ms.n_kernel_launches;
      ms.string_bytes += oc.heap_bytes;
    }
  }
  HIP_TRY(hipEventRecord(ev.e[3], s));

  // ---- 4b. sort, 4c. permute ------------------------------------------------------------------
  RadixPassScratch sc;  // (sides and histograms are allocated by the passes that need them)
  DevBuf<CmpPermuteCol> d_pcols;
  std::vector<CmpPermuteCol> h_pcols;  // (lives until the stream has been synchronised)
  std::vector<OutCol> moved(ncols);
  if (sorted) {
    ms.presorted = h_kstats[2] == 0 || n <= 1;
    if (!ms.presorted) {
      const uint64_t kmin = ~h_kstats[0], kmax = h_kstats[1];
      uint32_t bits = 0;
      for (uint64_t range = kmax - kmin; range; range >>= 1) ++bits;
      ms.passes = (bits + 7) / 8;
      // the first pass reads the gathered column; its rows are the identity
      st = radix_sort_passes(cols[sort_column].vals, nullptr, n, kmin, ms.passes, &sc, s);
      if (!st.ok()) return st;
      ms.n_kernel_launches += 3 * ms.passes;
      const uint32_t last = (ms.passes - 1) & 1;
      // the key column's sorted words are the last pass's
      moved[sort_column].vals = std::move(cols[sort_column].vals);
      cols[sort_column].vals = std::move(sc.keys[last]);
      for (uint32_t c = 0; c < ncols; ++c) {
        if (int(c) == sort_column) continue;
        OutCol& oc = cols[c];
        OutCol& from = moved[c];
        from.vals = std::move(oc.vals);
        from.nulls = std::move(oc.nulls);
        HIP_TRY(oc.vals.alloc(n * 8));
        if (from.nulls.p) HIP_TRY(oc.nulls.alloc(n));
        h_pcols.push_back(CmpPermuteCol{from.vals.p, oc.vals.p, from.nulls.p, oc.nulls.p});
      }
      if (!h_pcols.empty()) {
        HIP_TRY(d_pcols.alloc(h_pcols.size() * sizeof(CmpPermuteCol)));
        HIP_TRY(hipMemcpyAsync(d_pcols, h_pcols.data(), h_pcols.size() * sizeof(CmpPermuteCol),
                               hipMemcpyHostToDevice, s));
        CmpPermuteArgs pa{};
        pa.perm = sc.idx[last];
        pa.n = n;
        pa.cols = d_pcols;
        pa.ncols = uint32_t(h_pcols.size());
        pa.status = d_status.p + 2;
        HIP_TRY(launch_cmp_permute(pa, s));
        ++ms.n_kernel_launches;
      }
    }
  }
  HIP_TRY(hipMemcpyAsync(h_status, d_status.p, 3 * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipEventRecord(ev.e[4], s));

  // ---- 5. encode ------------------------------------------------------------------------------
  std::vector<DeviceColumnIn> in;
  for (uint32_t c = 0; c < ncols; ++c) {
    const OutCol& oc = cols[c];
    in.push_back({oc.vals, oc.nulls, plan.cells[c].is_string ? oc.heap.p : nullptr, nullptr, nullptr, 0});
  }
  evql_table* nt = nullptr;
  st = table_from_device_columns(q->ctx, specs, in, n, page_order, &nt);
  if (!st.ok()) return st;
  std::unique_ptr<evql_table> owned(nt);
  HIP_TRY(hipEventRecord(ev.e[5], s));
  HIP_TRY(hipEventSynchronize(ev.e[5]));
  ++ms.n_host_waits;
  if (h_status[0]) {
    uint32_t c = 0;
    while (c + 1 < ncols && !((h_status[0] >> c) & 1)) ++c;
    return Status::error(EVQL_ERUNTIME, "NULL in required column " + specs[c].name);
  }
  if (h_status[1]) {
    return Status::error(EVQL_ERUNTIME, "materialise: a first row or a string position outside the table");
  }
  if (h_status[2]) {
    return Status::error(EVQL_ERUNTIME, "the sort's permutation names a row behind the last");
  }

  float g0 = 0, g1 = 0, s0 = 0, s1 = 0;
  HIP_TRY(hipEventElapsedTime(&g0, ev.e[0], ev.e[1]));
  HIP_TRY(hipEventElapsedTime(&s0, ev.e[1], ev.e[2]));
  HIP_TRY(hipEventElapsedTime(&g1, ev.e[2], ev.e[3]));
  HIP_TRY(hipEventElapsedTime(&s1, ev.e[3], ev.e[4]));
  HIP_TRY(hipEventElapsedTime(&ms.encode_ms, ev.e[4], ev.e[5]));
  ms.gather_ms = g0 + g1;
  ms.sort_ms = s0 + s1;
  if (stats) *stats = ms;
  *out = owned.release();
  return Status();
}

}  // namespace evql
