// bare_scan.cc -- scans without GROUP BY / aggregate (KernelPlan::bare_scan):
// FastCSTableScan::nextBatch and CSTableScan's NO_AGGREGATION path handing their rows
// straight to the caller.  The rows leave in ROW ORDER -- a LimitExpression above the scan
// depends on it -- and the result, which can be as large as the table, is never held whole:
//
//   execute      evql_scan_count: passing rows per tile; their exclusive scan gives every
//                tile the position of its first output row (no pass when there is neither a
//                WHERE nor a row filter: the counts are arithmetic)
//   next_batch   takes consecutive tiles while their passing rows fit one WINDOW, runs
//                evql_scan_emit over them (value word + tag per output column and row, in
//                row order), packs the columns as SVector bytes on the device (the packers
//                of large GROUP BY results, results.cc), copies the window once into pinned
//                memory and hands out slices of it
//
// LIMIT / OFFSET select a range of the ordered passing rows: tiles wholly in front of the
// offset are skipped by their counts, tiles behind offset + limit are never emitted.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <thread>
#include "runtime.h"

namespace evql {

namespace {

// host mirror of the generated EvqlScanArgs
struct HostScanArgs {
  const uint64_t* tile_offset;
  uint64_t t0, t1;
  uint64_t window_base;
  uint64_t window_rows;
  uint64_t* words;
  uint8_t* tags;
};
struct HostArgsWithCount {
  HostArgs a;
  uint32_t* tile_count;
};
struct HostArgsWithScan {
  HostArgs a;
  HostScanArgs s;
};

// device and pinned staging of one window, each
const uint64_t kWindowBytes = 256ull << 20;

Status status_error(uint32_t st) {
  if (st & 1u) return Status::error(EVQL_ERUNTIME, "division by zero");
  if (st & 4u) return Status::error(EVQL_ERUNTIME, "modulo by zero");
  return Status();
}

// [lo, hi) of the passing rows that LIMIT / OFFSET leave (limit.cc:52-125)
void apply_limit(evql_query* q) {
  evql_query::BareScan& b = q->bare;
  const uint64_t total = b.tile_off.empty() ? 0 : b.tile_off.back();
  b.lo = 0;
  b.hi = total;
  if (q->has_limit) {
    b.lo = std::min(q->offset, total);
    b.hi = q->limit == 0 ? b.lo : (q->limit > total - b.lo ? total : b.lo + q->limit);
  }
  b.pos = b.lo;
  b.win_base = 0;
  b.win_rows = 0;
}

}  // namespace

// window size: rows whose value words, tags and packed bytes fit kWindowBytes on the
// device, and whose packed bytes fit as much pinned memory (string bytes come on top);
// EVQL_SCAN_WINDOW_ROWS overrides it.  Never less than one tile.
void bare_configure(evql_query* q) {
  const uint64_t ncols = std::max<uint64_t>(q->kp.scan_out.size(), 1);
  uint64_t rows = kWindowBytes / (18 * ncols);
  if (const char* e = getenv("EVQL_SCAN_WINDOW_ROWS")) {
    char* end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    if (end != e && v > 0) rows = v;
  }
  q->bare.window_rows = rows;
}

Status bare_launch(evql_query* q) {
  evql_query::BareScan& b = q->bare;
  const KernelPlan& kp = q->kp;
  hipStream_t s = q->ctx->stream;
  HostArgsWithCount ac{};
  fill_host_args(q, &ac.a);
  const HostArgs& a = ac.a;
  b.ntiles = a.ntiles;
  zone_stats_after_run(q, a.ntiles, 0);
  if (b.tiles_cap < b.ntiles + 1) {
    HIP_TRY(b.d_tile_count.alloc((b.ntiles + 1) * 4));
    HIP_TRY(b.d_tile_off.alloc((b.ntiles + 1) * 8));
    b.tiles_cap = b.ntiles + 1;
  }
  HIP_TRY(hipMemsetAsync(q->d_status, 0, 16, s));
  HIP_TRY(hipMemsetAsync(q->d_counters, 0, 64, s));
  b.tile_off.assign(b.ntiles + 1, 0);
  b.counted_on_device = (kp.where || kp.has_row_filter) && b.ntiles > 0;
  b.hb = nullptr;  // (evql_query_execute hands its heartbeat over when it has finished)
  b.hb_user = nullptr;
  HIP_TRY(hipEventRecord(q->ev0, s));
  if (b.counted_on_device) {
    ac.tile_count = b.d_tile_count;
    size_t sz = sizeof(ac);
    void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &ac, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz,
                      HIP_LAUNCH_PARAM_END};
    const unsigned grid = unsigned(std::min<uint64_t>(uint64_t(q->grid), b.ntiles));
    HIP_TRY(hipModuleLaunchKernel(q->module.fn_scan_count, grid, 1, 1, kp.block, 1, 1, 0, s, nullptr,
                                  config));
    HIP_TRY(launch_scan_u32(b.d_tile_count, b.ntiles, b.d_tile_off, s));
    q->stats.n_kernel_launches = 2;
  } else {
    // every row of the range passes: the counts are the tiles' shares of [row_begin, row_end)
    const uint64_t T = uint64_t(kp.tile_rows());
    for (uint64_t t = 0; t < b.ntiles; ++t) {
      const uint64_t r0 = std::max(a.row_begin, (a.tile0 + t) * T);
      const uint64_t r1 = std::min(a.row_end, (a.tile0 + t + 1) * T);
      b.tile_off[t + 1] = b.tile_off[t] + (r1 > r0 ? r1 - r0 : 0);
    }
    HIP_TRY(hipMemcpyAsync(b.d_tile_off, b.tile_off.data(), (b.ntiles + 1) * 8, hipMemcpyHostToDevice, s));
    q->stats.n_kernel_launches = 0;
  }
  HIP_TRY(hipEventRecord(q->ev1, s));
  q->launched = true;
  q->stats.rows_scanned = a.row_end - a.row_begin;
  return Status();
}

Status bare_finish(evql_query* q) {
  if (!q->launched) return Status::error(EVQL_EARG, "query was not launched");
  evql_query::BareScan& b = q->bare;
  hipStream_t s = q->ctx->stream;
  uint32_t status[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(status, q->d_status, 16, hipMemcpyDeviceToHost, s));
  uint64_t skipped = 0;
  if (b.counted_on_device) {
    HIP_TRY(hipMemcpyAsync(b.tile_off.data(), b.d_tile_off, (b.ntiles + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&skipped, q->d_counters + 5, 8, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  q->launched = false;
  Status se = status_error(status[0]);  // raised by WHERE
  if (!se.ok()) return se;
  float ms = 0;
  hipEventElapsedTime(&ms, q->ev0, q->ev1);
  q->stats.kernel_ms = ms;
  q->stats.total_ms = ms;
  q->stats.rows_passed = b.tile_off.back();
  q->zstats.tiles_skipped = skipped;
  if (q->reported_rows_scanned != ~0ull) q->stats.rows_scanned = q->reported_rows_scanned;
  q->stats.num_groups = 0;
  q->stats.used_lds_table = 0;
  q->ngroups = 0;
  b.emit_ms = 0;
  b.windows = 0;
  apply_limit(q);
  q->executed = true;
  q->fetched = true;
  return Status();
}

// an executed scan of nothing (evql_query_reset)
Status bare_reset(evql_query* q) {
  evql_query::BareScan& b = q->bare;
  HIP_TRY(hipStreamSynchronize(q->ctx->stream));
  b.ntiles = 0;
  b.tile_off.assign(1, 0);
  q->stats.rows_scanned = 0;
  q->stats.rows_passed = 0;
  q->stats.num_groups = 0;
  apply_limit(q);
  q->launched = false;
  q->executed = true;
  q->fetched = true;
  return Status();
}

// evql_query_set_order on a bare scan: LIMIT / OFFSET alone (LimitExpression over the
// ordered rows); a sort would have to see every row first
Status bare_set_limit(evql_query* q, uint32_t n_specs, int64_t limit, uint64_t offset) {
  if (n_specs > 0) return Status::error(EVQL_ENOTSUP, "ORDER BY over a bare scan is not fused");
  if (limit < 0) return Status::error(EVQL_EARG, "can't execute ORDER BY: no sort specs");
  q->has_limit = true;
  q->limit = uint64_t(limit);
  q->offset = offset;
  if (q->executed) apply_limit(q);
  return Status();
}

// emits, packs and copies the window that starts with the tile holding passing row b.pos
static Status load_window(evql_query* q) {
  evql_query::BareScan& b = q->bare;
  evql_table* t = q->table;
  const KernelPlan& kp = q->kp;
  hipStream_t s = q->ctx->stream;
  const uint32_t ncols = uint32_t(kp.scan_out.size());
  // tile_off[t0] <= pos < tile_off[t0 + 1]; then consecutive tiles while they fit the window
  // and still hold rows of the result
  const uint64_t t0 =
      uint64_t(std::upper_bound(b.tile_off.begin(), b.tile_off.end(), b.pos) - b.tile_off.begin()) - 1;
  uint64_t t1 = t0 + 1;
  while (t1 < b.ntiles && b.tile_off[t1] < b.hi && b.tile_off[t1 + 1] - b.tile_off[t0] <= b.window_rows) {
    ++t1;
  }
  const uint64_t n = b.tile_off[t1] - b.tile_off[t0];
  if (b.stage_cap < n * ncols) {
    HIP_TRY(b.d_words.alloc(n * ncols * 8));
    HIP_TRY(b.d_tags.alloc(n * ncols));
    b.stage_cap = n * ncols;
  }
  // (tags are written for nullable outputs only)
  HIP_TRY(hipMemsetAsync(b.d_tags, 0, n * ncols, s));
  HostArgsWithScan as{};
  fill_host_args(q, &as.a);
  as.s.tile_offset = b.d_tile_off;
  as.s.t0 = t0;
  as.s.t1 = t1;
  as.s.window_base = b.tile_off[t0];
  as.s.window_rows = n;
  as.s.words = b.d_words;
  as.s.tags = b.d_tags;
  size_t sz = sizeof(as);
  void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &as, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz,
                    HIP_LAUNCH_PARAM_END};
  const unsigned grid = unsigned(std::min<uint64_t>(uint64_t(q->grid), t1 - t0));
  // the heartbeat of the execute that ran this scan: once per window before its kernels are
  // launched, then every 5 ms while they run (like evql_query_execute); a beat that asks to
  // stop is honoured once the kernels have drained
  bool aborted = b.hb && b.hb(b.hb_user) != 0;
  if (aborted) return Status::error(EVQL_ERUNTIME, "query aborted by heartbeat");
  HIP_TRY(hipEventRecord(q->ev0, s));
  HIP_TRY(hipModuleLaunchKernel(q->module.fn_scan_emit, grid, 1, 1, kp.block, 1, 1, 0, s, nullptr,
                                config));
  HIP_TRY(hipEventRecord(q->ev1, s));

  // the columns as SVector bytes (svalue.cc:410-517): fixed-width columns by one kernel,
  // strings by sizes -> scan -> byte copy
  EmitArgs ea{};
  ea.n = n;
  ea.ncols = ncols;
  ea.first_vals = b.d_words;
  ea.first_tags = b.d_tags;
  ea.image = t->d_image;
  for (uint32_t i = 0; i < ncols; ++i) {
    EmitCol& e = ea.col[i];
    e = EmitCol{};
    e.kind = 2;  // the value words the scan wrote, column i of [ncols][n]
    e.src = i;
    e.stype = kp.scan_out[i]->type;
    e.is_string = e.stype == EVQL_T_STRING;
    e.is_bool = e.stype == EVQL_T_BOOL;
    e.elem = e.is_string ? 0 : (e.is_bool ? 2 : 9);
    if (e.is_string) e.pages = t->d_pages[kp.cols[kp.scan_out[i]->input].layout_index][0];
  }
  EmitColumnsJob job;
  Status stb = emit_columns_begin(q, &ea, &job);
  if (!stb.ok()) return stb;
  uint32_t status[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(status, q->d_status, 16, hipMemcpyDeviceToHost, s));
  if (b.hb) {
    auto last = std::chrono::steady_clock::now();
    while (hipStreamQuery(s) == hipErrorNotReady) {
      std::this_thread::sleep_for(std::chrono::microseconds(200));
      const auto now = std::chrono::steady_clock::now();
      if (now - last >= std::chrono::milliseconds(5)) {
        last = now;
        if (b.hb(b.hb_user) != 0) aborted = true;
      }
    }
  }
  HIP_TRY(hipStreamSynchronize(s));
  if (aborted) return Status::error(EVQL_ERUNTIME, "query aborted by heartbeat");
  // raised by a select expression of a passing row of this window
  Status se = status_error(status[0]);
  if (!se.ok()) return se;
  stb = emit_columns_finish(q, &ea, &job);
  if (!stb.ok()) return stb;
  HIP_TRY(hipStreamSynchronize(s));
  float ms = 0;
  hipEventElapsedTime(&ms, q->ev0, q->ev1);
  b.emit_ms += ms;
  b.windows += 1;
  q->stats.total_ms = q->stats.kernel_ms + b.emit_ms;
  q->stats.n_kernel_launches += 2;
  b.win_base = b.tile_off[t0];
  b.win_rows = n;
  return Status();
}

Status bare_next_batch(evql_query* q, size_t max_rows, evql_column_buf_t* cols, size_t* nrows) {
  if (!q->executed) return Status::error(EVQL_EARG, "execute() was not called");
  evql_query::BareScan& b = q->bare;
  const size_t ncols = q->kp.scan_out.size();
  *nrows = 0;
  for (size_t i = 0; i < ncols; ++i) {
    cols[i].data = nullptr;
    cols[i].size = 0;
  }
  if (b.pos >= b.hi || max_rows == 0) return Status();
  if (b.win_rows == 0 || b.pos < b.win_base || b.pos >= b.win_base + b.win_rows) {
    Status st = load_window(q);
    if (!st.ok()) return st;
  }
  // (the boundary tiles of a LIMIT are trimmed here: the window holds whole tiles)
  const uint64_t end = std::min(b.hi, b.win_base + b.win_rows);
  const uint64_t m = std::min<uint64_t>(end - b.pos, max_rows);
  const uint64_t i0 = b.pos - b.win_base;
  const evql_query::DeviceEmit& de = q->demit;
  for (size_t i = 0; i < ncols; ++i) {
    if (de.elem[i]) {
      cols[i].data = de.col[i] + i0 * de.elem[i];
      cols[i].size = size_t(m) * de.elem[i];
    } else {
      const uint64_t b0 = de.off[i][i0], b1 = de.off[i][i0 + m];
      cols[i].data = de.col[i] + b0;
      cols[i].size = size_t(b1 - b0);
    }
  }
  b.pos += m;
  *nrows = size_t(m);
  return Status();
}

}  // namespace evql
