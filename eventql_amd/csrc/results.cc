// results.cc -- groups leaving the device: fetch, ORDER BY .. LIMIT, and emission as
// SVector columns (on the device for large results, on the host otherwise).
#include <algorithm>
#include <cmath>
#include <cstring>
#include "radix_sort.h"
#include "runtime.h"
#include "sha1.h"

namespace evql {

// ---------------------------------------------------------------------------
// large results: the output columns packed on the device
// ---------------------------------------------------------------------------
// GroupByExpression::nextBatch (groupby.cc:187-220) runs `method_call` of every select
// expression per group and appends the value to the column's SVector.  For 1e7 groups the
// host loop (record copy, sort, one eval_expr per cell) took seconds.  When every select
// expression is the group key, a bare aggregate or the first-row value of a scan column --
// config 4 / 4s, and what `select k, count(1), sum(x) .. group by k` looks like -- one
// kernel writes the packed SVector bytes (svalue.cc:410-517) of every column for ALL groups;
// the host copies each column once into pinned memory and next_batch hands out slices.
// Row order is unspecified for a GROUP BY without ORDER BY; small results keep the
// host path and its deterministic order.  With ORDER BY the rows come in the order of the
// specs, ties in the order of sort_host_records, whether the host (order_fetched) or the
// device (sort_on_device) sorted them.  (kDeviceEmitMinGroups: partial_emit_plan.h)

// device time and work of one packing: evql_query_emit_stats
struct PackMeter {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  uint32_t launches = 0, waits = 0;
  ~PackMeter() {
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
  }
  hipError_t begin(hipStream_t s) {
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipEventRecord(e0, s);
    return e;
  }
  // in front of the last synchronisation of the packing ...
  hipError_t mark_end(hipStream_t s) { return hipEventRecord(e1, s); }
  // ... and behind it
  hipError_t finish(evql_emit_stats_t* st) {
    float ms = 0;
    hipError_t e = hipEventElapsedTime(&ms, e0, e1);
    st->pack_ms = ms;
    st->n_kernel_launches = launches;
    st->n_host_waits = waits;
    return e;
  }
};

// `ordered`: the records are the ORDER BY / LIMIT slice already (sort_on_device); every other
// caller asks about a result that order_fetched would still have to reorder
static bool device_emit_columns(const evql_query* q, bool merged, EmitArgs* ea, bool ordered = false) {
  const KernelPlan& kp = q->rplan();
  const size_t nsel = q->select.size();
  if (q->group_mode != EVQL_MODE_FINAL) return false;
  if (!ordered && (!q->order.empty() || q->has_limit)) return false;
  if (nsel == 0 || nsel > kMaxEmitCols) return false;
  for (size_t i = 0; i < nsel; ++i) {
    const LoweredProgram& lp = q->select[i];
    EmitCol& e = ea->col[i];
    e = EmitCol{};
    e.stype = lp.return_type;
    e.is_bool = lp.return_type == EVQL_T_BOOL;
    e.elem = e.is_bool ? 2 : 9;
    if (lp.return_type == EVQL_T_NIL) return false;
    if (lp.is_aggregate) {
      if (lp.call->kind != Expr::AGG_GET) return false;  // post-aggregate arithmetic: host
      const AggPlan* a = nullptr;
      if (!aggregate_cell(kp, q->select_agg_index[i], &e, &a)) return false;
      if (a->exact_index >= 0) return false;  // (128-bit rounding of an exact sum: host)
    } else if (q->select_passthrough[i]) {
      // (any key mode, and no bare-column rule: the other routes ask for both)
      if (lp.return_type == EVQL_T_STRING) return false;
      e.kind = 0;
    } else {
      if (merged || !kp.need_first_row || q->nested) return false;
      // (a string column is taken by string_hash alone; the other routes also ask that the
      // expression's type is STRING)
      if (!first_row_cell(kp, q->scan_select, lp, &e)) return false;
      if (e.is_string) e.elem = 0;
    }
  }
  ea->ncols = uint32_t(nsel);
  return true;
}

Status pinned_reserve(uint8_t** p, size_t* cap, size_t bytes) {
  if (bytes <= *cap && *p) return Status();
  if (*p) hipHostFree(*p);
  *p = nullptr;
  *cap = 0;
  const size_t want = bytes + bytes / 8 + 4096;
  HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(p), want, hipHostMallocDefault));
  *cap = want;
  return Status();
}

Status gather_first_rows(evql_query* q, const uint64_t* d_rec, uint64_t n, uint32_t rw,
                         uint64_t row_limit, uint64_t* d_status, FirstRows* fr) {
  const KernelPlan& kp = q->rplan();
  hipStream_t s = q->ctx->stream;
  const uint32_t nc = uint32_t(kp.cols.size());
  Status st = first_row_columns(q, &fr->host_cols);
  if (!st.ok()) return st;
  if (d_rec) HIP_TRY(fr->rows.alloc(n * 8));
  HIP_TRY(fr->cols.alloc(nc * sizeof(RtColumn)));
  HIP_TRY(fr->vals.alloc(n * nc * 8));
  HIP_TRY(fr->tags.alloc(n * nc));
  const uint32_t word = uint32_t(1 + kp.first_row_word());
  if (d_rec && row_limit != kNoRowLimit) {
    HIP_TRY(launch_mat_first_rows(d_rec, n, rw, word, row_limit, fr->rows, d_status, s));
  } else if (d_rec) {
    HIP_TRY(launch_extract_word(d_rec, n, rw, word, fr->rows, s));
  }
  HIP_TRY(hipMemcpyAsync(fr->cols, fr->host_cols.data(), nc * sizeof(RtColumn), hipMemcpyHostToDevice, s));
  HIP_TRY(launch_gather_rows(q->table->d_image, fr->cols, nc, fr->rows, n, fr->vals, fr->tags, s));
  return Status();
}

Status emit_columns_begin(evql_query* q, EmitArgs* ea, EmitColumnsJob* job) {
  hipStream_t s = q->ctx->stream;
  const uint32_t ncols = ea->ncols;
  const uint64_t n = ea->n;
  evql_query::DeviceEmit& de = q->demit;
  de.col.resize(ncols, nullptr);
  de.col_cap.resize(ncols, 0);
  de.off.resize(ncols, nullptr);
  de.off_cap.resize(ncols, 0);
  de.elem.assign(ncols, 0);
  // device buffers of the packed columns
  job->d_out = std::vector<DevBuf<uint8_t>>(ncols);
  job->d_off = std::vector<DevBuf<uint64_t>>(ncols);
  job->str_bytes.assign(ncols, 0);
  HIP_TRY(job->d_args.alloc(sizeof(EmitArgs)));
  for (uint32_t i = 0; i < ncols; ++i) {
    EmitCol& e = ea->col[i];
    de.elem[i] = e.elem;
    if (e.elem) {
      HIP_TRY(job->d_out[i].alloc(n * e.elem));
      e.out = job->d_out[i];
    } else {
      HIP_TRY(job->d_off[i].alloc((n + 2) * 8));
    }
  }
  HIP_TRY(hipMemcpyAsync(job->d_args, ea, sizeof(EmitArgs), hipMemcpyHostToDevice, s));
  HIP_TRY(launch_emit_fixed(job->d_args, n, s));
  ++job->launches;
  for (uint32_t i = 0; i < ncols; ++i) {
    if (ea->col[i].elem) continue;
    HIP_TRY(launch_emit_str_sizes(job->d_args, i, n, job->d_off[i], s));
    HIP_TRY(launch_exclusive_scan(job->d_off[i], n, job->d_off[i].p + n, s));
    HIP_TRY(hipMemcpyAsync(&job->str_bytes[i], job->d_off[i].p + n, 8, hipMemcpyDeviceToHost, s));
    job->launches += 2;
  }
  return Status();
}

Status emit_columns_finish(evql_query* q, EmitArgs* ea, EmitColumnsJob* job) {
  hipStream_t s = q->ctx->stream;
  const uint32_t ncols = ea->ncols;
  const uint64_t n = ea->n;
  evql_query::DeviceEmit& de = q->demit;
  bool strings = false;
  for (uint32_t i = 0; i < ncols; ++i) {
    if (ea->col[i].elem) continue;
    strings = true;
    HIP_TRY(job->d_out[i].alloc(job->str_bytes[i] + 16));
    ea->col[i].out = job->d_out[i];
    ea->col[i].offsets = job->d_off[i];
  }
  if (strings) {
    HIP_TRY(hipMemcpyAsync(job->d_args, ea, sizeof(EmitArgs), hipMemcpyHostToDevice, s));
    for (uint32_t i = 0; i < ncols; ++i) {
      if (ea->col[i].elem) continue;
      HIP_TRY(launch_emit_str_bytes(job->d_args, i, n, s));
      ++job->launches;
    }
  }
  // one copy per column into pinned host memory
  for (uint32_t i = 0; i < ncols; ++i) {
    const size_t bytes = ea->col[i].elem ? size_t(n) * ea->col[i].elem : size_t(job->str_bytes[i]);
    Status st = pinned_reserve(&de.col[i], &de.col_cap[i], bytes);
    if (!st.ok()) return st;
    if (bytes) HIP_TRY(hipMemcpyAsync(de.col[i], job->d_out[i], bytes, hipMemcpyDeviceToHost, s));
    if (!ea->col[i].elem) {
      uint8_t* po = reinterpret_cast<uint8_t*>(de.off[i]);
      st = pinned_reserve(&po, &de.off_cap[i], (n + 1) * 8);
      de.off[i] = reinterpret_cast<uint64_t*>(po);
      if (!st.ok()) return st;
      HIP_TRY(hipMemcpyAsync(de.off[i], job->d_off[i], (n + 1) * 8, hipMemcpyDeviceToHost, s));
    }
  }
  return Status();
}

static Status emit_on_device(evql_query* q, EmitArgs& ea, const uint64_t* d_rec, uint64_t n,
                             uint32_t nwords) {
  evql_table* t = q->table;
  const KernelPlan& kp = q->rplan();
  hipStream_t s = q->ctx->stream;
  const uint32_t nsel = ea.ncols;
  PackMeter pm;
  HIP_TRY(pm.begin(s));
  ea.records = d_rec;
  ea.n = n;
  ea.rw = nwords + 1;
  ea.image = t->d_image;
  bool need_first = false;
  for (uint32_t i = 0; i < nsel; ++i) {
    EmitCol& e = ea.col[i];
    need_first = need_first || e.kind == 2;
    if (!e.elem) e.pages = t->d_pages[kp.cols[e.src].layout_index][0];
  }
  FirstRows fr;
  if (need_first) {
    // (no row limit: this route trusts the recorded first rows; and it waits here, where the
    // PARTIAL route does not)
    Status stf = gather_first_rows(q, d_rec, n, nwords + 1, kNoRowLimit, nullptr, &fr);
    if (!stf.ok()) return stf;
    HIP_TRY(hipStreamSynchronize(s));
    pm.launches += 2;
    ++pm.waits;
    ea.first_vals = fr.vals;
    ea.first_tags = fr.tags;
  }
  EmitColumnsJob job;
  Status st = emit_columns_begin(q, &ea, &job);
  if (!st.ok()) return st;
  HIP_TRY(hipStreamSynchronize(s));
  ++pm.waits;
  st = emit_columns_finish(q, &ea, &job);
  if (!st.ok()) return st;
  pm.launches += job.launches;
  HIP_TRY(pm.mark_end(s));
  HIP_TRY(hipStreamSynchronize(s));
  ++pm.waits;
  HIP_TRY(pm.finish(&q->estats));
  q->demit.active = true;
  return Status();
}

// ---------------------------------------------------------------------------
// large EVQL_MODE_PARTIAL results: the (key, data) rows packed on the device
// ---------------------------------------------------------------------------
// PartialGroupByExpression (groupby.cc:438-472) sends (SHA-1 of the group tuple, concatenated
// saved states) per group.  The row loop of query_next_batch boxes every cell, allocates three
// vectors and runs one host sha1() per group.  For the plans plan_partial_emit accepts the same
// bytes are written by kernels: per-group sizes, two scans, the tuple heap (staging: only its
// digests leave the device), the data column, SHA-1 per tuple.
PartialEmitInput partial_emit_input(const evql_query* q, uint64_t n) {
  PartialEmitInput in;
  in.group_mode = q->group_mode;
  in.n = n;
  in.enabled = q->partial_device_emit;
  in.merged = q->merged;
  in.nested = q->nested;
  in.kp = &q->rplan();
  in.scan_select = &q->scan_select;
  in.group = &q->group;
  in.select = &q->select;
  in.select_agg_index = &q->select_agg_index;
  in.select_passthrough = &q->select_passthrough;
  return in;
}

static Status emit_partial_on_device(evql_query* q, const PartialEmitPlan& plan, const uint64_t* d_rec,
                                     uint64_t n, uint32_t nwords) {
  evql_table* t = q->table;
  const KernelPlan& kp = q->rplan();
  hipStream_t s = q->ctx->stream;
  evql_query::DeviceEmit& de = q->demit;
  PackMeter pm;
  HIP_TRY(pm.begin(s));
  de.col.resize(2, nullptr);
  de.col_cap.resize(2, 0);
  de.off.resize(2, nullptr);
  de.off_cap.resize(2, 0);
  de.elem.assign(2, 0);
  de.elem[0] = 25;  // u32 20, the digest, tag 0
  PartialArgs pa{};
  pa.records = d_rec;
  pa.n = n;
  pa.rw = nwords + 1;
  pa.image = t->d_image;
  pa.n_tuple = uint32_t(plan.tuple.size());
  pa.n_data = uint32_t(plan.data.size());
  for (uint32_t i = 0; i < pa.n_tuple; ++i) {
    pa.tuple[i] = plan.tuple[i];
    if (pa.tuple[i].is_string) pa.tuple[i].pages = t->d_pages[kp.cols[pa.tuple[i].src].layout_index][0];
  }
  for (uint32_t i = 0; i < pa.n_data; ++i) {
    pa.data[i] = plan.data[i];
    if (pa.data[i].is_string) pa.data[i].pages = t->d_pages[kp.cols[pa.data[i].src].layout_index][0];
  }
  FirstRows fr;
  if (plan.need_first) {
    // (no row limit: this route trusts the recorded first rows)
    Status stf = gather_first_rows(q, d_rec, n, nwords + 1, kNoRowLimit, nullptr, &fr);
    if (!stf.ok()) return stf;
    pm.launches += 2;
    pa.first_vals = fr.vals;
    pa.first_tags = fr.tags;
  }
  // sizes -> offsets; one wait reads both totals
  DevBuf<PartialArgs> d_args;
  DevBuf<uint64_t> d_toff, d_doff;
  HIP_TRY(d_args.alloc(sizeof(PartialArgs)));
  HIP_TRY(d_toff.alloc((n + 2) * 8));
  HIP_TRY(d_doff.alloc((n + 2) * 8));
  HIP_TRY(hipMemcpyAsync(d_args, &pa, sizeof(PartialArgs), hipMemcpyHostToDevice, s));
  HIP_TRY(launch_partial_sizes(d_args, n, d_toff, d_doff, s));
  HIP_TRY(launch_exclusive_scan(d_toff, n, d_toff.p + n, s));
  HIP_TRY(launch_exclusive_scan(d_doff, n, d_doff.p + n, s));
  uint64_t totals[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(&totals[0], d_toff.p + n, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&totals[1], d_doff.p + n, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  pm.launches += 3;
  ++pm.waits;
  // bytes and digests
  DevBuf<uint8_t> d_theap, d_data, d_key;
  HIP_TRY(d_theap.alloc(totals[0] + 16));
  HIP_TRY(d_data.alloc(totals[1] + 16));
  HIP_TRY(d_key.alloc(n * 25));
  HIP_TRY(launch_partial_tuple_bytes(d_args, n, d_toff, d_theap, s));
  HIP_TRY(launch_partial_data_bytes(d_args, n, d_doff, d_data, s));
  HIP_TRY(launch_sha1_ranges(d_theap, d_toff, n, d_key, 25, 1, s));
  pm.launches += 3;
  // one copy per column into pinned host memory
  Status st = pinned_reserve(&de.col[0], &de.col_cap[0], n * 25);
  if (!st.ok()) return st;
  st = pinned_reserve(&de.col[1], &de.col_cap[1], totals[1]);
  if (!st.ok()) return st;
  uint8_t* po = reinterpret_cast<uint8_t*>(de.off[1]);
  st = pinned_reserve(&po, &de.off_cap[1], (n + 1) * 8);
  de.off[1] = reinterpret_cast<uint64_t*>(po);
  if (!st.ok()) return st;
  HIP_TRY(hipMemcpyAsync(de.col[0], d_key, n * 25, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(de.col[1], d_data, totals[1], hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(de.off[1], d_doff, (n + 1) * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(pm.mark_end(s));
  HIP_TRY(hipStreamSynchronize(s));
  ++pm.waits;
  HIP_TRY(pm.finish(&q->estats));
  q->estats.key_bytes = n * 25;
  q->estats.data_bytes = totals[1];
  de.active = true;
  return Status();
}

// evql_ctx_sha1_ranges: k_sha1_ranges over host bytes (offsets validated by the caller)
Status sha1_ranges_on_device(evql_ctx* ctx, const void* bytes, size_t len, const uint64_t* offsets,
                             size_t n, uint8_t* out20) {
  if (n == 0) return Status();
  hipStream_t s = ctx->stream;
  DevBuf<uint8_t> d_bytes, d_out;
  DevBuf<uint64_t> d_off;
  HIP_TRY(d_bytes.alloc(len));
  HIP_TRY(d_off.alloc((n + 1) * 8));
  HIP_TRY(d_out.alloc(n * 20));
  if (len) HIP_TRY(hipMemcpyAsync(d_bytes, bytes, len, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_off, offsets, (n + 1) * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(launch_sha1_ranges(d_bytes, d_off, n, d_out, 20, 0, s));
  HIP_TRY(hipMemcpyAsync(out20, d_out, n * 20, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return Status();
}

// step 1: the dense records of the partitioned path and the compacted slots of the group
// table (after an exchange: of the merged table) in one buffer (FetchedRecords: runtime.h)
Status collect_records(evql_query* q, FetchedRecords* r) {
  evql_ctx* ctx = q->ctx;
  const KernelPlan& kp = q->rplan();
  hipStream_t s = ctx->stream;
  // after an exchange the groups live in the merged table (wider slots)
  const bool merged = q->merged;
  r->nwords = merged ? q->m_words : uint32_t(kp.words_per_slot());
  uint64_t* const gtab = merged ? q->d_mtab : q->d_gtab;
  const uint64_t gcap = merged ? (q->merged_dense ? q->mdense_n : q->mcap) : q->gcap;
  const uint64_t stride = gcap + 8;
  const uint64_t maxrec = gcap + 2;
  RecordsView view;
  if (!merged) {
    Status stv = query_records_view(q, &view);
    if (!stv.ok()) return stv;
  }
  const uint64_t dense_n = merged ? 0 : view.nd;
  uint64_t* d_cnt = q->d_counters + 5;
  // the record buffer is sized by the number of groups (counted by finish /
  // recount / reset), not by the table capacity
  r->n = q->stats.num_groups;
  if (r->n > maxrec + dense_n) r->n = maxrec + dense_n;
  r->total = r->n;
  // small results (the usual case) reuse a per-query 1 MiB buffer: no allocation
  // inside a step
  const size_t kSmallRec = 1 << 20;
  if (r->n && merged && q->merged_dense) {
    // (a bucketed merge left the groups as dense records already)
    r->n = std::min(r->n, q->mdense_n);
    r->d_rec = q->d_mdense;
  } else if (r->n) {
    if (r->n * (r->nwords + 1) * 8 <= kSmallRec) {
      if (!q->d_small_rec) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&q->d_small_rec), kSmallRec));
      r->d_rec = q->d_small_rec;
    } else {
      HIP_TRY(r->own.alloc(r->n * (r->nwords + 1) * 8));
      r->d_rec = r->own;
    }
    // dense records of the partitioned path first, the table's groups behind them
    const uint64_t nd = std::min(dense_n, r->n);
    if (nd) {
      HIP_TRY(hipMemcpyAsync(r->d_rec, view.dense, nd * (r->nwords + 1) * 8, hipMemcpyDeviceToDevice, s));
    }
    HIP_TRY(hipMemsetAsync(d_cnt, 0, 8, s));
    if (r->n > nd) {
      HIP_TRY(launch_table_compact(gtab, gcap, stride, r->nwords, r->d_rec + nd * (r->nwords + 1),
                                   r->n - nd, d_cnt, s));
    }
  }
  return Status();
}

// step 2, ORDER BY .. LIMIT asking for fewer rows than there are groups: only the
// want = offset + limit smallest records by the first sort key (plus, with further sort
// keys, every tie of the boundary key) leave the device: radix select over the dense
// records, 8 bits per pass
static Status select_top_records(evql_query* q, uint64_t want, FetchedRecords* r) {
  hipStream_t s = q->ctx->stream;
  uint64_t m = 0;
  if (want > 0) {
    DevBuf<uint64_t> d_keys, d_hist, d_idx, d_ctr;
    HIP_TRY(d_keys.alloc(r->n * 8));
    HIP_TRY(d_hist.alloc(256 * 8));
    HIP_TRY(d_idx.alloc(r->n * 8));
    HIP_TRY(d_ctr.alloc(3 * 8));
    OrderKeyArgs ka = q->order_key;
    ka.records = r->d_rec;
    ka.record_words = r->nwords + 1;
    ka.n = r->n;
    ka.keys = d_keys;
    HIP_TRY(launch_order_keys(ka, s));
    uint64_t hi_mask = 0, hi_value = 0, remaining = want;
    for (int shift = 56; shift >= 0; shift -= 8) {
      uint64_t hist[256];
      HIP_TRY(hipMemsetAsync(d_hist, 0, sizeof(hist), s));
      HIP_TRY(launch_radix_hist(d_keys, r->n, hi_mask, hi_value, uint32_t(shift), d_hist, s));
      HIP_TRY(hipMemcpyAsync(hist, d_hist, sizeof(hist), hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      uint64_t d = 0;
      while (d < 255 && hist[d] < remaining) remaining -= hist[d++];
      hi_value |= d << shift;
      hi_mask |= 0xFFull << shift;
    }
    // `remaining` = how many records with key == hi_value the result needs
    const uint64_t max_eq = q->order.size() == 1 ? remaining : r->n;
    uint64_t ctr[3] = {0, 0, 0};
    HIP_TRY(hipMemsetAsync(d_ctr, 0, sizeof(ctr), s));
    HIP_TRY(launch_order_collect(d_keys, r->n, hi_value, max_eq, d_idx, d_ctr, s));
    HIP_TRY(hipMemcpyAsync(ctr, d_ctr, sizeof(ctr), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    m = ctr[2];
    DevBuf<uint64_t> d_rec2;
    HIP_TRY(d_rec2.alloc(m * (r->nwords + 1) * 8));
    HIP_TRY(launch_gather_records(r->d_rec, r->nwords + 1, d_idx, m, d_rec2, s));
    HIP_TRY(hipStreamSynchronize(s));
    r->own = std::move(d_rec2);
    r->d_rec = r->own;
  }
  r->n = m;
  return Status();
}

// step 3: the records on the host in a deterministic order: by first row (scan order) or
// by identity
static void sort_host_records(evql_query* q, uint64_t n, uint32_t nwords) {
  const KernelPlan& kp = q->rplan();
  const size_t rw = nwords + 1;
  std::vector<uint64_t> idx(n);
  for (uint64_t i = 0; i < n; ++i) idx[i] = i;
  const size_t keyw = kp.need_first_row ? size_t(1 + kp.first_row_word()) : 1;
  const uint64_t* r = q->records.data();
  std::sort(idx.begin(), idx.end(), [&](uint64_t a, uint64_t b) {
    const uint64_t ka = r[a * rw + keyw], kb = r[b * rw + keyw];
    if (ka != kb) return ka < kb;
    return r[a * rw] < r[b * rw];
  });
  std::vector<uint64_t> sorted(q->records.size());
  for (uint64_t i = 0; i < n; ++i) {
    memcpy(&sorted[i * rw], &r[idx[i] * rw], rw * 8);
  }
  q->records.swap(sorted);
}

// (`in_order`: the records are the sorted slice of sort_on_device and stay as they come)
static Status records_to_host(evql_query* q, const uint64_t* d_rec, uint64_t n, uint32_t nwords,
                              bool in_order) {
  hipStream_t s = q->ctx->stream;
  q->records.assign(n * (nwords + 1), 0);
  if (n) {
    HIP_TRY(hipMemcpyAsync(q->records.data(), d_rec, n * (nwords + 1) * 8,
                           hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  if (!in_order) sort_host_records(q, n, nwords);
  return Status();
}

// ---------------------------------------------------------------------------
// ORDER BY over a large result: sorted on the device
// ---------------------------------------------------------------------------
// order_fetched boxes every cell of every group and runs a std::stable_sort with value_cmp
// over the records in sort_host_records order.  For the results plan_order_sort accepts the
// same order comes out of stable LSD radix sorts over order-preserving keys, least significant
// first: the kind word and the base word (sort_host_records' order), then the specs from the
// last to the first.  The OFFSET / LIMIT slice is gathered in that order and emitted as it lies.
OrderSortInput order_sort_input(const evql_query* q, uint64_t n) {
  OrderSortInput in;
  in.group_mode = q->group_mode;
  in.n = n;
  in.enabled = q->order_device_sort;
  in.kp = &q->rplan();
  in.select = &q->select;
  in.select_agg_index = &q->select_agg_index;
  in.select_passthrough = &q->select_passthrough;
  in.order = &q->order;
  in.order_desc = &q->order_desc;
  return in;
}

// rows [lo, hi) of n ordered records are the result, as order_fetched has it
static void limit_slice(const evql_query* q, uint64_t n, uint64_t* lo, uint64_t* hi) {
  *lo = 0;
  *hi = n;
  if (q->has_limit) {
    *lo = std::min(q->offset, n);
    *hi = q->limit == 0 ? *lo : std::min(n, q->offset + q->limit);
    if (*hi < *lo) *hi = *lo;  // (offset + limit wrapped)
  }
}

// step 2b: r's records become the ordered slice.  A NaN float key leaves r as it is and
// q->ostats.decision = OSORT_NAN_KEY: value_cmp on a NaN is no order a radix sort reproduces.
static Status sort_on_device(evql_query* q, const OrderSortPlan& plan, FetchedRecords* r) {
  hipStream_t s = q->ctx->stream;
  const uint64_t n = r->n;
  const uint32_t rw = r->nwords + 1;
  evql_order_stats_t& os = q->ostats;
  uint64_t lo, hi;
  limit_slice(q, n, &lo, &hi);
  const uint64_t m = hi - lo;
  PackMeter pm;
  HIP_TRY(pm.begin(s));
  // every allocation of the sort, once
  DevBuf<uint64_t> d_keys, d_out;
  DevBuf<uint32_t> d_idx;
  RadixSortScratch sc;
  HIP_TRY(d_keys.alloc(n * 8));
  HIP_TRY(d_idx.alloc(n * 4));
  HIP_TRY(d_out.alloc(m * rw * 8));
  Status st = sc.alloc(n);
  if (!st.ok()) return st;
  HIP_TRY(hipMemsetAsync(sc.stats, 0, 4 * 8, s));
  // least significant key first: kind, base word, specs last to first
  const size_t ns = plan.keys.size();
  for (size_t k = 0; k < ns + 2 && m > 0; ++k) {
    OrdKeyPermArgs ka{};
    if (k < 2) {
      ka.plain_word = 1;
      ka.key.word = k == 0 ? 0 : plan.base_word;
    } else {
      ka.key = plan.keys[ns + 1 - k];
    }
    ka.key.records = r->d_rec;
    ka.key.record_words = rw;
    ka.key.n = n;
    ka.key.keys = d_keys;
    ka.perm = sc.idx_identity ? nullptr : d_idx.p;
    ka.status = sc.stats.p + 3;
    HIP_TRY(launch_ord_key_perm(ka, s));
    ++sc.launches;
    st = radix_sort_pairs(&d_keys, &d_idx, n, &sc, s, &os.n_sort_passes, &os.n_passes_skipped);
    if (!st.ok()) return st;
    ++os.n_keys;
    if (sc.h_stats[3] & kOrdStatusBounds) {
      return Status::error(EVQL_ERUNTIME, "order sort: a permutation entry outside the records");
    }
    if (sc.h_stats[3] & kOrdStatusNaN) {
      os.decision = OSORT_NAN_KEY;
      os.n_kernel_launches = sc.launches;
      os.n_host_waits = sc.waits;
      return Status();
    }
  }
  uint64_t gather_status = 0;
  HIP_TRY(launch_ord_gather(r->d_rec, rw, n, sc.idx_identity ? nullptr : d_idx.p, lo, m, d_out,
                            sc.stats.p + 3, s));
  HIP_TRY(hipMemcpyAsync(&gather_status, sc.stats.p + 3, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(pm.mark_end(s));
  HIP_TRY(hipStreamSynchronize(s));
  if (m) ++sc.launches;
  ++sc.waits;
  if (gather_status & kOrdStatusBounds) {
    return Status::error(EVQL_ERUNTIME, "order sort: a permutation entry outside the records");
  }
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, pm.e0, pm.e1));
  os.sort_ms = ms;
  os.n_kernel_launches = sc.launches;
  os.n_host_waits = sc.waits;
  os.sorted_on_device = 1;
  r->own = std::move(d_out);
  r->d_rec = r->own;
  r->n = m;
  return Status();
}

// steps 1 to 3 of an eager step tail (query_run.cc): the epilogue of the launch left the
// records in the pinned block, finish has waited for it -- no device work here
static void records_from_block(evql_query* q, uint64_t n, uint32_t nwords) {
  const uint64_t* rec = q->h_tail + kTailRecords;
  q->records.assign(rec, rec + n * (nwords + 1));
  sort_host_records(q, n, nwords);
}

// step 4a, after an exchange: the first-row values of every scan column out of the merged
// records
static Status first_rows_from_records(evql_query* q, uint64_t n, uint32_t nwords) {
  const KernelPlan& kp = q->rplan();
  // the merged records carry the first-row values themselves: one word per scan
  // column, one word of NULL-tag bits; string words point into the received bytes
  const uint32_t nc = uint32_t(kp.cols.size());
  const size_t rw = nwords + 1, fr0 = size_t(kp.words_per_slot()) + 1;
  q->first_vals.resize(n * nc);
  q->first_tags.resize(n * nc);
  q->first_str_off.assign(n * nc, 0);
  q->first_str_heap = q->m_heap;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t* rec = &q->records[i * rw];
    const uint64_t tags = rec[fr0 + nc];
    for (uint32_t c = 0; c < nc; ++c) {
      q->first_vals[uint64_t(c) * n + i] = rec[fr0 + c];
      q->first_tags[uint64_t(c) * n + i] = uint8_t((tags >> c) & 1);
      if (kp.cols[c].string_hash) {
        const uint64_t off = rec[fr0 + c] & kStrOffMask;
        if (off + (rec[fr0 + c] >> 40) > q->first_str_heap.size()) {
          return Status::error(EVQL_ERUNTIME, "exchange: string offset outside the received bytes");
        }
        q->first_str_off[uint64_t(c) * n + i] = off;
      }
    }
  }
  return Status();
}

// step 4b: the first-row values of every scan column gathered from the table, and the bytes
// of the strings among them
static Status first_rows_from_table(evql_query* q, uint64_t n, uint32_t nwords) {
  evql_table* t = q->table;
  const KernelPlan& kp = q->rplan();
  hipStream_t s = q->ctx->stream;
  const uint32_t nc = uint32_t(kp.cols.size());
  std::vector<uint64_t> rows(n);
  const size_t rw = nwords + 1;
  // (never hand an unrecorded first row to the gather: it would read far outside the table)
  const uint64_t row_limit = q->nested ? q->nested_rows : t->layout.num_rows;
  for (uint64_t i = 0; i < n; ++i) {
    rows[i] = q->records[i * rw + 1 + kp.first_row_word()];
    if (rows[i] >= row_limit) {
      return Status::error(EVQL_ERUNTIME, "a group's first row was not recorded");
    }
  }
  // (the rows are on the host already and checked above: they go up as they are)
  FirstRows fr;
  HIP_TRY(fr.rows.alloc(n * 8));
  HIP_TRY(hipMemcpyAsync(fr.rows, rows.data(), n * 8, hipMemcpyHostToDevice, s));
  Status stf = gather_first_rows(q, nullptr, n, 0, kNoRowLimit, nullptr, &fr);
  if (!stf.ok()) return stf;
  q->first_vals.resize(n * nc);
  q->first_tags.resize(n * nc);
  HIP_TRY(hipMemcpyAsync(q->first_vals.data(), fr.vals, n * nc * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(q->first_tags.data(), fr.tags, n * nc, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  // bytes of the first-row strings: one packed heap per string column
  q->first_str_off.assign(n * nc, 0);
  q->first_str_heap.clear();
  for (uint32_t c = 0; c < nc; ++c) {
    const ColAccess& ca = kp.cols[c];
    if (!ca.string_hash) continue;
    std::vector<uint64_t> offs(n);
    uint64_t total = q->first_str_heap.size();
    const uint64_t heap0 = total;
    for (uint64_t i = 0; i < n; ++i) {
      offs[i] = total - heap0;
      q->first_str_off[uint64_t(c) * n + i] = total;
      if (!q->first_tags[uint64_t(c) * n + i]) total += q->first_vals[uint64_t(c) * n + i] >> 40;
    }
    const uint64_t bytes = total - heap0;
    q->first_str_heap.resize(total);
    if (bytes == 0) continue;
    DevBuf<uint64_t> d_offs;
    DevBuf<uint8_t> d_heap;
    HIP_TRY(d_offs.alloc(n * 8));
    HIP_TRY(d_heap.alloc(bytes));
    HIP_TRY(hipMemcpyAsync(d_offs, offs.data(), n * 8, hipMemcpyHostToDevice, s));
    // (NULL rows carry strpos 0: length 0, nothing copied)
    HIP_TRY(launch_copy_strings(t->d_image, t->d_pages[ca.layout_index][0], fr.vals.p + uint64_t(c) * n,
                                d_offs, n, d_heap, s));
    HIP_TRY(hipMemcpyAsync(q->first_str_heap.data() + heap0, d_heap, bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  return Status();
}

// step 5, PARTIAL mode: the distinct values of every group and count_distinct aggregate
static Status fetch_distinct_sets(evql_query* q, uint64_t n, uint32_t nwords) {
  const KernelPlan& kp = q->rplan();
  const bool merged = q->merged;
  q->distinct_values.clear();
  if (q->group_mode == EVQL_MODE_PARTIAL && kp.n_distinct > 0) {
    // count_distinct's saved state is the set itself (aggregate.cc:111-117): the
    // (group, value, flags) triples of the aggregate's pair set, grouped on the host
    const bool hashed = kp.key_mode == KEY_HASHED;
    q->distinct_values.resize(kp.n_distinct);
    std::vector<uint64_t> host;
    for (int d = 0; d < kp.n_distinct; ++d) {
      // (merged results: the union of the ranks' / tables' sets, exchange.cc)
      const uint64_t cap = merged ? q->mset_cap[d] : q->pairset_cap;
      const uint64_t* d_set = merged ? q->d_mset[d] : q->d_pairset[d];
      host.assign(cap * 3, ~0ull);
      if (d_set && cap) HIP_TRY(hipMemcpy(host.data(), d_set, cap * 3 * 8, hipMemcpyDeviceToHost));
      auto& sets = q->distinct_values[d];
      for (uint64_t sl = 0; sl < cap; ++sl) {
        uint64_t ident = host[sl], value = host[cap + sl], flags = host[2 * cap + sl];
        if (ident == ~0ull || value == ~0ull || flags == ~0ull) continue;
        uint64_t second;
        if (hashed) {
          // (a value of 2^64-1 is stored as 2^64-2 with the flags word scrambled: such
          // a group is found under the unscrambled second identity word)
          second = flags;
          if (value == ~0ull - 1 && !sets.count({ident, second})) {
            const uint64_t alt = flags ^ 0xc2b2ae3d27d4eb4full;
            bool known = false;
            for (uint64_t g = 0; g < n && !known; ++g) {
              const uint64_t* rec = &q->records[g * (nwords + 1)];
              known = rec[1] == ident && rec[2] == alt;
            }
            if (known) {
              second = alt;
              value = ~0ull;
            }
          }
        } else {
          if (flags & 2u) ident = ~0ull;
          if (flags & 4u) value = ~0ull;
          second = flags & 1u;  // NULL key
        }
        sets[{ident, second}].push_back(value);
      }
      for (auto& kv : sets) std::sort(kv.second.begin(), kv.second.end());
    }
  }
  return Status();
}

static Status fetch_results(evql_query* q) {
  const KernelPlan& kp = q->rplan();
  FetchedRecords r;
  Status st;
  const uint64_t want = q->offset + q->limit;
  // the eager step tail: every group of the table is in the pinned block already (not after
  // a merge, an import or a recount -- they clear tail_valid --, and not where ORDER BY ..
  // LIMIT, set after the launch, selects its records on the device)
  const bool from_block = q->tail_valid && !q->merged &&
                          !(!q->order.empty() && q->has_limit && want < q->stats.num_groups);
  if (from_block) {
    r.nwords = uint32_t(kp.words_per_slot());
    r.n = r.total = q->stats.num_groups;
  } else {
    st = collect_records(q, &r);
    if (!st.ok()) return st;
    if (r.n && !q->order.empty() && q->has_limit && want < r.n) {
      st = select_top_records(q, want, &r);
      if (!st.ok()) return st;
    }
  }
  // step 2b: ORDER BY over a large result is sorted, and OFFSET / LIMIT cut, on the device
  q->order_applied = false;
  q->ostats = evql_order_stats_t{};
  q->ostats.records = r.n;
  {
    uint64_t lo, hi;
    limit_slice(q, r.n, &lo, &hi);
    q->ostats.rows = hi - lo;
    OrderSortPlan oplan;
    q->ostats.decision = uint32_t(plan_order_sort(order_sort_input(q, r.n), &oplan));
    if (q->ostats.decision == OSORT_DEVICE && !from_block) {
      st = sort_on_device(q, oplan, &r);
      if (!st.ok()) return st;
      q->order_applied = q->ostats.sorted_on_device != 0;
    }
  }
  const bool ordered = q->order_applied;
  const uint64_t n = r.n;
  q->ngroups = n;
  q->rec_stride = r.nwords + 1;
  q->demit.active = false;
  q->estats = evql_emit_stats_t{};
  q->estats.partial = q->group_mode == EVQL_MODE_PARTIAL;
  q->estats.rows = n;
  EmitArgs ea{};
  PartialEmitPlan pplan;
  if (from_block) {
    // (plans that read first rows or count distinct values never arm the block)
    records_from_block(q, n, r.nwords);
    q->first_vals.clear();
    q->first_tags.clear();
    q->distinct_values.clear();
  } else if (n >= kDeviceEmitMinGroups && device_emit_columns(q, q->merged, &ea, ordered)) {
    st = emit_on_device(q, ea, r.d_rec, n, r.nwords);
    if (!st.ok()) return st;
    q->records.clear();
    q->distinct_values.clear();
  } else if (plan_partial_emit(partial_emit_input(q, n), &pplan) == PEMIT_DEVICE) {
    st = emit_partial_on_device(q, pplan, r.d_rec, n, r.nwords);
    if (!st.ok()) return st;
    q->records.clear();
    q->distinct_values.clear();
  } else {
    st = records_to_host(q, r.d_rec, n, r.nwords, ordered);
    if (!st.ok()) return st;
    q->first_vals.clear();
    q->first_tags.clear();
    if (kp.need_first_row && n) {
      st = q->merged ? first_rows_from_records(q, n, r.nwords) : first_rows_from_table(q, n, r.nwords);
      if (!st.ok()) return st;
    }
    st = fetch_distinct_sets(q, n, r.nwords);
    if (!st.ok()) return st;
  }
  q->estats.device_packed = q->demit.active;
  q->stats.num_groups = r.total;
  q->emit_pos = 0;
  q->executed = true;
  q->fetched = true;
  return Status();
}

// ---------------------------------------------------------------------------
// result emission: GroupByExpression::nextBatch (groupby.cc:187-220)
// ---------------------------------------------------------------------------
// EVQL_FLOAT_SUM_EXACT: (sum of high parts) * 2^31 + (sum of low parts) multiples of
// 2^e, rounded to nearest once
static double exact_sum_value(uint64_t hi, uint64_t lo, int e) {
  const __int128 total = (__int128(int64_t(hi)) << 31) + __int128(int64_t(lo));
  return std::ldexp(double(total), e);  // (int128 -> double rounds to nearest even)
}

static Value agg_value(const evql_query* q, const AggPlan& a, const uint64_t* st) {
  Value v;
  v.tag = 0;
  const uint64_t w0 = st[a.first_word];
  switch (a.fn) {
    case EVQL_AGG_COUNT:
    case EVQL_AGG_SUM_UINT64:
    case EVQL_AGG_COUNT_DISTINCT_UINT64:
      v.type = EVQL_T_UINT64;
      v.bits = w0;
      break;
    case EVQL_AGG_SUM_INT64:
      v.type = EVQL_T_INT64;
      v.bits = w0;
      break;
    case EVQL_AGG_SUM_FLOAT64:
      v.type = EVQL_T_FLOAT64;
      v.bits = w0;
      if (a.exact_index >= 0) {
        const double d = exact_sum_value(w0, st[a.first_word + 1], q->fsum_exp[a.exact_index]);
        memcpy(&v.bits, &d, 8);
      }
      break;
    case EVQL_AGG_MIN_UINT64:
    case EVQL_AGG_MAX_UINT64:
    case EVQL_AGG_MIN_INT64:
    case EVQL_AGG_MAX_INT64:
    case EVQL_AGG_MIN_FLOAT64:
    case EVQL_AGG_MAX_FLOAT64: {
      v.type = (a.fn <= EVQL_AGG_MAX_UINT64) ? EVQL_T_UINT64
               : (a.fn <= EVQL_AGG_MAX_INT64 ? EVQL_T_INT64 : EVQL_T_FLOAT64);
      const uint64_t cnt = st[a.first_word + 1];
      if (cnt == 0) {
        v.bits = 0;
        v.tag = EVQL_STAG_NULL;
      } else {
        v.bits = w0;
      }
      break;
    }
    default: {  // mean
      v.type = EVQL_T_FLOAT64;
      const uint64_t cnt = st[a.first_word + 1];
      if (cnt == 0) {
        v.bits = 0;
        v.tag = EVQL_STAG_NULL;
      } else {
        double sum, m;
        memcpy(&sum, &w0, 8);
        m = sum / double(cnt);
        memcpy(&v.bits, &m, 8);
      }
    }
  }
  (void) q;
  return v;
}

static void put_varuint(std::vector<uint8_t>* b, uint64_t v) {
  do {
    uint8_t x = v & 0x7f;
    v >>= 7;
    if (v) x |= 0x80;
    b->push_back(x);
  } while (v);
}

// instance_savestate of each aggregate: count / sum = LEB128 varuint
// (aggregate.cc:55-57,171-173,207-209); build-supplied: sum_float64 = 8 raw
// bytes, min/max/mean = varuint(non-null count) + 8 raw bytes
static void save_state(const evql_query* q, const AggPlan& a, const uint64_t* st,
                       std::vector<uint8_t>* out, const uint64_t* rec = nullptr) {
  const uint64_t w0 = st[a.first_word];
  if (a.fn == EVQL_AGG_COUNT_DISTINCT_UINT64) {
    // varuint size, then the values ascending (std::set order, aggregate.cc:111-117)
    static const std::vector<uint64_t> none;
    const std::vector<uint64_t>* vals = &none;
    if (rec && a.distinct_index >= 0 && size_t(a.distinct_index) < q->distinct_values.size()) {
      const uint64_t kind = rec[0];
      const uint64_t ident = kind == 1 ? ~0ull : (kind == 2 ? 0 : rec[1]);
      const uint64_t second = q->kp.key_mode == KEY_HASHED ? rec[2] : (kind == 2 ? 1 : 0);
      const auto& sets = q->distinct_values[a.distinct_index];
      auto hit = sets.find({q->kp.key_mode == KEY_NONE ? 0 : ident, second});
      if (hit != sets.end()) vals = &hit->second;
    }
    put_varuint(out, vals->size());
    for (uint64_t v : *vals) put_varuint(out, v);
    return;
  }
  const uint8_t* p = reinterpret_cast<const uint8_t*>(&w0);
  switch (a.fn) {
    case EVQL_AGG_COUNT:
    case EVQL_AGG_SUM_UINT64:
    case EVQL_AGG_SUM_INT64:
      put_varuint(out, w0);
      return;
    case EVQL_AGG_SUM_FLOAT64:
      if (a.exact_index >= 0) {  // the wire carries the rounded double
        const double d = exact_sum_value(w0, st[a.first_word + 1], q->fsum_exp[a.exact_index]);
        const uint8_t* pd = reinterpret_cast<const uint8_t*>(&d);
        out->insert(out->end(), pd, pd + 8);
        return;
      }
      out->insert(out->end(), p, p + 8);
      return;
    default: {
      // min / max / mean.  A group without a non-NULL value: the state word still holds the
      // operation's identity (min: all ones) -- on the wire an untouched state is 0
      const uint64_t cnt = st[a.first_word + 1];
      put_varuint(out, cnt);
      static const uint8_t zero[8] = {0};
      if (cnt == 0) {
        out->insert(out->end(), zero, zero + 8);
      } else {
        out->insert(out->end(), p, p + 8);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// ORDER BY .. LIMIT fused above the GROUP BY (orderby.cc:60-160, limit.cc:52-125)
// ---------------------------------------------------------------------------
Status query_set_order(evql_query* q, const evql_sort_spec_t* specs, uint32_t n, int64_t limit,
                       uint64_t offset) {
  if (q->kp.bare_scan) return bare_set_limit(q, n, limit, offset);
  if (q->group_mode == EVQL_MODE_PARTIAL) {
    return Status::error(EVQL_EARG, "ORDER BY / LIMIT above a partial aggregate");
  }
  if (n == 0 && limit < 0) {
    return Status::error(EVQL_EARG, "can't execute ORDER BY: no sort specs");  // orderby.cc:53
  }
  std::vector<LoweredProgram> order(n);
  std::vector<bool> desc(n);
  for (uint32_t i = 0; i < n; ++i) {
    bool unsup = false;
    std::string e = lower_program(specs[i].expr, &order[i], &unsup);
    if (!e.empty()) return Status::error(unsup ? EVQL_ENOTSUP : EVQL_EARG, e);
    if (order[i].is_aggregate) return Status::error(EVQL_EARG, "aggregate in ORDER BY");
    std::vector<uint32_t> ins;
    expr_inputs(order[i].call, &ins);
    for (uint32_t in : ins) {
      if (in >= q->select.size()) return Status::error(EVQL_EARG, "invalid input index");
    }
    switch (order[i].return_type) {  // there is no cmp#int64/bool;bool;
      case EVQL_T_UINT64: case EVQL_T_INT64: case EVQL_T_FLOAT64: case EVQL_T_TIMESTAMP64:
      case EVQL_T_STRING:
        break;
      default:
        return Status::error(EVQL_EARG, "no comparator for the sort expression's type");
    }
    desc[i] = specs[i].descending != 0;
  }
  OrderKeyArgs ok{};
  if (n > 0) {
    // (the classification is order_sort_plan.cc's: the device sort asks it of every spec)
    switch (classify_order_key(q->rplan(), q->select, q->select_agg_index, q->select_passthrough,
                               order[0], desc[0], &ok)) {
      case OKEY_RECORD:
        break;
      case OKEY_EXPRESSION:
        return Status::error(EVQL_ENOTSUP, "first sort expression is not a plain output column");
      case OKEY_EXACT_SUM:
        return Status::error(EVQL_ENOTSUP, "ORDER BY an exact float sum is not fused");
      default:
        return Status::error(EVQL_ENOTSUP,
                             "first sort expression cannot be read from a group record");
    }
  }
  q->order.swap(order);
  q->order_desc.swap(desc);
  q->has_limit = limit >= 0;
  q->limit = limit >= 0 ? uint64_t(limit) : 0;
  q->offset = offset;
  q->order_key = ok;
  q->fetched = false;
  q->order_applied = false;
  return Status();
}

// cmp#int64/X;X; (boolean.cc:81-180): payloads only
static int value_cmp(uint32_t type, const Value& a, const Value& b) {
  switch (type) {
    case EVQL_T_INT64: {
      const int64_t l = int64_t(a.bits), r = int64_t(b.bits);
      return l < r ? -1 : (l > r ? 1 : 0);
    }
    case EVQL_T_FLOAT64: {
      double l, r;
      memcpy(&l, &a.bits, 8);
      memcpy(&r, &b.bits, 8);
      return l < r ? -1 : (l > r ? 1 : 0);
    }
    case EVQL_T_STRING: {
      const size_t m = std::min(a.str.size(), b.str.size());
      const int c = m ? strncmp(a.str.data(), b.str.data(), m) : 0;
      if (c != 0) return c < 0 ? -1 : 1;
      return a.str.size() < b.str.size() ? -1 : (a.str.size() > b.str.size() ? 1 : 0);
    }
    default:
      return a.bits < b.bits ? -1 : (a.bits > b.bits ? 1 : 0);
  }
}

// The scan select list of fetched group g: the scan columns of the group's first row as
// Values (`scan_vals`, scratch), then every scan select expression over them.  Plans without
// a first row leave `sel_inputs` as it is; their select expressions read no inputs.
static Status group_select_inputs(const evql_query* q, uint64_t g, std::vector<Value>* scan_vals,
                                  std::vector<Value>* sel_inputs) {
  const KernelPlan& kp = q->rplan();
  const uint32_t nc = uint32_t(kp.cols.size());
  scan_vals->resize(nc);
  sel_inputs->resize(q->scan_select.size());
  if (!kp.need_first_row) return Status();
  for (uint32_t c = 0; c < nc; ++c) {
    const ColAccess& ca = kp.cols[c];
    Value v;
    v.type = ca.stype;
    v.tag = q->first_tags[uint64_t(c) * q->ngroups + g];
    const uint64_t raw = q->first_vals[uint64_t(c) * q->ngroups + g];
    if (ca.string_hash) {
      if (!v.tag) {
        const uint64_t off = q->first_str_off[uint64_t(c) * q->ngroups + g];
        v.str.assign(reinterpret_cast<const char*>(q->first_str_heap.data()) + off,
                     size_t(raw >> 40));
        // A cell of the Dremel scan is a boxed SValue (CSTableScan.cc:300-330): a string
        // of 11 bytes is exactly the 16 bytes of the inline buffer, whose last byte --
        // the value's tag -- also holds STAG_INLINE (svalue.cc:346-368).  X_INPUT copies
        // the bytes as they lie, so the tag 0x80 reaches the group key's SHA1
        // (PartialGroupBy keys) and the output vectors.  Found by the round-3 soak.
        if (q->nested && v.str.size() == 11) v.tag = 0x80;
      }
    } else if (ca.stype == EVQL_T_FLOAT64 && ca.from_uint_to_float) {
      double d = double(raw);
      memcpy(&v.bits, &d, 8);
    } else if (ca.stype == EVQL_T_BOOL) {
      v.bits = raw != 0;
    } else {
      v.bits = raw;
    }
    (*scan_vals)[c] = v;
  }
  for (size_t j = 0; j < q->scan_select.size(); ++j) {
    std::string e = eval_expr(q->scan_select[j].call, *scan_vals, nullptr, &(*sel_inputs)[j]);
    if (!e.empty()) return Status::error(EVQL_ERUNTIME, e);
  }
  return Status();
}

// value of select expression i of fetched record `rec` as EVQL_MODE_FINAL emits it: an
// expression over the group's aggregate, the group key itself, or an expression over the
// scan select list (`inputs`)
static Status select_value(const evql_query* q, size_t i, const uint64_t* rec,
                           const std::vector<Value>& inputs, Value* out) {
  const KernelPlan& kp = q->rplan();
  const LoweredProgram& lp = q->select[i];
  std::string e;
  if (lp.is_aggregate) {
    Value av = agg_value(q, kp.aggs[q->select_agg_index[i]], rec + 1 + kp.state_word_base());
    e = eval_expr(lp.call, inputs, &av, out);
  } else if (q->select_passthrough[i]) {
    bool null_key;
    out->bits = cell_bits(ResultCell(), rec, nullptr, nullptr, 0, 0, &null_key);  // (kind 0: the key)
    out->tag = null_key ? uint8_t(EVQL_STAG_NULL) : uint8_t(0);
  } else {
    e = eval_expr(lp.call, inputs, nullptr, out);
  }
  if (!e.empty()) return Status::error(EVQL_ERUNTIME, e);
  out->type = lp.return_type;
  return Status();
}

// the select-list values of fetched record g (EVQL_MODE_FINAL), as query_next_batch emits
// them; ORDER BY evaluates its sort expressions over these
static Status final_row_values(evql_query* q, uint64_t g, std::vector<Value>* outs) {
  std::vector<Value> scan_vals, sel_inputs;
  Status st = group_select_inputs(q, g, &scan_vals, &sel_inputs);
  if (!st.ok()) return st;
  const std::vector<Value> none;
  const std::vector<Value>& inputs = q->rplan().need_first_row ? sel_inputs : none;
  outs->assign(q->select.size(), Value());
  for (size_t i = 0; i < outs->size(); ++i) {
    st = select_value(q, i, &q->records[g * q->rec_stride], inputs, &(*outs)[i]);
    if (!st.ok()) return st;
  }
  return Status();
}

// orders the fetched records by every sort spec and applies OFFSET / LIMIT
static Status order_fetched(evql_query* q) {
  const uint64_t n = q->ngroups;
  q->emit_order.clear();
  if (q->order.empty() && !q->has_limit) return Status();
  std::vector<uint64_t> idx(n);
  for (uint64_t i = 0; i < n; ++i) idx[i] = i;
  if (!q->order.empty()) {
    const size_t ns = q->order.size();
    std::vector<Value> keys(n * ns), row;
    for (uint64_t g = 0; g < n; ++g) {
      Status st = final_row_values(q, g, &row);
      if (!st.ok()) return st;
      for (size_t j = 0; j < ns; ++j) {
        std::string e = eval_expr(q->order[j].call, row, nullptr, &keys[g * ns + j]);
        if (!e.empty()) return Status::error(EVQL_ERUNTIME, e);
      }
    }
    std::stable_sort(idx.begin(), idx.end(), [&](uint64_t a, uint64_t b) {
      for (size_t j = 0; j < ns; ++j) {
        const int c = value_cmp(q->order[j].return_type, keys[a * ns + j], keys[b * ns + j]);
        if (c != 0) return q->order_desc[j] ? c > 0 : c < 0;
      }
      return false;
    });
  }
  uint64_t lo = 0, hi = n;
  if (q->has_limit) {
    lo = std::min(q->offset, n);
    hi = q->limit == 0 ? lo : std::min(n, q->offset + q->limit);
  }
  q->emit_order.assign(idx.begin() + lo, idx.begin() + hi);
  return Status();
}

// Select lists made of the group key and plain aggregate reads in EVQL_MODE_FINAL without
// ORDER BY / LIMIT -- what device_emit_columns recognises, less the first-row columns -- are
// packed straight from the fetched record words: no Value, no eval_expr, no vector per row.
// Everything else (post-aggregate arithmetic, exact sums, strings, PARTIAL rows) keeps the
// row loop of query_next_batch.
static bool direct_pack_columns(const evql_query* q, EmitArgs* ea) {
  if (q->eager_tail != evql_query::EAGER_ON) return false;
  // (with first rows the row loop also evaluates the scan select list, which can raise)
  if (q->rplan().need_first_row) return false;
  if (!device_emit_columns(q, q->merged, ea)) return false;
  for (uint32_t i = 0; i < ea->ncols; ++i) {
    if (ea->col[i].kind == 2) return false;
  }
  return true;
}

// byte for byte what select_value / agg_value + append_svector write for these columns
static void pack_direct(evql_query* q, const EmitArgs& ea, size_t max_rows, evql_column_buf_t* cols,
                        size_t* nrows) {
  const size_t rw = q->rec_stride;
  const uint64_t m = std::min<uint64_t>(q->ngroups - q->emit_pos, max_rows);
  const uint64_t* rec0 = m ? &q->records[q->emit_pos * rw] : nullptr;
  q->out_cols.resize(ea.ncols);
  for (uint32_t i = 0; i < ea.ncols; ++i) {
    const EmitCol& e = ea.col[i];
    std::vector<uint8_t>& out = q->out_cols[i];
    out.resize(size_t(m) * e.elem);  // (keeps its capacity from batch to batch)
    uint8_t* p = out.data();
    for (uint64_t g = 0; g < m; ++g, p += e.elem) {
      // (no first-row cell gets here: direct_pack_columns)
      bool null;
      const uint64_t bits = cell_bits(e, rec0 + g * rw, nullptr, nullptr, 0, 0, &null);
      const uint8_t tag = null ? uint8_t(EVQL_STAG_NULL) : uint8_t(0);
      if (e.elem == 2) {
        p[0] = bits ? 1 : 0;
        p[1] = tag;
      } else {
        memcpy(p, &bits, 8);
        p[8] = tag;
      }
    }
    cols[i].data = out.data();
    cols[i].size = out.size();
  }
  q->emit_pos += m;
  *nrows = size_t(m);
}

Status query_next_batch(evql_query* q, size_t max_rows, evql_column_buf_t* cols, size_t* nrows) {
  if (q->kp.bare_scan) return bare_next_batch(q, max_rows, cols, nrows);
  if (!q->executed) return Status::error(EVQL_EARG, "execute() was not called");
  if (!q->fetched) {
    Status st = fetch_results(q);
    if (!st.ok()) return st;
    // (sort_on_device left the records as the ordered slice already)
    if (q->order_applied) {
      q->emit_order.clear();
    } else {
      st = order_fetched(q);
      if (!st.ok()) return st;
    }
  }
  if (q->demit.active) {
    // slices of the columns packed on the device (emit_on_device)
    const evql_query::DeviceEmit& de = q->demit;
    const uint64_t left = q->ngroups - q->emit_pos;
    const uint64_t m = std::min<uint64_t>(left, max_rows);
    for (size_t i = 0; i < de.col.size(); ++i) {
      if (de.elem[i]) {
        cols[i].data = de.col[i] + q->emit_pos * de.elem[i];
        cols[i].size = size_t(m) * de.elem[i];
      } else {
        const uint64_t b0 = de.off[i][q->emit_pos], b1 = de.off[i][q->emit_pos + m];
        cols[i].data = de.col[i] + b0;
        cols[i].size = size_t(b1 - b0);
      }
    }
    q->emit_pos += m;
    *nrows = size_t(m);
    return Status();
  }
  {
    EmitArgs ea{};
    if (direct_pack_columns(q, &ea)) {
      pack_direct(q, ea, max_rows, cols, nrows);
      return Status();
    }
  }
  const KernelPlan& kp = q->rplan();
  const size_t nsel = q->select.size();
  const bool partial = q->group_mode == EVQL_MODE_PARTIAL;
  q->out_cols.assign(partial ? 2 : nsel, std::vector<uint8_t>());
  const size_t rw = q->rec_stride;
  size_t emitted = 0;
  std::vector<Value> scan_vals, sel_inputs;
  const std::vector<Value> none;
  const bool reordered = !q->order_applied && (!q->order.empty() || q->has_limit);
  const uint64_t emit_total = reordered ? q->emit_order.size() : q->ngroups;
  while (q->emit_pos < emit_total && emitted < max_rows) {
    const uint64_t g = reordered ? q->emit_order[q->emit_pos] : q->emit_pos;
    const uint64_t* rec = &q->records[g * rw];
    const uint64_t kind = rec[0], ident = rec[1];
    const uint64_t* st = rec + 1 + kp.state_word_base();
    Status sti = group_select_inputs(q, g, &scan_vals, &sel_inputs);
    if (!sti.ok()) return sti;
    const std::vector<Value>& inputs = kp.need_first_row ? sel_inputs : none;
    std::vector<uint8_t> pdata;  // PARTIAL mode: concatenated saved states
    for (size_t i = 0; i < nsel; ++i) {
      const LoweredProgram& lp = q->select[i];
      Value out;
      if (partial && lp.is_aggregate) {
        save_state(q, kp.aggs[q->select_agg_index[i]], st, &pdata, rec);
        continue;
      }
      Status stv = select_value(q, i, rec, inputs, &out);
      if (!stv.ok()) return stv;
      if (partial) {
        // SValue::encode (svalue.cc): u8 type, lenenc(value || tag bytes)
        std::vector<uint8_t> enc;
        append_svector(lp.return_type, out, &enc);
        // A reference quirk kept for byte-identical wire rows: the value is boxed in an
        // SValue whose 16-byte inline buffer ends in its tag byte, where setData also keeps
        // the internal STAG_INLINE flag (svalue.cc:346-368).  A value of exactly 16 bytes --
        // a string of 11 -- therefore leaves with bit 7 set in its tag.
        if (enc.size() == 16) enc.back() |= 0x80;
        pdata.push_back(uint8_t(lp.return_type));
        put_varuint(&pdata, enc.size());
        pdata.insert(pdata.end(), enc.begin(), enc.end());
      } else {
        append_svector(lp.return_type, out, &q->out_cols[i]);
      }
    }
    if (partial) {
      // group key = SHA1 of the tuple bytes, LAST group expression first
      // (groupby.cc:112-135: the VM stack grows downward)
      std::vector<uint8_t> tuple;
      for (size_t gi = q->group.size(); gi-- > 0;) {
        Value gv;
        if (kp.key_mode == KEY_EXACT) {
          gv.type = q->group[gi].return_type;
          gv.bits = kind == 2 ? 0 : ident;
          gv.tag = kind == 2 ? EVQL_STAG_NULL : 0;
        } else {
          std::string e = eval_expr(q->group[gi].call, sel_inputs, nullptr, &gv);
          if (!e.empty()) return Status::error(EVQL_ERUNTIME, e);
        }
        append_svector(q->group[gi].return_type, gv, &tuple);
      }
      Sha1Digest d = sha1(tuple.data(), tuple.size());
      Value kv, dv;
      kv.str.assign(reinterpret_cast<const char*>(d.bytes), 20);
      dv.str.assign(reinterpret_cast<const char*>(pdata.data()), pdata.size());
      append_svector(EVQL_T_STRING, kv, &q->out_cols[0]);
      append_svector(EVQL_T_STRING, dv, &q->out_cols[1]);
    }
    ++q->emit_pos;
    ++emitted;
  }
  for (size_t i = 0; i < q->out_cols.size(); ++i) {
    cols[i].data = q->out_cols[i].data();
    cols[i].size = q->out_cols[i].size();
  }
  *nrows = emitted;
  return Status();
}

}  // namespace evql
