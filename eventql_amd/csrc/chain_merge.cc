// chain_merge.cc -- chains: the tables of one partition scanned by one operator each
// (evql_query_create_chain).
//
// PartitionCursor hands the batches of its scans to ONE GroupByExpression, newest table
// first (server/sql/partition_cursor.cc:56-81, groupby.cc:69-185).  Here every table was
// aggregated by its own launch; their groups are merged like the partial aggregates of
// several ranks (exchange.cc) -- table i plays rank i: records in chain order into a fresh
// table, first rows resolved inside the table that produced them, (table << 44 | row) as the
// scan position, string bytes into one heap, count_distinct pairs re-inserted into one set.
#include "runtime.h"

namespace evql {
namespace {

// the buffers of the per-table loop (sized for the largest table; sizes / heap per table)
struct ChainBuffers {
  DevBuf<uint64_t> d_rec, d_wire, d_sizes;
  DevBuf<RtColumn> d_cols;
  DevBuf<uint8_t> d_heap;
};

// table `pi` of the chain: records -> wire form -> merge
Status merge_table(evql_query* head, evql_query* q, size_t pi, const GroupRecordLayout& L,
                   MergeResolvedArgs& ma, ChainBuffers& b) {
  hipStream_t s = head->ctx->stream;
  const uint64_t n = q->ngroups;
  if (n == 0) return Status();
  RecordsView view;
  Status st = query_records_view(q, &view);
  if (st.ok()) st = query_dense_records(q, L, view, b.d_rec);
  if (!st.ok()) return st;
  if (!L.resolved) {
    HIP_TRY(launch_table_merge(ma.m, b.d_rec, n, s));
    return Status();
  }
  std::vector<RtColumn> rc;
  st = resolve_first_rows(q, L, uint64_t(pi) << 44, &rc, b.d_cols, b.d_rec, n, b.d_wire);
  if (!st.ok()) return st;
  const uint64_t seg[2] = {0, n};  // (one segment)
  uint64_t segoff[2] = {0, 0};
  if (!L.str_cols.empty()) {
    HIP_TRY(b.d_sizes.alloc((n + 4) * 8));
    auto heap_for = [&](uint64_t bytes) {
      return b.d_heap.alloc(bytes + 16) == hipSuccess ? b.d_heap.p : nullptr;
    };
    st = wire_strings(q, L, nullptr, b.d_wire, n, seg, 1, b.d_sizes, b.d_sizes.p + n + 2, heap_for,
                      segoff);
    if (!st.ok()) return st;
  }
  const uint64_t heap_bytes = segoff[1];
  ma.heap_base = head->m_heap.size();
  HIP_TRY(launch_table_merge_resolved(ma, b.d_wire, n, s));
  HIP_TRY(hipStreamSynchronize(s));  // (rc lives until here)
  if (!heap_bytes) return Status();
  // the strings behind the head's heap: on the device (an exchange of this head exports them
  // from there) and on the host
  const size_t old = head->m_heap.size();
  if (old + heap_bytes > head->mheap_cap) {
    const uint64_t want = std::max<uint64_t>(2 * head->mheap_cap, old + heap_bytes + 4096);
    DevBuf<uint8_t> grown;
    HIP_TRY(grown.alloc(want));
    if (old) HIP_TRY(hipMemcpyAsync(grown, head->d_mheap, old, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    head->d_mheap = std::move(grown);
    head->mheap_cap = want;
  }
  HIP_TRY(hipMemcpyAsync(head->d_mheap.p + old, b.d_heap, heap_bytes, hipMemcpyDeviceToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));  // (d_heap is allocated anew for the next table)
  head->m_heap.resize(old + heap_bytes);
  HIP_TRY(hipMemcpy(head->m_heap.data() + old, b.d_heap, heap_bytes, hipMemcpyDeviceToHost));
  return Status();
}

// count_distinct: the union of the tables' pair sets
Status merge_pairsets(evql_query* head, const std::vector<evql_query*>& parts,
                      const GroupRecordLayout& L) {
  hipStream_t s = head->ctx->stream;
  const KernelPlan& kp = head->rplan();
  const size_t np_ = parts.size();
  std::vector<uint64_t> counts(size_t(kp.n_distinct) * np_, 0), tots(kp.n_distinct, 0);
  uint64_t max_total = 0;
  for (int d = 0; d < kp.n_distinct; ++d) {
    uint64_t& tot = tots[d];
    for (size_t pi = 0; pi < np_; ++pi) {
      evql_query* q = parts[pi];
      if (!q->d_pairset[d]) continue;
      Status st = pairset_count(q, q->d_pairset[d], q->pairset_cap, &counts[size_t(d) * np_ + pi]);
      if (!st.ok()) return st;
      tot += counts[size_t(d) * np_ + pi];
    }
    max_total = std::max(max_total, tot);
  }
  uint64_t set_cap = 1 << 16;
  while (set_cap < max_total * 2) set_cap <<= 1;
  for (const auto& ag : kp.aggs) {
    if (ag.distinct_index < 0) continue;
    const int d = ag.distinct_index;
    const uint64_t tot = tots[d];
    DevBuf<uint64_t> d_tr;
    HIP_TRY(d_tr.alloc(std::max<uint64_t>(tot, 1) * 24));
    uint64_t off = 0;
    for (size_t pi = 0; pi < np_; ++pi) {
      evql_query* q = parts[pi];
      const uint64_t np = counts[size_t(d) * np_ + pi];
      if (!np) continue;
      uint64_t* d_cnt = q->d_counters + kScratchCounter;
      HIP_TRY(hipMemsetAsync(d_cnt, 0, 8, s));
      HIP_TRY(launch_pairset_export(q->d_pairset[d], q->pairset_cap, d_tr.p + off * 3, np, d_cnt, s));
      off += np;
    }
    // (PARTIAL emission reads the values of every group from the merged set, fetch_results)
    Status st = merged_set_fill(head, L, d, set_cap, uint32_t(kp.state_word_base() + ag.first_word),
                                d_tr, tot);
    if (!st.ok()) return st;
    HIP_TRY(hipStreamSynchronize(s));  // (d_tr lives until here)
  }
  return Status();
}

}  // namespace

Status chain_merge(evql_query* head) {
  hipStream_t s = head->ctx->stream;
  const KernelPlan& kp = head->rplan();
  std::vector<evql_query*> parts;
  parts.push_back(head);
  for (evql_query* c : head->chain) parts.push_back(c);
  const GroupRecordLayout L = group_record_layout(kp);
  // (the string-column limit used to be met at the first table with groups, behind the checks
  // below and a re-initialised d_mtab: now it is answered first, whatever the tables hold)
  Status st = group_record_layout_check(L, "a chain");
  if (!st.ok()) return st;
  if (parts.size() >= (1u << 19)) return Status::error(EVQL_EARG, "too many tables in a chain");
  uint64_t total = 0, max_n = 0;
  for (evql_query* p : parts) {
    // (same plan everywhere: the slot layouts agree; a table whose string key has no usable
    // dictionary keeps the hashed plan, its records have the coded tables' rplan() layout)
    if (uint32_t(p->rplan().words_per_slot()) != L.W || p->rplan().cols.size() != L.nc ||
        p->rplan().key_mode != kp.key_mode || p->rplan().need_first_row != kp.need_first_row) {
      return Status::error(EVQL_ERUNTIME, "chain: the tables' plans disagree");
    }
    if (!p->executed) return Status::error(EVQL_EARG, "execute() was not called");
    total += p->ngroups;
    max_n = std::max(max_n, p->ngroups);
  }
  MergeResolvedArgs ma;
  st = merged_table_prepare(head, L, total, &ma);
  if (!st.ok()) return st;
  HIP_TRY(hipMemsetAsync(head->d_status, 0, 16, s));
  ChainBuffers b;
  HIP_TRY(b.d_rec.alloc(std::max<uint64_t>(max_n, 1) * L.rw_in * 8));
  if (L.resolved) {
    HIP_TRY(b.d_wire.alloc(std::max<uint64_t>(max_n, 1) * L.rw * 8));
    HIP_TRY(b.d_cols.alloc(std::max<uint32_t>(L.nc, 1) * sizeof(RtColumn)));
  }
  head->m_heap.clear();
  uint64_t rows_scanned = 0, rows_passed = 0;
  double kernel_ms = 0;
  for (size_t pi = 0; pi < parts.size(); ++pi) {
    rows_scanned += parts[pi]->stats.rows_scanned;
    rows_passed += parts[pi]->stats.rows_passed;
    kernel_ms += parts[pi]->stats.kernel_ms;
    st = merge_table(head, parts[pi], pi, L, ma, b);
    if (!st.ok()) return st;
  }
  if (head->m_heap.size() > kStrOffMask) {
    return Status::error(EVQL_ENOTSUP, "chain: first-row strings exceed the offset range");
  }
  if (kp.n_distinct > 0) {
    st = merge_pairsets(head, parts, L);
    if (!st.ok()) return st;
  }
  uint32_t status[4] = {0};
  HIP_TRY(hipMemcpyAsync(status, head->d_status, 16, hipMemcpyDeviceToHost, s));
  uint64_t ng = 0;
  HIP_TRY(hipMemcpyAsync(&ng, ma.m.fresh, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  st = merge_status_error(status[0], "merged ");
  if (!st.ok()) return st;
  head->merged = true;
  head->chain_merged = true;
  head->ngroups = ng;
  head->stats.num_groups = ng;
  head->stats.rows_scanned = rows_scanned;
  head->stats.rows_passed = rows_passed;
  head->stats.kernel_ms = kernel_ms;
  head->stats.total_ms = kernel_ms;
  head->fetched = false;
  head->order_applied = false;
  head->tail_valid = false;
  head->emit_pos = 0;
  return Status();
}

}  // namespace evql
