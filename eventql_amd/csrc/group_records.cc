// group_records.cc -- groups that leave the scan that produced them: what the exchange, the
// chain merge and the group imports share.  Raw device pointers: the callers own their buffers.
#include "runtime.h"

namespace evql {

GroupRecordLayout group_record_layout(const KernelPlan& kp) {
  GroupRecordLayout L;
  L.W = uint32_t(kp.words_per_slot());
  L.nc = uint32_t(kp.cols.size());
  L.resolved = kp.need_first_row;
  L.rw_in = L.W + 1;
  L.rw = L.resolved ? L.rw_in + L.nc + 1 : L.rw_in;
  L.mw = L.resolved ? L.W + L.nc + 1 : L.W;
  for (uint32_t c = 0; L.resolved && c < L.nc; ++c) {
    if (kp.cols[c].string_hash) {
      L.str_mask |= 1ull << c;
      L.str_cols.push_back(c);
    }
  }
  if (L.resolved) L.first_row_word = uint32_t(kp.first_row_word());
  L.has_ident2 = kp.has_ident2() ? 1 : 0;
  return L;
}

Status group_record_layout_check(const GroupRecordLayout& L, const char* plan_kind) {
  if (L.mw > uint32_t(kMaxStateWords + 3)) {
    return Status::error(EVQL_ENOTSUP, "too many words per merged group");
  }
  if (L.str_cols.size() > kMaxWireStrCols) {
    return Status::error(EVQL_ENOTSUP, std::string("too many string columns in ") + plan_kind + " plan");
  }
  return Status();
}

void slot_identities(const KernelPlan& kp, uint32_t nwords, uint64_t* out) {
  // the host's one op -> identity mapping, by EVQL_OP_* (device side: evql_device.h)
  static const uint64_t kIdentity[8] = {0, 0, 0xFFFFFFFFFFFFFFFFull, 0, 0x7FFFFFFFFFFFFFFFull,
                                        0x8000000000000000ull, 0x7FF0000000000000ull,
                                        0xFFF0000000000000ull};
  uint32_t w = 0;
  out[w++] = 0xFFFFFFFFFFFFFFFFull;
  if (kp.has_ident2()) out[w++] = 0xFFFFFFFFFFFFFFFFull;
  if (kp.need_first_row) out[w++] = 0xFFFFFFFFFFFFFFFFull;
  for (const auto& sw : kp.states) out[w++] = sw.op >= 0 && sw.op < 8 ? kIdentity[sw.op] : 0;
  for (; w < nwords; ++w) out[w] = 0;  // (first-row value words of a merged slot)
}

void merge_ops(const KernelPlan& kp, bool skip_distinct, MergeArgs* a) {
  a->nwords = uint32_t(kp.words_per_slot());
  a->has_ident2 = kp.has_ident2() ? 1 : 0;
  int w = 1;
  if (kp.has_ident2()) a->ops[w++] = 255;  // (an identity word: never combined)
  if (kp.need_first_row) a->ops[w++] = 2;  // min
  for (const auto& sw : kp.states) a->ops[w++] = uint32_t(sw.op);
  for (const auto& ag : kp.aggs) {
    if (skip_distinct && ag.distinct_index >= 0) a->ops[kp.state_word_base() + ag.first_word] = kMergeSkip;
  }
}

// A flat table: the narrow copy / the decoded SoA words / the pages, as the plan reads them.
// A nested scan: its first rows are FLATTENED rows, so the sources are the operator's own
// per-row arrays -- the 8-byte words of nested_flat (strings: nested_strpos), or the narrow
// copy of a column that has one.  The two hold the same values: query_prepare (query_run.cc,
// the nested_packed loop) makes narrow copies only of operators without a mixed-depth WHERE
// (!nested_where_mixed), the only ones whose flattened words are rewritten per query
// (apply_where_resets); everywhere else the narrow array was packed from those very words.
Status first_row_columns(evql_query* q, std::vector<RtColumn>* out) {
  evql_table* t = q->table;
  const KernelPlan& kp = q->rplan();
  const uint32_t nc = uint32_t(kp.cols.size());
  out->assign(nc, RtColumn{});
  for (uint32_t c = 0; c < nc; ++c) {
    const ColAccess& ca = kp.cols[c];
    RtColumn& rc = (*out)[c];
    rc.pages = ca.layout_index >= 0 ? t->d_pages[ca.layout_index][0] : nullptr;
    rc.mode = ca.mode;
    rc.bits = ca.bits;
    if (ca.mode == ColAccess::NARROW_F32) {
      // a float32 copy serves the tile loads only: a single row comes from the file's pages
      rc.mode = ColAccess::PLAIN64;
      rc.bits = 0;
      continue;
    }
    if (q->nested) {
      if (ca.packed) {
        rc.pages = nullptr;
        rc.base = q->nested_packed[c].base;
      }
      rc.soa = ca.string_hash ? q->nested_strpos[c] : q->nested_flat[c];
    } else if (ca.packed || ca.mode == ColAccess::SOA) {
      auto hit = t->materialized.find(ca.name);  // (query_prepare made it)
      if (hit == t->materialized.end()) {
        return Status::error(EVQL_ERUNTIME, "first rows: column " + ca.name + " was not materialised");
      }
      const MaterializedColumn& m = hit->second;
      if (ca.packed) {
        rc.pages = nullptr;  // (a flat array: ColAccess::NARROW)
        rc.base = m.d_packed;
      } else {
        // strings: (len << 40 | position); their bytes are copied out by the caller
        rc.soa = ca.string_hash ? m.d_strpos : m.d_values;
        rc.tags = m.d_tags;
      }
    }
  }
  return Status();
}

Status resolve_first_rows(evql_query* q, const GroupRecordLayout& L, uint64_t rank_tag,
                          std::vector<RtColumn>* rc, RtColumn* d_cols, const uint64_t* in, uint64_t n,
                          uint64_t* out) {
  hipStream_t s = q->ctx->stream;
  Status st = first_row_columns(q, rc);
  if (!st.ok()) return st;
  HIP_TRY(hipMemcpyAsync(d_cols, rc->data(), L.nc * sizeof(RtColumn), hipMemcpyHostToDevice, s));
  ResolveArgs ra{};
  ra.image = q->table->d_image;
  ra.cols = d_cols;
  ra.ncols = L.nc;
  ra.in_words = L.rw_in;
  ra.first_row_word = 1 + L.first_row_word;
  ra.rank_tag = rank_tag;
  ra.in = in;
  ra.n = n;
  ra.out = out;
  HIP_TRY(launch_resolve_records(ra, s));
  return Status();
}

Status query_dense_records(evql_query* q, const GroupRecordLayout& L, const RecordsView& view,
                           uint64_t* dst) {
  hipStream_t s = q->ctx->stream;
  const uint64_t n = q->ngroups, nd = view.nd;
  if (nd) HIP_TRY(hipMemcpyAsync(dst, view.dense, nd * L.rw_in * 8, hipMemcpyDeviceToDevice, s));
  if (n > nd) {
    uint64_t* d_cnt = q->d_counters + kScratchCounter;
    HIP_TRY(hipMemsetAsync(d_cnt, 0, 8, s));
    HIP_TRY(launch_table_compact(q->d_gtab, q->gcap, q->gcap + 8, L.W, dst + nd * L.rw_in, n - nd,
                                 d_cnt, s));
  }
  return Status();
}

Status pairset_count(evql_query* q, const uint64_t* set, uint64_t cap, uint64_t* n) {
  hipStream_t s = q->ctx->stream;
  uint64_t* d_cnt = q->d_counters + kScratchCounter;
  HIP_TRY(hipMemsetAsync(d_cnt, 0, 8, s));
  if (set) HIP_TRY(launch_pairset_export(set, cap, nullptr, 0, d_cnt, s));
  HIP_TRY(hipMemcpyAsync(n, d_cnt, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return Status();
}

Status merged_table_prepare(evql_query* q, const GroupRecordLayout& L, uint64_t total_records,
                            MergeResolvedArgs* ma) {
  hipStream_t s = q->ctx->stream;
  uint64_t cap = 1 << 16;
  while (cap < total_records * 2) cap <<= 1;
  if (!q->d_mtab || q->mcap != cap || q->m_words != L.mw) {
    if (q->d_mtab) hipFree(q->d_mtab);
    q->d_mtab = nullptr;
    q->mcap = 0;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&q->d_mtab), (cap + 8) * uint64_t(L.mw) * 8));
  }
  q->mcap = cap;
  q->m_words = L.mw;
  TableInitArgs ia{};
  ia.words = q->d_mtab;
  ia.stride = cap + 8;
  ia.nwords = L.mw;
  slot_identities(q->rplan(), L.mw, ia.identity);
  HIP_TRY(launch_table_init(ia, s));
  *ma = MergeResolvedArgs{};
  merge_ops(q->rplan(), true, &ma->m);
  ma->m.nwords = L.mw;  // (the slots also carry the first-row value words)
  ma->m.words = q->d_mtab;
  ma->m.gcap = cap;
  ma->m.stride = cap + 8;
  ma->m.status = q->d_status;
  ma->state_words = L.W;
  ma->first_row_word = L.first_row_word;
  ma->ncols = L.nc;
  ma->str_mask = L.str_mask;
  // a batch is the groups of one rank / one table: pairwise different identities, so plain
  // read-modify-write behind the identity CAS, new slots counted as they are claimed
  ma->m.exclusive = 1;
  ma->m.fresh = q->d_counters + kFreshGroupCounter;
  HIP_TRY(hipMemsetAsync(ma->m.fresh, 0, 8, s));
  return Status();
}

Status merged_set_fill(evql_query* q, const GroupRecordLayout& L, int which, uint64_t cap,
                       uint32_t word, const uint64_t* d_triples, uint64_t n) {
  hipStream_t s = q->ctx->stream;
  if (q->d_mset[which] && q->mset_cap[which] != cap) {
    hipFree(q->d_mset[which]);
    q->d_mset[which] = nullptr;
    q->mset_cap[which] = 0;
  }
  if (!q->d_mset[which]) HIP_TRY(hipMalloc(reinterpret_cast<void**>(&q->d_mset[which]), cap * 24));
  q->mset_cap[which] = cap;
  HIP_TRY(hipMemsetAsync(q->d_mset[which], 0xff, cap * 24, s));
  PairsetMergeArgs pa{};
  pa.set = q->d_mset[which];
  pa.set_cap = cap;
  pa.words = q->d_mtab;
  pa.gcap = q->mcap;
  pa.nwords = L.mw;
  pa.word = word;
  pa.key_mode = uint32_t(q->rplan().key_mode);
  pa.status = q->d_status;
  HIP_TRY(launch_pairset_merge(pa, d_triples, n, s));
  return Status();
}

Status wire_strings(evql_query* q, const GroupRecordLayout& L, const uint8_t* flat, uint64_t* records,
                    uint64_t n, const uint64_t* seg, uint32_t nseg, uint64_t* d_sizes, uint64_t* d_seg,
                    const std::function<uint8_t*(uint64_t)>& heap_for, uint64_t* segoff) {
  hipStream_t s = q->ctx->stream;
  evql_table* t = q->table;
  WireStrArgs wa{};
  wa.image = t->d_image;
  wa.flat = flat;
  wa.records = records;
  wa.n = n;
  wa.rw = L.rw;
  wa.tags_word = L.rw_in + L.nc;
  wa.nstr = uint32_t(L.str_cols.size());
  for (size_t k = 0; k < L.str_cols.size(); ++k) {
    wa.word[k] = L.rw_in + L.str_cols[k];
    wa.col[k] = L.str_cols[k];
    if (!flat) wa.pages[k] = t->d_pages[q->rplan().cols[L.str_cols[k]].layout_index][0];
  }
  wa.sizes = d_sizes;
  wa.nranks = nseg;
  wa.starts = d_seg;
  HIP_TRY(hipMemcpyAsync(d_seg, seg, (nseg + 1) * 8, hipMemcpyHostToDevice, s));
  HIP_TRY(launch_wire_str_sizes(wa, s));
  HIP_TRY(launch_exclusive_scan(d_sizes, n, d_sizes + n, s));
  uint64_t heap_bytes = 0;
  HIP_TRY(hipMemcpyAsync(&heap_bytes, d_sizes + n, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));  // (`seg` lives until here)
  segoff[0] = 0;  // segment borders in bytes
  for (uint32_t r = 1; r <= nseg; ++r) {
    segoff[r] = heap_bytes;
    if (seg[r] < n) HIP_TRY(hipMemcpy(&segoff[r], d_sizes + seg[r], 8, hipMemcpyDeviceToHost));
  }
  wa.heap = heap_for(heap_bytes);
  if (!wa.heap) return Status::error(EVQL_EDEVICE, "hipMalloc of the string heap failed");
  HIP_TRY(launch_wire_str_copy(wa, s));
  return Status();
}

Status merge_status_error(uint32_t status, const char* what) {
  if (status & 2u) return Status::error(EVQL_ENOMEM, std::string(what) + "group table full");
  if (status & 8u) return Status::error(EVQL_ENOMEM, std::string(what) + "count_distinct set full");
  return Status();
}

}  // namespace evql
