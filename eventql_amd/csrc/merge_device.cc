// merge_device.cc -- GroupByMergeExpression for PartialGroupBy wire rows, on the device
// (evql_merge_create_device).
//
// The host merge (merge.cc) keeps one hash-map node and one vector per group and is fed row by
// row.  Here a frame is validated once on the host (merge_frame_index.cc), uploaded whole and
// decoded by one thread per row into fixed-width records [3 key words][cell words].  The
// records of the merged groups and, behind them, of the rows not yet folded ("pending", in
// arrival order) lie in one array.  A fold sorts (first key word, row) pairs with the stable
// radix passes of the sorted compaction, marks the group heads by comparing all 20 key bytes,
// and lets one thread per group fold its rows in order from the zero state -- the order and
// the arithmetic of the reference's mergeInstance loop, so float sums are bit-exact, and the
// last row of a group carries the non-aggregate values (groupby.cc:606-610).  The result has
// the layout of its input, so it is the next fold's first part.
#include "merge_device.h"
#include "radix_sort.h"
#include <chrono>
#include <cstdlib>
#include <cstring>

namespace evql {

namespace {
double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
uint64_t align8(uint64_t v) { return (v + 7) & ~7ull; }
static const uint64_t kMaxResidentRows = 0xffffffffull;
}  // namespace

struct MergeDevice {
  // (the context's device and stream, copied: destroying the merge does not touch the context,
  // which may be gone by then)
  int device = 0;
  hipStream_t s = nullptr;
  std::vector<LoweredProgram> select;
  MergeRecordLayout L;
  std::vector<uint32_t> str_cols;  // select expressions of class MCELL_STRING
  uint64_t pending_limit = 1ull << 24;
  // records: [0, ngroups) the merged groups, [ngroups, ngroups + npending) the pending rows
  DevBuf<uint64_t> rec;
  uint64_t rec_cap = 0, ngroups = 0, npending = 0;
  // uploaded payloads (and, in front of them, the merged groups' strings)
  DevBuf<uint8_t> arena;
  uint64_t arena_cap = 0, arena_used = 0;
  uint8_t* h_stage = nullptr;  // pinned
  size_t stage_cap = 0;
  bool stage_busy = false;     // an upload may still read h_stage
  evql_merge_stats_t st{};
  // iteration
  bool iterating = false;
  uint64_t pos = 0;
  std::vector<uint64_t> h_rec;    // host pack: the records
  std::vector<uint8_t> h_arena;   //            and their strings
  std::vector<std::vector<uint8_t>> packed;      // device pack: whole columns
  std::vector<std::vector<uint64_t>> packed_off; //   strings: n + 1 offsets
  std::vector<std::vector<uint64_t>> state_words; // computed aggregates: [state][count] words
  std::vector<std::vector<uint8_t>> out_cols;
  ~MergeDevice() {
    if (h_stage) hipHostFree(h_stage);
  }
};

namespace {

Status index_error(MergeIndexResult r, const char* malformed) {
  switch (r) {
    case MINDEX_MALFORMED: return Status::error(EVQL_EIO, malformed);
    case MINDEX_CELL_CLASS:
      return Status::error(EVQL_ENOTSUP, "device merge: a cell of another size class than its select expression");
    default: return Status::error(EVQL_ENOTSUP, "device merge: frame or string too large");
  }
}

Status grow_records(MergeDevice* d, uint64_t need) {
  if (need <= d->rec_cap) return Status();
  const uint64_t cap = std::max<uint64_t>(std::max(need, 2 * d->rec_cap), 1024);
  DevBuf<uint64_t> nb;
  HIP_TRY(nb.alloc(cap * d->L.rw * 8));
  const uint64_t live = d->ngroups + d->npending;
  if (live) HIP_TRY(hipMemcpyAsync(nb.p, d->rec.p, live * d->L.rw * 8, hipMemcpyDeviceToDevice, d->s));
  HIP_TRY(hipStreamSynchronize(d->s));
  d->stage_busy = false;
  d->rec = std::move(nb);
  d->rec_cap = cap;
  return Status();
}

Status grow_arena(MergeDevice* d, uint64_t need) {
  if (need <= d->arena_cap) return Status();
  const uint64_t cap = std::max<uint64_t>(std::max(need, 2 * d->arena_cap), 4096);
  DevBuf<uint8_t> nb;
  HIP_TRY(nb.alloc(cap));
  if (d->arena_used) HIP_TRY(hipMemcpyAsync(nb.p, d->arena.p, d->arena_used, hipMemcpyDeviceToDevice, d->s));
  HIP_TRY(hipStreamSynchronize(d->s));
  d->stage_busy = false;
  d->arena = std::move(nb);
  d->arena_cap = cap;
  return Status();
}

// the pinned staging block, free to be overwritten
Status stage_for(MergeDevice* d, size_t bytes) {
  if (d->stage_busy) {
    HIP_TRY(hipStreamSynchronize(d->s));
    d->stage_busy = false;
  }
  if (bytes <= d->stage_cap) return Status();
  if (d->h_stage) hipHostFree(d->h_stage);
  d->h_stage = nullptr;
  d->stage_cap = 0;
  const size_t cap = std::max(bytes, size_t(1) << 20);
  HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&d->h_stage), cap, hipHostMallocDefault));
  d->stage_cap = cap;
  return Status();
}

// Side 1 of the ping-pong holds the current order: every sort here runs an even number of
// passes, so it ends where it began.
struct SortScratch : RadixPassScratch {
  bool have_perm = false;
};

// a stable sort of the current order (the identity at first) by the low `bits` bits of record
// word `word`: the digit passes over gathered key words, kmin 0, no statistics
Status sort_by_word(MergeDevice* d, SortScratch* S, uint64_t n, uint32_t word, uint32_t bits) {
  const uint32_t passes = bits / 8;
  if (passes & 1) return Status::error(EVQL_ERUNTIME, "merge: an odd number of sort passes");
  const uint32_t* perm = S->have_perm ? S->idx[1].p : nullptr;
  HIP_TRY(launch_mrg_gather_key(d->rec, d->L.rw, word, perm, n, S->keys[1], d->s));
  Status st = radix_sort_passes(S->keys[1], perm, n, 0, passes, S, d->s);
  if (!st.ok()) return st;
  S->have_perm = S->have_perm || passes > 0;
  d->st.sort_passes += passes;
  return Status();
}

// folds the pending rows into the groups
Status compact(MergeDevice* d) {
  if (d->npending == 0) return Status();
  const auto t0 = std::chrono::steady_clock::now();
  const uint64_t n = d->ngroups + d->npending;
  const uint32_t rw = d->L.rw;
  SortScratch S;
  for (int b = 0; b < 2; ++b) {
    HIP_TRY(S.keys[b].alloc(n * 8));
    HIP_TRY(S.idx[b].alloc(n * 4));
  }
  HIP_TRY(S.hist.alloc(size_t(256) * ((n + kSortTile - 1) / kSortTile) * 4));
  HIP_TRY(S.totals.alloc(256 * 4));
  DevBuf<uint8_t> flags;
  DevBuf<uint64_t> heads, counters;
  HIP_TRY(flags.alloc(n));
  HIP_TRY(heads.alloc((n + 1) * 8));
  HIP_TRY(counters.alloc(8));
  uint64_t h_collisions = 0, h_groups = 0;
  for (int round = 0; round < 2; ++round) {
    Status st;
    if (round == 1) {
      // equal prefixes, different keys: the remaining 12 bytes as lower-order digits
      S.have_perm = false;
      st = sort_by_word(d, &S, n, 2, 32);
      if (st.ok()) st = sort_by_word(d, &S, n, 1, 64);
      ++d->st.full_key_sorts;
    }
    if (st.ok()) st = sort_by_word(d, &S, n, 0, 64);
    if (!st.ok()) return st;
    HIP_TRY(hipMemsetAsync(counters.p, 0, 8, d->s));
    HIP_TRY(launch_mrg_heads(d->rec, rw, S.idx[1], n, flags, heads, counters, d->s));
    HIP_TRY(launch_exclusive_scan(heads, n, heads.p + n, d->s));
    HIP_TRY(hipMemcpyAsync(&h_collisions, counters.p, 8, hipMemcpyDeviceToHost, d->s));
    HIP_TRY(hipMemcpyAsync(&h_groups, heads.p + n, 8, hipMemcpyDeviceToHost, d->s));
    HIP_TRY(hipStreamSynchronize(d->s));
    d->stage_busy = false;
    if (round == 0) d->st.prefix_collisions += h_collisions;
    if (h_collisions == 0) break;
  }
  if (h_groups == 0 || h_groups > n) return Status::error(EVQL_ERUNTIME, "device merge: group count out of range");
  DevBuf<uint64_t> out;
  HIP_TRY(out.alloc(h_groups * rw * 8));
  MrgFoldArgs fa{};
  fa.L = d->L;
  fa.records = d->rec;
  fa.perm = S.idx[1];
  fa.flags = flags;
  fa.seg = heads;
  fa.n = n;
  fa.out = out;
  fa.out_cap = h_groups;
  HIP_TRY(launch_mrg_fold(fa, d->s));
  DevBuf<uint8_t> new_arena;
  uint64_t new_arena_bytes = 0;
  if (!d->str_cols.empty()) {
    // the groups' strings into an arena of their own; the payloads go with the old one
    MrgStrArgs sa{};
    sa.records = out;
    sa.n = h_groups;
    sa.rw = rw;
    sa.nstr = uint32_t(d->str_cols.size());
    for (size_t x = 0; x < d->str_cols.size(); ++x) sa.word[x] = d->L.word[d->str_cols[x]];
    const uint64_t cells = h_groups * sa.nstr;
    DevBuf<uint64_t> sizes;
    HIP_TRY(sizes.alloc((cells + 1) * 8));
    sa.sizes = sizes;
    sa.src = d->arena;
    sa.src_len = d->arena_used;
    HIP_TRY(launch_mrg_str_sizes(sa, d->s));
    HIP_TRY(launch_exclusive_scan(sizes, cells, sizes.p + cells, d->s));
    HIP_TRY(hipMemcpyAsync(&new_arena_bytes, sizes.p + cells, 8, hipMemcpyDeviceToHost, d->s));
    HIP_TRY(hipStreamSynchronize(d->s));
    HIP_TRY(new_arena.alloc(new_arena_bytes));
    sa.dst = new_arena;
    sa.dst_cap = new_arena_bytes;
    HIP_TRY(launch_mrg_str_copy(sa, d->s));
    HIP_TRY(hipStreamSynchronize(d->s));
    d->arena = std::move(new_arena);
    d->arena_cap = std::max<uint64_t>(new_arena_bytes, 1);
    d->arena_used = new_arena_bytes;
  } else {
    HIP_TRY(hipStreamSynchronize(d->s));
    d->arena_used = 0;
  }
  d->rec = std::move(out);
  d->rec_cap = h_groups;
  d->ngroups = h_groups;
  d->npending = 0;
  ++d->st.compactions;
  d->st.merge_ms += ms_since(t0);
  return Status();
}

// rows decoded behind the pending ones; `staged` bytes of h_stage go to the arena in one copy
// (the *_at arguments: where the parts lie in the staged bytes; data_off_at == 0: a frame)
Status upload_and_decode(MergeDevice* d, uint64_t n, size_t staged, size_t keys_at, size_t data_at,
                         size_t key_off_at, size_t data_off_at, size_t data_end_at) {
  const uint64_t base = align8(d->arena_used);
  Status st = grow_arena(d, base + staged);
  if (!st.ok()) return st;
  st = grow_records(d, d->ngroups + d->npending + n);
  if (!st.ok()) return st;
  HIP_TRY(hipMemcpyAsync(d->arena.p + base, d->h_stage, staged, hipMemcpyHostToDevice, d->s));
  d->stage_busy = true;
  const uint8_t* up = d->arena.p + base;
  MrgDecodeArgs a{};
  a.L = d->L;
  a.keys = up + keys_at;
  a.data = up + data_at;
  a.key_off = reinterpret_cast<const uint32_t*>(up + key_off_at);
  a.data_off = data_off_at ? reinterpret_cast<const uint32_t*>(up + data_off_at) : nullptr;
  a.data_end = data_end_at ? reinterpret_cast<const uint32_t*>(up + data_end_at) : nullptr;
  a.n = n;
  a.arena_pos = base + data_at;
  a.records = d->rec.p + (d->ngroups + d->npending) * d->L.rw;
  HIP_TRY(launch_mrg_decode(a, d->s));
  d->npending += n;
  d->st.rows_added += n;
  // without string cells nothing refers to the upload once it is decoded (stream order)
  d->arena_used = d->str_cols.empty() ? 0 : base + staged;
  return Status();
}

Status check_resident(const MergeDevice* d, uint64_t n) {
  if (d->ngroups + d->npending + n > kMaxResidentRows) {
    return Status::error(EVQL_ENOTSUP, "device merge: more than 2^32 - 1 resident rows");
  }
  return Status();
}

// instance `get` of merge.cc state_value, over the record words of an aggregate
Value state_value(uint32_t fn, uint64_t w, uint64_t cnt) {
  Value v;
  v.tag = 0;
  v.bits = w;
  switch (fn) {
    case EVQL_AGG_COUNT:
    case EVQL_AGG_SUM_UINT64: v.type = EVQL_T_UINT64; return v;
    case EVQL_AGG_SUM_INT64: v.type = EVQL_T_INT64; return v;
    case EVQL_AGG_SUM_FLOAT64: v.type = EVQL_T_FLOAT64; return v;
    case EVQL_AGG_MIN_UINT64:
    case EVQL_AGG_MAX_UINT64: v.type = EVQL_T_UINT64; break;
    case EVQL_AGG_MIN_INT64:
    case EVQL_AGG_MAX_INT64: v.type = EVQL_T_INT64; break;
    case EVQL_AGG_MIN_FLOAT64:
    case EVQL_AGG_MAX_FLOAT64: v.type = EVQL_T_FLOAT64; break;
    default: {
      v.type = EVQL_T_FLOAT64;
      if (cnt) {
        double s;
        memcpy(&s, &w, 8);
        s /= double(cnt);
        memcpy(&v.bits, &s, 8);
      }
    }
  }
  if (cnt == 0) {
    v.bits = 0;
    v.tag = EVQL_STAG_NULL;
  }
  return v;
}

bool two_words(const MergeRecordLayout& L, size_t i) {
  return L.cls[i] != MCELL_VARUINT && L.cls[i] != MCELL_RAW8;
}
bool bare_aggregate(const LoweredProgram& lp) {
  return lp.is_aggregate && lp.call && lp.call->kind == Expr::AGG_GET;
}
uint32_t cell_elem(uint32_t return_type) {
  return return_type == EVQL_T_BOOL ? 2 : 9;
}

// every output column of all groups as SVector bytes, packed by kernels, into d->packed
Status pack_on_device(MergeDevice* d) {
  const uint64_t n = d->ngroups;
  const size_t nsel = d->select.size();
  d->packed.assign(nsel, std::vector<uint8_t>());
  d->packed_off.assign(nsel, std::vector<uint64_t>());
  d->state_words.assign(nsel, std::vector<uint64_t>());
  std::vector<DevBuf<uint8_t>> d_out(nsel);
  std::vector<DevBuf<uint64_t>> d_aux(nsel);
  std::unique_ptr<EmitArgs> ea(new EmitArgs());
  ea->records = d->rec;
  ea->n = n;
  ea->rw = d->L.rw;
  ea->ncols = uint32_t(nsel);
  bool any_fixed_agg = false;
  for (size_t i = 0; i < nsel; ++i) {
    const LoweredProgram& lp = d->select[i];
    EmitCol& e = ea->col[i];
    if (!bare_aggregate(lp)) continue;  // (elem 0: k_emit_fixed leaves the column alone)
    // a state cell by the merge record's own layout (merge_frame_index.h), not the plan's
    e.kind = 1;
    e.stype = lp.return_type;
    e.word = d->L.word[i];
    if (two_words(d->L, i)) e.count_word = int32_t(d->L.word[i] + 1);
    e.is_mean = d->L.op[i] == MFOLD_MEAN;
    e.elem = 9;
    HIP_TRY(d_out[i].alloc(n * 9));
    e.out = d_out[i];
    d->packed[i].resize(n * 9);
    any_fixed_agg = true;
  }
  DevBuf<EmitArgs> d_ea;
  if (any_fixed_agg) {
    HIP_TRY(d_ea.alloc(sizeof(EmitArgs)));
    HIP_TRY(hipMemcpyAsync(d_ea.p, ea.get(), sizeof(EmitArgs), hipMemcpyHostToDevice, d->s));
    HIP_TRY(launch_emit_fixed(d_ea, n, d->s));
  }
  for (size_t i = 0; i < nsel; ++i) {
    const LoweredProgram& lp = d->select[i];
    if (bare_aggregate(lp)) {
      HIP_TRY(hipMemcpyAsync(d->packed[i].data(), d_out[i].p, n * 9, hipMemcpyDeviceToHost, d->s));
    } else if (lp.is_aggregate) {
      // a computed aggregate: its state words come down, eval_expr runs per batch
      const uint32_t words = two_words(d->L, i) ? 2 : 1;
      HIP_TRY(d_aux[i].alloc(n * words * 8));
      d->state_words[i].resize(n * words);
      for (uint32_t w = 0; w < words; ++w) {
        HIP_TRY(launch_extract_word(d->rec, n, d->L.rw, d->L.word[i] + w, d_aux[i].p + w * n, d->s));
      }
      HIP_TRY(hipMemcpyAsync(d->state_words[i].data(), d_aux[i].p, n * words * 8, hipMemcpyDeviceToHost, d->s));
    } else if (lp.return_type == EVQL_T_NIL) {
      continue;  // popVector on NIL appends nothing
    } else {
      MrgCellArgs ca{};
      ca.records = d->rec;
      ca.n = n;
      ca.rw = d->L.rw;
      ca.word = d->L.word[i];
      ca.arena = d->arena;
      ca.arena_len = d->arena_used;
      if (lp.return_type != EVQL_T_STRING) {
        ca.elem = cell_elem(lp.return_type);
        HIP_TRY(d_out[i].alloc(n * ca.elem));
        ca.out = d_out[i];
        ca.out_cap = n * ca.elem;
        HIP_TRY(launch_mrg_cell_fixed(ca, d->s));
        d->packed[i].resize(n * ca.elem);
        HIP_TRY(hipMemcpyAsync(d->packed[i].data(), d_out[i].p, n * ca.elem, hipMemcpyDeviceToHost, d->s));
        continue;
      }
      HIP_TRY(d_aux[i].alloc((n + 1) * 8));
      ca.offsets = d_aux[i];
      HIP_TRY(launch_mrg_cell_str_sizes(ca, d->s));
      HIP_TRY(launch_exclusive_scan(d_aux[i], n, d_aux[i].p + n, d->s));
      d->packed_off[i].resize(n + 1);
      HIP_TRY(hipMemcpyAsync(d->packed_off[i].data(), d_aux[i].p, (n + 1) * 8, hipMemcpyDeviceToHost, d->s));
      HIP_TRY(hipStreamSynchronize(d->s));
      const uint64_t bytes = d->packed_off[i][n];
      HIP_TRY(d_out[i].alloc(bytes));
      ca.out = d_out[i];
      ca.out_cap = bytes;
      HIP_TRY(launch_mrg_cell_str_bytes(ca, d->s));
      d->packed[i].resize(bytes);
      HIP_TRY(hipMemcpyAsync(d->packed[i].data(), d_out[i].p, bytes, hipMemcpyDeviceToHost, d->s));
    }
  }
  HIP_TRY(hipStreamSynchronize(d->s));
  d->stage_busy = false;
  return Status();
}

Status begin_iteration(MergeDevice* d) {
  Status st = compact(d);
  if (!st.ok()) return st;
  const auto t0 = std::chrono::steady_clock::now();
  const size_t nsel = d->select.size();
  d->st.packed_on_device = d->ngroups >= kDeviceEmitMinGroups && nsel > 0 && nsel <= kMaxEmitCols;
  d->h_rec.clear();
  d->h_arena.clear();
  d->packed.clear();
  d->packed_off.clear();
  d->state_words.clear();
  if (d->st.packed_on_device) {
    st = pack_on_device(d);
    if (!st.ok()) return st;
  } else {
    d->h_rec.resize(d->ngroups * d->L.rw);
    if (d->ngroups) HIP_TRY(hipMemcpyAsync(d->h_rec.data(), d->rec.p, d->h_rec.size() * 8, hipMemcpyDeviceToHost, d->s));
    if (!d->str_cols.empty() && d->arena_used) {
      d->h_arena.resize(d->arena_used);
      HIP_TRY(hipMemcpyAsync(d->h_arena.data(), d->arena.p, d->arena_used, hipMemcpyDeviceToHost, d->s));
    }
    HIP_TRY(hipStreamSynchronize(d->s));
    d->stage_busy = false;
  }
  d->st.pack_ms = ms_since(t0);
  d->pos = 0;
  d->iterating = true;
  return Status();
}

}  // namespace

Status merge_device_create(evql_ctx* ctx, const std::vector<LoweredProgram>& select, MergeDevice** out) {
  std::unique_ptr<MergeDevice> d(new MergeDevice());
  switch (merge_record_layout(select, &d->L)) {
    case MLAYOUT_OK: break;
    case MLAYOUT_AGGREGATE:
      return Status::error(EVQL_ENOTSUP, "device merge: count_distinct states are sets (use evql_merge_create)");
    default: return Status::error(EVQL_ENOTSUP, "device merge: too many select expressions");
  }
  d->device = ctx->device;
  d->s = ctx->stream;
  d->select = select;
  for (uint32_t i = 0; i < d->L.ncols; ++i) {
    if (d->L.cls[i] == MCELL_STRING) d->str_cols.push_back(i);
  }
  if (const char* e = getenv("EVQL_MERGE_PENDING_ROWS")) {
    char* end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    if (end != e) d->pending_limit = v;
  }
  d->st.on_device = 1;
  *out = d.release();
  return Status();
}

void merge_device_destroy(MergeDevice* d) {
  if (!d) return;
  // (hipFree waits for the device's outstanding work itself)
  hipSetDevice(d->device);
  delete d;
}

int merge_device_ordinal(const MergeDevice* d) { return d->device; }

Status merge_device_add_frame(MergeDevice* d, const void* payload, size_t len) {
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<uint32_t> row_off;
  MergeIndexResult r = index_merge_frame(d->L, static_cast<const uint8_t*>(payload), len, &row_off);
  d->st.host_index_ms += ms_since(t0);
  if (r != MINDEX_OK) return index_error(r, "invalid partialaggr result encoding");
  const uint64_t n = row_off.size() - 1;
  Status st = check_resident(d, n);
  if (!st.ok()) return st;
  d->iterating = false;
  ++d->st.frames;
  if (n == 0) return Status();
  const auto t1 = std::chrono::steady_clock::now();
  const size_t off_at = align8(len), staged = off_at + row_off.size() * 4;
  st = stage_for(d, staged);
  if (!st.ok()) return st;
  memcpy(d->h_stage, payload, len);
  memcpy(d->h_stage + off_at, row_off.data(), row_off.size() * 4);
  st = upload_and_decode(d, n, staged, 0, 0, off_at, 0, 0);
  d->st.upload_ms += ms_since(t1);
  if (!st.ok()) return st;
  return d->npending > d->pending_limit ? compact(d) : Status();
}

Status merge_device_add_rows(MergeDevice* d, const void* keys, size_t keys_len, const void* data,
                             size_t data_len, size_t nrows) {
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<uint32_t> key_off, data_off, data_end;
  MergeIndexResult r = index_merge_rows(d->L, static_cast<const uint8_t*>(keys), keys_len,
                                        static_cast<const uint8_t*>(data), data_len, nrows, &key_off,
                                        &data_off, &data_end);
  d->st.host_index_ms += ms_since(t0);
  if (r != MINDEX_OK) return index_error(r, "invalid partial aggregate rows");
  Status st = check_resident(d, nrows);
  if (!st.ok()) return st;
  d->iterating = false;
  if (nrows == 0) return Status();
  const auto t1 = std::chrono::steady_clock::now();
  // keys | data | the three offset arrays
  const size_t data_at = align8(keys_len), key_off_at = data_at + align8(data_len);
  const size_t data_off_at = key_off_at + align8(nrows * 4), data_end_at = data_off_at + align8(nrows * 4);
  const size_t staged = data_end_at + nrows * 4;
  st = stage_for(d, staged);
  if (!st.ok()) return st;
  memcpy(d->h_stage, keys, keys_len);
  memcpy(d->h_stage + data_at, data, data_len);
  memcpy(d->h_stage + key_off_at, key_off.data(), nrows * 4);
  memcpy(d->h_stage + data_off_at, data_off.data(), nrows * 4);
  memcpy(d->h_stage + data_end_at, data_end.data(), nrows * 4);
  st = upload_and_decode(d, nrows, staged, 0, data_at, key_off_at, data_off_at, data_end_at);
  d->st.upload_ms += ms_since(t1);
  if (!st.ok()) return st;
  return d->npending > d->pending_limit ? compact(d) : Status();
}

Status merge_device_num_groups(MergeDevice* d, uint64_t* out) {
  Status st = compact(d);
  *out = d->ngroups;
  return st;
}

Status merge_device_next_batch(MergeDevice* d, size_t max_rows, evql_column_buf_t* cols, size_t* nrows) {
  if (!d->iterating) {
    Status st = begin_iteration(d);
    if (!st.ok()) return st;
  }
  const auto t0 = std::chrono::steady_clock::now();
  const size_t nsel = d->select.size();
  const uint64_t take = std::min<uint64_t>(max_rows, d->ngroups - d->pos);
  const uint64_t n = d->ngroups, lo = d->pos, hi = d->pos + take;
  d->out_cols.assign(nsel, std::vector<uint8_t>());
  const std::vector<Value> no_inputs;
  for (size_t i = 0; i < nsel; ++i) {
    const LoweredProgram& lp = d->select[i];
    const uint32_t word = d->L.word[i];
    const bool two = two_words(d->L, i);
    if (d->st.packed_on_device && !(lp.is_aggregate && !bare_aggregate(lp))) {
      // a slice of the packed column
      if (lp.return_type == EVQL_T_NIL && !lp.is_aggregate) {
        cols[i].data = nullptr;
        cols[i].size = 0;
      } else if (!d->packed_off[i].empty()) {
        cols[i].data = d->packed[i].data() + d->packed_off[i][lo];
        cols[i].size = size_t(d->packed_off[i][hi] - d->packed_off[i][lo]);
      } else {
        const uint32_t elem = lp.is_aggregate ? 9 : cell_elem(lp.return_type);
        cols[i].data = d->packed[i].data() + lo * elem;
        cols[i].size = size_t(take * elem);
      }
      continue;
    }
    for (uint64_t g = lo; g < hi; ++g) {
      Value out;
      if (lp.is_aggregate) {
        uint64_t w, cnt = 0;
        if (d->st.packed_on_device) {
          w = d->state_words[i][g];
          if (two) cnt = d->state_words[i][n + g];
        } else {
          w = d->h_rec[g * d->L.rw + word];
          if (two) cnt = d->h_rec[g * d->L.rw + word + 1];
        }
        const Value av = state_value(lp.aggregate_fn, w, cnt);
        std::string e = eval_expr(lp.call, no_inputs, &av, &out);
        if (!e.empty()) return Status::error(EVQL_ERUNTIME, e);
      } else {
        // copyBoxed of the value decoded last (groupby.cc:660-662)
        const uint64_t w = d->h_rec[g * d->L.rw + word], meta = d->h_rec[g * d->L.rw + word + 1];
        out.type = lp.return_type;
        out.tag = uint8_t(meta >> 8);
        if (d->L.cls[i] == MCELL_STRING) {
          const uint64_t len = w >> 40, at = w & kStrOffMask;
          if (len && at + len <= d->h_arena.size()) {
            out.str.assign(reinterpret_cast<const char*>(d->h_arena.data() + at), len);
          }
        } else {
          out.bits = w;
        }
      }
      append_svector(lp.return_type, out, &d->out_cols[i]);
    }
    cols[i].data = d->out_cols[i].data();
    cols[i].size = d->out_cols[i].size();
  }
  d->pos = hi;
  *nrows = size_t(take);
  d->st.pack_ms += ms_since(t0);
  return Status();
}

void merge_device_stats(const MergeDevice* d, evql_merge_stats_t* out) {
  *out = d->st;
  out->rows_pending = d->npending;
  out->groups = d->ngroups;
  out->device_bytes = d->rec_cap * d->L.rw * 8 + d->arena_cap;
}

}  // namespace evql
