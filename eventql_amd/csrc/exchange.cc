// exchange.cc -- the exchange step of a GROUP BY that ran on several GPUs.
//
// The reference fans partial aggregates in over TCP: every partition's
// PartialGroupByExpression rows travel as EVQL_OP_QUERY_PARTIALAGGR frames to the
// coordinator's GroupByMergeExpression (sql/statements/select/groupby.cc:438-472,
// 528-637; server/sql/scheduler.cc:117-162).  Here a partition's groups sit in the HBM
// of the GPU that scanned it, as dense records [kind, identity, (identity 2), (first
// row), states...]; they are bucketed by owner on the device, moved GPU to GPU (RCCL
// send/recv over xGMI, or peer copies inside one process) and merged with one kernel
// launch per source rank, in rank order, into a fresh table.
#include <rccl/rccl.h>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include "runtime.h"

using namespace evql;

// ---------------------------------------------------------------------------------------
// in-process hub: ranks are threads of one process
// ---------------------------------------------------------------------------------------
struct evql_hub {
  int nranks = 0;
  std::mutex mu;
  std::condition_variable cv;
  int arrived = 0;
  uint64_t generation = 0;
  std::vector<const uint64_t*> host_send;              // all_gather
  std::vector<const uint64_t*> dev_send;               // all_to_all: packed send buffers
  std::vector<std::vector<uint64_t>> send_counts;      // [src][dst]
  int error = EVQL_OK;                                 // first failure of any rank (sticky)
  std::string error_msg;
  void barrier() {
    std::unique_lock<std::mutex> lk(mu);
    const uint64_t gen = generation;
    if (++arrived == nranks) {
      arrived = 0;
      ++generation;
      cv.notify_all();
    } else {
      cv.wait(lk, [&] { return generation != gen; });
    }
  }
};

struct evql_exchange {
  evql_ctx* ctx = nullptr;
  int nranks = 1, rank = 0;
  evql_transport_t tr{};
  std::string name;
  // built-in transports
  evql_hub* hub = nullptr;
  ncclComm_t comm = nullptr;
  uint64_t* d_scratch = nullptr;  // rccl all_gather of counts
  evql_exchange_stats_t stats{};
  // device buffers of the exchange step, kept (and only ever grown) between calls:
  // a step of a running query allocates nothing
  struct Slot {
    void* p = nullptr;
    size_t cap = 0;
  };
  Slot ws[20];
  hipError_t get(int slot, size_t bytes, void** out) {
    Slot& sl = ws[slot];
    if (bytes > sl.cap) {
      if (sl.p) hipFree(sl.p);
      sl.p = nullptr;
      sl.cap = 0;
      const size_t want = bytes + bytes / 4 + 4096;
      hipError_t e = hipMalloc(&sl.p, want);
      if (e != hipSuccess) return e;
      sl.cap = want;
    }
    *out = sl.p;
    return hipSuccess;
  }
  ~evql_exchange() {
    for (auto& sl : ws) {
      if (sl.p) hipFree(sl.p);
    }
  }
};

// a typed view of a workspace slot with DevBuf's interface
template <typename T>
struct WsBuf {
  evql_exchange* x;
  int slot;
  T* p = nullptr;
  WsBuf(evql_exchange* xx, int s) : x(xx), slot(s) {}
  hipError_t alloc(size_t bytes) { return x->get(slot, bytes ? bytes : 8, reinterpret_cast<void**>(&p)); }
  operator T*() const { return p; }
};

namespace {

// Every rank reaches every barrier of a collective even after a local failure (a rank
// that returned early would leave its peers waiting on the condition variable for
// ever); the first error is kept in the hub and every rank reports it.  A transport
// error is fatal to the hub / communicator: the caller tears it down.  (A refusal that
// exchange() agrees on in its go / no-go gather is none: it never comes through here.)
int hub_fail(evql_hub* h, int code, const char* msg) {
  std::unique_lock<std::mutex> lk(h->mu);
  if (h->error == EVQL_OK) {
    h->error = code;
    h->error_msg = msg;
  }
  return code;
}

int hub_result(evql_hub* h) {
  std::unique_lock<std::mutex> lk(h->mu);
  if (h->error != EVQL_OK) return fail(h->error, h->error_msg);
  return EVQL_OK;
}

int hub_all_gather(void* user, const uint64_t* send, uint64_t n, uint64_t* recv) {
  evql_exchange* x = static_cast<evql_exchange*>(user);
  evql_hub* h = x->hub;
  h->host_send[x->rank] = send;
  h->barrier();
  for (int r = 0; r < x->nranks; ++r) memcpy(recv + uint64_t(r) * n, h->host_send[r], n * 8);
  h->barrier();
  return hub_result(h);
}

int hub_all_to_all(void* user, const uint64_t* d_send, const uint64_t* send_counts, uint64_t* d_recv,
                   const uint64_t* recv_counts, void* stream) {
  evql_exchange* x = static_cast<evql_exchange*>(user);
  evql_hub* h = x->hub;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the send buffer has to be complete before another rank's thread reads it
  if (hipStreamSynchronize(s) != hipSuccess) hub_fail(h, EVQL_EDEVICE, "hub: stream sync failed");
  h->dev_send[x->rank] = d_send;
  h->send_counts[x->rank].assign(send_counts, send_counts + x->nranks);
  h->barrier();
  uint64_t roff = 0;
  bool ok = hub_result(h) == EVQL_OK;
  for (int r = 0; ok && r < x->nranks; ++r) {
    uint64_t soff = 0;
    for (int d = 0; d < x->rank; ++d) soff += h->send_counts[r][d];
    const uint64_t cnt = h->send_counts[r][x->rank];
    if (cnt != recv_counts[r]) {
      hub_fail(h, EVQL_ERUNTIME, "hub: counts disagree");
      ok = false;
      break;
    }
    if (cnt && hipMemcpyAsync(d_recv + roff, h->dev_send[r] + soff, cnt * 8, hipMemcpyDefault, s) !=
                   hipSuccess) {
      hub_fail(h, EVQL_EDEVICE, "hub: device copy failed");
      ok = false;
      break;
    }
    roff += cnt;
  }
  if (hipStreamSynchronize(s) != hipSuccess) hub_fail(h, EVQL_EDEVICE, "hub: stream sync failed");
  h->barrier();  // nobody reuses a send buffer before everyone has copied from it
  return hub_result(h);
}

int rccl_all_gather(void* user, const uint64_t* send, uint64_t n, uint64_t* recv) {
  evql_exchange* x = static_cast<evql_exchange*>(user);
  hipStream_t s = x->ctx->stream;
  if (n > 512) return fail(EVQL_EARG, "rccl all_gather: too many words");
  uint64_t* d_send = x->d_scratch;
  uint64_t* d_recv = x->d_scratch + 512;
  if (hipMemcpyAsync(d_send, send, n * 8, hipMemcpyHostToDevice, s) != hipSuccess) {
    return fail(EVQL_EDEVICE, "rccl all_gather: copy failed");
  }
  if (ncclAllGather(d_send, d_recv, n, ncclUint64, x->comm, s) != ncclSuccess) {
    return fail(EVQL_EDEVICE, "ncclAllGather failed");
  }
  if (hipMemcpyAsync(recv, d_recv, uint64_t(x->nranks) * n * 8, hipMemcpyDeviceToHost, s) !=
          hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess) {
    return fail(EVQL_EDEVICE, "rccl all_gather: copy back failed");
  }
  return EVQL_OK;
}

int rccl_all_to_all(void* user, const uint64_t* d_send, const uint64_t* send_counts, uint64_t* d_recv,
                    const uint64_t* recv_counts, void* stream) {
  evql_exchange* x = static_cast<evql_exchange*>(user);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // xGMI is point to point: one send and one receive per peer, all in flight at once
  if (ncclGroupStart() != ncclSuccess) return fail(EVQL_EDEVICE, "ncclGroupStart failed");
  ncclResult_t rc = ncclSuccess;
  bool self_ok = true;
  uint64_t soff = 0, roff = 0;
  for (int r = 0; r < x->nranks; ++r) {
    // (a failed call inside the group: the group is still closed, so that the calls
    // already queued are matched on the peers, and the error is reported afterwards)
    if (r == x->rank) {
      // this rank's own share never leaves the device: one copy on the stream instead of
      // a send / receive pair through the communicator's staging kernels
      if (send_counts[r] != recv_counts[r]) {
        self_ok = false;
      } else if (send_counts[r] &&
                 hipMemcpyAsync(d_recv + roff, d_send + soff, send_counts[r] * 8,
                                hipMemcpyDeviceToDevice, s) != hipSuccess) {
        self_ok = false;
      }
    } else {
      if (send_counts[r] && rc == ncclSuccess) {
        rc = ncclSend(d_send + soff, send_counts[r], ncclUint64, r, x->comm, s);
      }
      if (recv_counts[r] && rc == ncclSuccess) {
        rc = ncclRecv(d_recv + roff, recv_counts[r], ncclUint64, r, x->comm, s);
      }
    }
    soff += send_counts[r];
    roff += recv_counts[r];
  }
  const ncclResult_t rce = ncclGroupEnd();
  if (rc != ncclSuccess) {
    return fail(EVQL_EDEVICE, std::string("ncclSend / ncclRecv failed: ") + ncclGetErrorString(rc));
  }
  if (rce != ncclSuccess) {
    return fail(EVQL_EDEVICE, std::string("ncclGroupEnd failed: ") + ncclGetErrorString(rce));
  }
  if (!self_ok) return fail(EVQL_EDEVICE, "exchange: copy of this rank's own share failed");
  return EVQL_OK;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// One exchange: what crosses its steps, and the steps in the order exchange_steps runs them.
struct ExchangeRun {
  evql_query* const q;
  evql_exchange* const x;
  const hipStream_t s;
  const int N;
  const GroupRecordLayout L;
  // a chain head (a chain of two or more files): its groups are those chain_merge left in d_mtab
  const bool from_chain;
  const bool by_owner;    // else: every rank gets every record
  uint64_t n = 0, rank_tag = 0;  // this rank's groups; what goes in front of their scan positions
  // device buffers: slots of the exchange's workspace
  WsBuf<uint64_t> d_rec{x, 0}, d_wire{x, 1}, d_send{x, 3}, d_aux{x, 4}, d_sizes{x, 5}, d_recv{x, 7},
      d_rep{x, 8}, d_hsend{x, 9}, d_hrecv{x, 10};
  WsBuf<RtColumn> d_cols{x, 2};
  WsBuf<uint8_t> d_heap{x, 6};
  // this rank's n wire records, what is sent, the received records rank by rank
  const uint64_t *d_src = nullptr, *d_out = nullptr, *d_in = nullptr;
  std::vector<uint64_t> send_counts, starts;  // records per owner, first record of every owner
  std::vector<uint64_t> heap_counts;          // string bytes per destination
  std::vector<uint64_t> recv_rec, hbase;      // per source rank: records, first byte of its strings
  uint64_t total_rec = 0, total_heap_words = 0;
  uint64_t ng = 0;  // merged groups (read back by finish_merge's synchronisation)
  std::chrono::steady_clock::time_point t0, t1, t2;

  ExchangeRun(evql_query* qq, evql_exchange* xx, int mode)
      : q(qq), x(xx), s(qq->ctx->stream), N(xx->nranks), L(group_record_layout(qq->rplan())),
        from_chain(qq->merged && qq->chain_merged),
        by_owner(mode == EVQL_EXCHANGE_BY_OWNER && xx->nranks > 1), send_counts(N, 0),
        starts(N + 1, 0), heap_counts(N, 0), recv_rec(N, 0), hbase(N, 0) {}
  // d_aux: [counts per owner | starts | cursors]
  static constexpr size_t kAuxBytes = (3 * kMaxExchangeRanks + 4) * 8;
  uint64_t* d_counts() const { return d_aux.p; }
  uint64_t* d_starts() const { return d_aux.p + kMaxExchangeRanks; }
  uint64_t* d_cursors() const { return d_aux.p + 2 * kMaxExchangeRanks + 2; }

  Status go_no_go();
  Status export_records();
  Status bucket_by_owner();
  Status export_strings();
  Status transfer();
  Status merge_received();
  Status bucketed_merge(bool* done);
  Status exchange_pairsets();
  Status exchange_pairset(int which, const uint64_t* src_set, uint64_t src_cap, uint32_t word);
  Status finish_merge();
};

// count_distinct (aggregate.cc:77-137: a std::set per group, merged by insertion): the
// stored triples of pair set `which` go to the ranks that own their groups (all ranks
// for GATHER_ALL) and are inserted into a fresh set there; every triple that is new to
// it adds 1 to state word `word` of its group in the merged table.
// `src_set` / `src_cap`: this rank's own set -- the scan's, or for a chain head the chain's
// merged one, which is also the destination: its triples are in the workspace before it is
// reallocated or cleared.
Status ExchangeRun::exchange_pairset(int which, const uint64_t* src_set, uint64_t src_cap,
                               uint32_t word) {
  const bool exact = q->kp.key_mode == KEY_EXACT;
  uint64_t np = 0;
  uint64_t* d_cnt = q->d_counters + kScratchCounter;
  Status st = pairset_count(q, src_set, src_cap, &np);
  if (!st.ok()) return st;
  WsBuf<uint64_t> d_tr(x, 11), d_tsend(x, 12), d_trecv(x, 13);
  HIP_TRY(d_tr.alloc(std::max<uint64_t>(np, 1) * 24));
  if (np) {
    HIP_TRY(hipMemsetAsync(d_cnt, 0, 8, s));
    HIP_TRY(launch_pairset_export(src_set, src_cap, d_tr, np, d_cnt, s));
  }
  std::vector<uint64_t> tr_counts(N, np), tr_starts(N + 1, 0);
  if (by_owner) {
    HIP_TRY(d_tsend.alloc(std::max<uint64_t>(np, 1) * 24));
    HIP_TRY(hipMemsetAsync(d_aux, 0, kAuxBytes, s));  // (bucket_by_owner's)
    HIP_TRY(launch_triple_owner_hist(d_tr, np, uint32_t(N), exact, d_counts(), s));
    HIP_TRY(hipMemcpyAsync(tr_counts.data(), d_counts(), N * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int r = 0; r < N; ++r) tr_starts[r + 1] = tr_starts[r] + tr_counts[r];
    HIP_TRY(hipMemcpyAsync(d_starts(), tr_starts.data(), (N + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_triple_owner_scatter(d_tr, np, uint32_t(N), exact, d_starts(), d_cursors(), d_tsend, s));
  } else {
    // the same triples to everybody (replicated per destination like the records)
    HIP_TRY(d_tsend.alloc(std::max<uint64_t>(np * N, 1) * 24));
    for (int r = 0; r < N; ++r) {
      HIP_TRY(hipMemcpyAsync(d_tsend.p + uint64_t(r) * np * 3, d_tr, np * 24, hipMemcpyDeviceToDevice, s));
    }
  }
  std::vector<uint64_t> all(uint64_t(N) * N);
  int rc = x->tr.all_gather_u64(x->tr.user, tr_counts.data(), N, all.data());
  if (rc != EVQL_OK) return Status::error(rc, "exchange: all_gather of the pair counts failed");
  std::vector<uint64_t> send_words(N), recv_words(N);
  uint64_t total = 0;
  for (int r = 0; r < N; ++r) {
    const uint64_t from_r = all[uint64_t(r) * N + x->rank];
    send_words[r] = tr_counts[r] * 3;
    recv_words[r] = from_r * 3;
    total += from_r;
  }
  HIP_TRY(d_trecv.alloc(std::max<uint64_t>(total, 1) * 24));
  rc = x->tr.all_to_all_words(x->tr.user, d_tsend, send_words.data(), d_trecv, recv_words.data(), s);
  if (rc != EVQL_OK) return Status::error(rc, "exchange: transfer of the count_distinct pairs failed");
  HIP_TRY(hipStreamSynchronize(s));
  x->stats.bytes_sent += (by_owner ? np : np * uint64_t(N - 1)) * 24;
  uint64_t set_cap = 1024;
  while (set_cap < total * 2) set_cap <<= 1;
  // the merged set belongs to the query: EVQL_MODE_PARTIAL rows carry the values of every
  // group's set (aggregate.cc:111-117), read back from here at emission
  return merged_set_fill(q, L, which, set_cap, word, d_trecv, total);
}

// -----------------------------------------------------------------------------------------
// large merges: split by identity hash into LDS-sized buckets, merge every bucket in the LDS
// -----------------------------------------------------------------------------------------
// Merging 1e7 received records into an HBM hash table costs 2.1 ms however few atomics a
// record needs (scattered line accesses over a > 1 GB table).  From kBucketedMergeMin
// records on, the records take two LDS-staged scatter passes (<= 256 bins each, regions
// with slack instead of a histogram pass) and one LDS merge per bucket, and the merged
// groups stay with the query as dense records (q->d_mdense).  *done = false: the shape
// does not fit (count_distinct needs the table for its lookups, records too wide for a
// tile / an LDS table) or a region outgrew its slack -- the caller merges through the table.
static const uint64_t kBucketedMergeMin = 1ull << 18;

Status ExchangeRun::bucketed_merge(bool* done) {
  *done = false;
  const uint32_t mw = L.mw, rw = mw + 1;
  if (total_rec < kBucketedMergeMin || recv_rec.size() > kMaxExchangeRanks) return Status();
  // LDS table of a bucket: <= 60 KB (30 KB tables = twice the buckets measured slower: 1.44 vs
  // 1.05 ms per 1e7 records), power of two slots + the two keyless groups
  uint32_t slots = 1;
  while (uint64_t(slots * 2 + 2) * (mw * 8 + 4) <= 60 * 1024) slots *= 2;
  if (slots < 64) return Status();
  uint32_t tile = uint32_t((56 * 1024) / (rw * 8)) / 256 * 256;
  if (tile > 2048) tile = 2048;
  if (tile < 256) return Status();
  int nsrc = 0;
  for (uint64_t c : recv_rec) nsrc += c ? 1 : 0;
  // buckets: a power of two with <= slots / 3 records on average, two levels of <= 256 bins
  uint32_t fbits = 1;
  while ((total_rec >> fbits) > slots / 3) ++fbits;
  const uint32_t c1_bits = (fbits + 1) / 2, c2_bits = fbits - c1_bits;
  if (c1_bits > 8) return Status();
  const uint32_t C1 = 1u << c1_bits, C2 = 1u << c2_bits;
  const uint64_t F = uint64_t(C1) * C2;
  // a group arrives once per source rank: the spread of a region is that of nsrc-fold copies
  auto region_cap = [&](double avg, double floor_) {
    return uint64_t(avg + 6.0 * std::sqrt(avg * std::max(nsrc, 1)) + floor_);
  };
  const uint64_t cap1 = region_cap(double(total_rec) / C1, 1024);
  const uint64_t cap2 = region_cap(double(total_rec) / double(F), 64);
  WsBuf<uint64_t> d_stage1(x, 14), d_stage2(x, 15), d_cur(x, 16);
  HIP_TRY(d_stage1.alloc(uint64_t(C1) * cap1 * rw * 8));
  HIP_TRY(d_stage2.alloc(F * cap2 * rw * 8));
  // cursors, then -- each on a line of its own -- the output counter (one add per bucket)
  // and the overflow flag (read by every workgroup of the later passes: next to the counter
  // those reads queued behind its atomics, 0.43 -> 2.7 ms for the merge pass)
  const uint64_t ncur = C1 + F + 64;
  HIP_TRY(d_cur.alloc(ncur * 8));
  HIP_TRY(hipMemsetAsync(d_cur, 0, ncur * 8, s));
  uint64_t* d_cnt1 = d_cur.p;
  uint64_t* d_cnt2 = d_cur.p + C1;
  uint64_t* d_out_count = d_cur.p + C1 + F + 16;
  uint32_t* d_flag = reinterpret_cast<uint32_t*>(d_cur.p + C1 + F + 48);
  if (q->mdense_cap < total_rec) {
    if (q->d_mdense) hipFree(q->d_mdense);
    q->d_mdense = nullptr;
    q->mdense_cap = 0;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&q->d_mdense), total_rec * rw * 8));
    q->mdense_cap = total_rec;
  }
  BucketScatterArgs sa{};
  sa.in = d_in;
  sa.out = d_stage1;
  sa.in_counts = nullptr;
  sa.n_in = total_rec;
  sa.in_region_cap = total_rec;
  sa.in_regions = 1;
  sa.tiles_per_region = uint32_t((total_rec + tile - 1) / tile);
  sa.tile = tile;
  sa.rw = rw;
  sa.rw_inv = uint32_t(((1ull << 32) + rw - 1) / rw);
  sa.shift = 64 - c1_bits;
  sa.bins = C1;
  sa.out_region_cap = cap1;
  sa.out_counts = d_cnt1;
  sa.status = d_flag;
  sa.first_value_word = 1 + L.W;
  sa.ncols = L.nc;
  sa.str_mask = L.str_mask;
  sa.nranks = uint32_t(recv_rec.size());
  uint64_t off = 0;
  for (size_t r = 0; r < recv_rec.size(); ++r) {
    sa.rank_start[r] = off;
    sa.heap_base[r] = hbase[r];
    off += recv_rec[r];
  }
  sa.rank_start[recv_rec.size()] = off;
  HIP_TRY(launch_bucket_scatter(sa, s));
  const bool two_levels = c2_bits > 0;
  BucketScatterArgs sb = sa;
  sb.in = d_stage1;
  sb.out = d_stage2;
  sb.in_counts = d_cnt1;
  sb.in_region_cap = cap1;
  sb.in_regions = C1;
  sb.tiles_per_region = uint32_t((cap1 + tile - 1) / tile);
  sb.shift = 64 - c1_bits - c2_bits;
  sb.bins = C2;
  sb.out_region_cap = cap2;
  sb.out_counts = d_cnt2;
  sb.nranks = 0;
  sb.str_mask = 0;
  if (two_levels) HIP_TRY(launch_bucket_scatter(sb, s));
  BucketMergeArgs ba{};
  ba.stage = two_levels ? d_stage2.p : d_stage1.p;
  ba.counts = two_levels ? d_cnt2 : d_cnt1;
  ba.region_cap = two_levels ? cap2 : cap1;
  ba.buckets = uint32_t(F);
  ba.mw = mw;
  ba.has_ident2 = L.has_ident2;
  ba.state_words = L.W;
  ba.first_row_word = L.first_row_word;
  ba.ncols = L.resolved ? L.nc : 0;
  ba.lds_slots = slots;
  MergeArgs m{};
  merge_ops(q->rplan(), true, &m);
  for (uint32_t w = 0; w < mw; ++w) ba.ops[w] = m.ops[w];
  slot_identities(q->rplan(), mw, ba.identity);
  ba.out = q->d_mdense;
  ba.out_cap = q->mdense_cap;
  ba.out_count = d_out_count;
  ba.status = d_flag;
  HIP_TRY(launch_bucket_merge(ba, s));
  uint64_t tail[33] = {0};  // [groups, ..., flag]
  HIP_TRY(hipMemcpyAsync(tail, d_out_count, sizeof(tail), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (tail[32] & 0xffffffffull) return Status();  // (a region / an LDS table overflowed)
  q->mdense_n = tail[0];
  q->merged_dense = true;
  x->stats.merge_buckets = F;
  *done = true;
  return Status();
}

// -----------------------------------------------------------------------------------------
// the exchange itself: its steps in the order exchange_steps runs them
// -----------------------------------------------------------------------------------------
// What this rank alone can tell -- before anything is allocated or filled -- only sets a
// status: a rank that returned here would leave its peers waiting in the first collective.
// One gather of [status, tables scanned, the four exact-sum quanta] per rank tells
// everybody; a refusal is no transport error and leaves the hub / communicator as it was.
Status ExchangeRun::go_no_go() {
  const KernelPlan& kp = q->rplan();
  Status pre = group_record_layout_check(L, "an exchanged");
  if (!q->executed) {
    pre = Status::error(EVQL_EARG, "execute() was not called");
  } else if (q->merged && !q->chain_merged) {
    pre = Status::error(EVQL_EARG, "the query was exchanged already");
  } else if (pre.ok() && from_chain && q->m_words + 1 != L.rw) {
    pre = Status::error(EVQL_ERUNTIME, "chain: the merged slots do not match the plan");
  }
  const uint32_t kGo = 6;
  std::vector<uint64_t> mine_g(kGo), all_g(uint64_t(kGo) * N);
  mine_g[0] = uint64_t(int64_t(pre.code));
  mine_g[1] = 1 + q->chain.size();
  for (int k = 0; k < 4; ++k) mine_g[2 + k] = uint64_t(int64_t(q->fsum_exp[k]));
  const int rcg = x->tr.all_gather_u64(x->tr.user, mine_g.data(), kGo, all_g.data());
  if (rcg != EVQL_OK) return Status::error(rcg, "exchange: all_gather of the go / no-go records failed");
  if (!pre.ok()) return pre;
  uint64_t max_tables = 1;
  for (int r = 0; r < N; ++r) {
    const int code = int(int64_t(all_g[uint64_t(r) * kGo]));
    if (code != EVQL_OK) {
      return Status::error(EVQL_ERUNTIME, "exchange refused by rank " + std::to_string(r) +
                                              " (status " + std::to_string(code) + ")");
    }
    max_tables = std::max(max_tables, all_g[uint64_t(r) * kGo + 1]);
  }
  // the scan position of a first row, ordered by (rank, table of the chain, row):
  // rank << (44 + tb) | table << 44 | row.  No chain anywhere: tb = 0, rank << 44 | row.
  auto bits_of = [](uint64_t v) {
    uint32_t b = 0;
    for (; v; v >>= 1) ++b;
    return b;
  };
  const uint32_t tb = bits_of(max_tables - 1);
  if (L.resolved && 44 + tb + bits_of(uint64_t(N - 1)) > 63) {
    // (every rank sees the same counts: all of them answer this)
    return Status::error(EVQL_ENOTSUP, "too many ranks x tables of a chain for the scan position word");
  }
  rank_tag = uint64_t(x->rank) << (44 + tb);
  if (kp.n_exact > 0) {
    // EVQL_FLOAT_SUM_EXACT: the state words are integer multiples of 2^fsum_exp and are
    // added as they are -- every rank must have chosen the same quantum.  With
    // float_sum_bound = 0 each rank derives it from its OWN table's maxima, which may
    // fall on either side of a power of two.
    for (int r = 0; r < N; ++r) {
      for (int k = 0; k < kp.n_exact; ++k) {
        if (all_g[uint64_t(r) * kGo + 2 + k] != mine_g[2 + k]) {
          return Status::error(EVQL_EARG,
                               "exact float sums: the ranks chose different quanta (the tables' "
                               "maxima differ); pass the same float_sum_bound on every rank");
        }
      }
    }
  }
  return Status();
}

// This rank's groups as wire records (d_src): dense records, with first-row values if resolved.
Status ExchangeRun::export_records() {
  // (a chain head: the count the chain merge left, which a fetch under ORDER BY .. LIMIT keeps
  // -- q->ngroups is then the number of rows that fetch emitted)
  n = from_chain ? q->stats.num_groups : q->ngroups;
  if (from_chain) {
    // a slot of the merged table behind its kind word is a wire record already (first-row
    // words resolved inside the table that produced them, strings as offsets into the
    // chain's heap): one pass, which also puts the rank in front of the scan position.  It
    // is complete on the stream before merge_received re-initialises d_mtab.
    HIP_TRY(d_wire.alloc(std::max<uint64_t>(n, 1) * L.rw * 8));
    uint64_t* d_cnt = q->d_counters + kScratchCounter;
    HIP_TRY(hipMemsetAsync(d_cnt, 0, 8, s));
    HIP_TRY(launch_mtab_compact(q->d_mtab, q->mcap, q->m_words, L.first_row_word, rank_tag,
                                d_wire, n, d_cnt, s));
    d_src = d_wire;
    return Status();
  }
  RecordsView view;
  Status st = query_records_view(q, &view);
  if (!st.ok()) return st;
  const uint64_t* d_records = view.dense;  // n records of rw_in words
  if (!(n && view.nd == n)) {
    // (else the partitioned path left every group as a dense record: read in place)
    HIP_TRY(d_rec.alloc(std::max<uint64_t>(n, 1) * L.rw_in * 8));
    st = query_dense_records(q, L, view, d_rec);
    if (!st.ok()) return st;
    d_records = d_rec;
  }
  d_src = d_records;
  if (!L.resolved) return Status();
  HIP_TRY(d_cols.alloc(std::max<uint32_t>(L.nc, 1) * sizeof(RtColumn)));
  HIP_TRY(d_wire.alloc(std::max<uint64_t>(n, 1) * L.rw * 8));
  std::vector<RtColumn> rc;
  st = resolve_first_rows(q, L, rank_tag, &rc, d_cols, d_records, n, d_wire);
  if (!st.ok()) return st;
  HIP_TRY(hipStreamSynchronize(s));  // (d_cols / rc live until here)
  d_src = d_wire;
  return Status();
}

// The wire records in the order they are sent (d_out), send_counts / starts.
Status ExchangeRun::bucket_by_owner() {
  const uint32_t rw = L.rw;
  HIP_TRY(d_send.alloc(std::max<uint64_t>(n, 1) * rw * 8));
  d_out = d_send.p;
  HIP_TRY(d_aux.alloc(kAuxBytes));
  if (by_owner) {
    HIP_TRY(hipMemsetAsync(d_aux, 0, kAuxBytes, s));
    HIP_TRY(launch_owner_hist(d_src, n, rw, uint32_t(N), d_counts(), s));
    HIP_TRY(hipMemcpyAsync(send_counts.data(), d_counts(), N * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int r = 0; r < N; ++r) starts[r + 1] = starts[r] + send_counts[r];
    HIP_TRY(hipMemcpyAsync(d_starts(), starts.data(), (N + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(launch_owner_scatter(d_src, n, rw, uint32_t(N), d_starts(), d_cursors(), d_send, s));
    return Status();
  }
  // every rank gets every record: "bucket" r = all of them (copied only when the string
  // words are about to be rewritten in place, export_strings)
  if (!L.str_cols.empty()) {
    HIP_TRY(hipMemcpyAsync(d_send, d_src, n * rw * 8, hipMemcpyDeviceToDevice, s));
  } else {
    d_out = d_src;
  }
  for (int r = 0; r < N; ++r) send_counts[r] = n;
  for (int r = 1; r <= N; ++r) starts[r] = n;  // (one segment)
  return Status();
}

// String bytes in record order: d_heap, heap_counts (transfer re-packs them to whole words).
Status ExchangeRun::export_strings() {
  if (L.str_cols.empty() || !n) return Status();
  const uint8_t* flat = nullptr;
  if (from_chain) {
    // (the chain's first-row strings: offsets into its device heap)
    if (!q->d_mheap.p) {  // (every string empty)
      HIP_TRY(q->d_mheap.alloc(8));
      q->mheap_cap = 8;
    }
    flat = q->d_mheap;
  }
  HIP_TRY(d_sizes.alloc((n + 2) * 8));
  const uint32_t nseg = by_owner ? uint32_t(N) : 1u;  // (GATHER_ALL: starts = [0, n, ..], one segment)
  std::vector<uint64_t> segoff(N + 1, 0);
  auto heap_for = [&](uint64_t bytes) {
    return d_heap.alloc(bytes + 8 * (N + 1)) == hipSuccess ? d_heap.p : nullptr;
  };
  Status st = wire_strings(q, L, flat, d_send, n, starts.data(), nseg, d_sizes, d_starts(), heap_for,
                           segoff.data());
  if (!st.ok()) return st;
  for (int r = 0; r < N; ++r) heap_counts[r] = by_owner ? segoff[r + 1] - segoff[r] : segoff[1];
  return Status();
}

// Counts, then the records and the string bytes: d_in / recv_rec, d_hrecv / hbase.
Status ExchangeRun::transfer() {
  const uint32_t rw = L.rw;
  // per destination: [record count, heap bytes]
  std::vector<uint64_t> mine(2 * N), all(uint64_t(2) * N * N);
  for (int r = 0; r < N; ++r) {
    mine[2 * r] = by_owner ? send_counts[r] : n;
    mine[2 * r + 1] = heap_counts[r];
  }
  int rc = x->tr.all_gather_u64(x->tr.user, mine.data(), 2 * N, all.data());
  if (rc != EVQL_OK) return Status::error(rc, "exchange: all_gather of the counts failed");
  std::vector<uint64_t> recv_heap(N), send_words(N), recv_words(N);
  for (int r = 0; r < N; ++r) {
    recv_rec[r] = all[uint64_t(r) * 2 * N + 2 * x->rank];
    recv_heap[r] = all[uint64_t(r) * 2 * N + 2 * x->rank + 1];
    total_rec += recv_rec[r];
    total_heap_words += (recv_heap[r] + 7) / 8;
    send_words[r] = mine[2 * r] * rw;
    recv_words[r] = recv_rec[r] * rw;
  }
  HIP_TRY(d_recv.alloc(std::max<uint64_t>(N == 1 ? 1 : total_rec, 1) * rw * 8));
  d_in = d_recv.p;
  if (by_owner) {
    rc = x->tr.all_to_all_words(x->tr.user, d_send, send_words.data(), d_recv, recv_words.data(), s);
  } else {
    // GATHER_ALL: the same n records to everybody -- as an all-to-all whose send
    // segments coincide (the transports read `send_counts[r]` words at the running
    // offset, so the buffer is replicated per destination only logically)
    if (N == 1) {
      // a single rank receives exactly what it sends: merged where it lies
      d_in = d_out;
    } else {
      HIP_TRY(d_rep.alloc(std::max<uint64_t>(n * rw * N, 1) * 8));
      for (int r = 0; r < N; ++r) {
        HIP_TRY(hipMemcpyAsync(d_rep.p + uint64_t(r) * n * rw, d_out, n * rw * 8,
                               hipMemcpyDeviceToDevice, s));
      }
      rc = x->tr.all_to_all_words(x->tr.user, d_rep, send_words.data(), d_recv, recv_words.data(), s);
    }
    if (rc == EVQL_OK) HIP_TRY(hipStreamSynchronize(s));
  }
  if (rc != EVQL_OK) return Status::error(rc, "exchange: transfer of the records failed");
  // string heaps: word-aligned segments
  if (!L.str_cols.empty()) {
    std::vector<uint64_t> hs(N), hr(N);
    uint64_t tot = 0;
    for (int r = 0; r < N; ++r) {
      hs[r] = (heap_counts[r] + 7) / 8;
      hr[r] = (recv_heap[r] + 7) / 8;
      tot += hs[r];
    }
    HIP_TRY(d_hsend.alloc(std::max<uint64_t>(tot, 1) * 8));
    HIP_TRY(d_hrecv.alloc(std::max<uint64_t>(total_heap_words, 1) * 8));
    uint64_t woff = 0, boff = 0;
    for (int r = 0; r < N; ++r) {
      if (heap_counts[r]) {
        HIP_TRY(hipMemcpyAsync(d_hsend.p + woff, d_heap.p + (by_owner ? boff : 0), heap_counts[r],
                               hipMemcpyDeviceToDevice, s));
      }
      woff += hs[r];
      if (by_owner) boff += heap_counts[r];
    }
    rc = x->tr.all_to_all_words(x->tr.user, d_hsend, hs.data(), d_hrecv, hr.data(), s);
    if (rc != EVQL_OK) return Status::error(rc, "exchange: transfer of the strings failed");
    uint64_t b = 0;
    for (int r = 0; r < N; ++r) {
      hbase[r] = b;
      b += hr[r] * 8;
    }
  }
  HIP_TRY(hipStreamSynchronize(s));
  x->stats.transfer_ms = ms_since(t1);
  t2 = std::chrono::steady_clock::now();
  x->stats.groups_sent = by_owner ? n : n * uint64_t(N);
  x->stats.groups_received = total_rec;
  for (int r = 0; r < N; ++r) {
    if (r != x->rank) x->stats.bytes_sent += send_words[r] * 8 + heap_counts[r];
  }
  return Status();
}

// The received records into a fresh table -- or, when they are many, into dense records.
Status ExchangeRun::merge_received() {
  HIP_TRY(hipMemsetAsync(q->d_status, 0, 16, s));
  q->merged_dense = false;
  bool bucketed = false;
  if (q->rplan().n_distinct == 0) {
    Status stb = bucketed_merge(&bucketed);
    if (!stb.ok()) return stb;
  }
  if (bucketed) {
    ng = q->mdense_n;
    q->m_words = L.mw;
    return Status();
  }
  MergeResolvedArgs ma;
  Status st = merged_table_prepare(q, L, total_rec, &ma);
  if (!st.ok()) return st;
  uint64_t roff = 0;
  for (int r = 0; r < N; ++r) {  // (one launch per source rank, in rank order)
    ma.heap_base = hbase[r];
    if (recv_rec[r] && L.resolved) {
      HIP_TRY(launch_table_merge_resolved(ma, d_in + roff * L.rw, recv_rec[r], s));
    } else if (recv_rec[r]) {
      HIP_TRY(launch_table_merge(ma.m, d_in + roff * L.rw, recv_rec[r], s));
    }
    roff += recv_rec[r];
  }
  HIP_TRY(hipMemcpyAsync(&ng, ma.m.fresh, 8, hipMemcpyDeviceToHost, s));
  return Status();
}

// count_distinct: the pair sets follow their groups
Status ExchangeRun::exchange_pairsets() {
  const KernelPlan& kp = q->rplan();
  for (const auto& ag : kp.aggs) {
    if (ag.distinct_index < 0) continue;
    const int d = ag.distinct_index;
    Status st = exchange_pairset(d, from_chain ? q->d_mset[d] : q->d_pairset[d],
                                 from_chain ? q->mset_cap[d] : q->pairset_cap,
                                 uint32_t(kp.state_word_base() + ag.first_word));
    if (!st.ok()) return st;
  }
  return Status();
}

// what the merge kernels reported, then the query holds the exchanged groups
Status ExchangeRun::finish_merge() {
  uint32_t status[4] = {0};
  HIP_TRY(hipMemcpyAsync(status, q->d_status, 16, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  Status st = merge_status_error(status[0], "merged ");
  if (!st.ok()) return st;
  // the received string bytes are what the merged groups' string words point into
  q->m_heap.clear();
  if (!L.str_cols.empty() && total_heap_words) {
    q->m_heap.resize(total_heap_words * 8);
    HIP_TRY(hipMemcpy(q->m_heap.data(), d_hrecv, total_heap_words * 8, hipMemcpyDeviceToHost));
  }
  q->merged = true;
  q->chain_merged = false;  // (d_mtab / d_mdense now hold the exchanged groups)
  q->ngroups = ng;
  q->stats.num_groups = ng;
  q->fetched = false;
  q->order_applied = false;
  q->tail_valid = false;  // (the eager block holds this rank's groups before the merge)
  q->emit_pos = 0;
  x->stats.merge_ms = ms_since(t2);
  return Status();
}

// *source_gone: set once the call starts to overwrite what it reads its groups from (only a
// chain head's: d_mtab / d_mset are source and destination)
static Status exchange_steps(evql_query* q, evql_exchange* x, int mode, bool* source_gone) {
  if (x->nranks > int(kMaxExchangeRanks)) return Status::error(EVQL_EARG, "too many ranks");
  ExchangeRun R(q, x, mode);
  R.t0 = std::chrono::steady_clock::now();
  x->stats = evql_exchange_stats_t{};
  Status st = R.go_no_go();  // (the first collective: no rank returns before it)
  if (st.ok()) st = R.export_records();
  if (st.ok()) st = R.bucket_by_owner();
  if (st.ok()) st = R.export_strings();
  if (!st.ok()) return st;
  x->stats.export_ms = ms_since(R.t0);
  R.t1 = std::chrono::steady_clock::now();
  st = R.transfer();
  if (!st.ok()) return st;
  *source_gone = R.from_chain;
  st = R.merge_received();
  if (st.ok()) st = R.exchange_pairsets();
  if (st.ok()) st = R.finish_merge();
  return st;
}

Status exchange(evql_query* q, evql_exchange* x, int mode) {
  bool source_gone = false;
  Status st = exchange_steps(q, x, mode, &source_gone);
  if (!st.ok() && source_gone) {
    // A late failure (merged table / set full, a transport error behind the transfer) of a
    // chain head: its merged table and sets are re-initialised or half filled with exchanged
    // data.  A plain query still has d_gtab; this one holds nothing it could emit or exchange
    // again and asks for a new execute().
    q->executed = false;
    q->merged = false;
    q->chain_merged = false;
    q->merged_dense = false;
    q->ngroups = 0;
    q->stats.num_groups = 0;
  }
  return st;
}

}  // namespace

// ---------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------
extern "C" {

int evql_exchange_create(evql_ctx_t* ctx, int nranks, int rank, const evql_transport_t* transport,
                         evql_exchange_t** out) {
  if (!ctx || !transport || !out || nranks < 1 || rank < 0 || rank >= nranks ||
      !transport->all_gather_u64 || !transport->all_to_all_words) {
    return fail(EVQL_EARG, "bad arguments");
  }
  evql_exchange* x = new evql_exchange();
  x->ctx = ctx;
  x->nranks = nranks;
  x->rank = rank;
  x->tr = *transport;
  x->name = transport->name ? transport->name : "custom";
  *out = x;
  return EVQL_OK;
}

int evql_hub_create(int nranks, evql_hub_t** out) {
  if (nranks < 1 || !out) return fail(EVQL_EARG, "bad arguments");
  evql_hub* h = new evql_hub();
  h->nranks = nranks;
  h->host_send.assign(nranks, nullptr);
  h->dev_send.assign(nranks, nullptr);
  h->send_counts.assign(nranks, std::vector<uint64_t>(nranks, 0));
  *out = h;
  return EVQL_OK;
}

void evql_hub_destroy(evql_hub_t* hub) { delete hub; }

int evql_exchange_create_hub(evql_ctx_t* ctx, evql_hub_t* hub, int rank, evql_exchange_t** out) {
  if (!ctx || !hub || !out || rank < 0 || rank >= hub->nranks) return fail(EVQL_EARG, "bad arguments");
  evql_exchange* x = new evql_exchange();
  x->ctx = ctx;
  x->nranks = hub->nranks;
  x->rank = rank;
  x->hub = hub;
  x->tr.user = x;
  x->tr.all_gather_u64 = hub_all_gather;
  x->tr.all_to_all_words = hub_all_to_all;
  x->name = "hub";
  *out = x;
  return EVQL_OK;
}

int evql_rccl_unique_id(void* id128) {
  if (!id128) return fail(EVQL_EARG, "null argument");
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return fail(EVQL_EDEVICE, "ncclGetUniqueId failed");
  memcpy(id128, &id, sizeof(id));
  return EVQL_OK;
}

int evql_exchange_create_rccl(evql_ctx_t* ctx, int nranks, int rank, const void* id128,
                              evql_exchange_t** out) {
  if (!ctx || !id128 || !out || nranks < 1 || rank < 0 || rank >= nranks) {
    return fail(EVQL_EARG, "bad arguments");
  }
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(EVQL_EDEVICE, "hipSetDevice failed");
  ncclUniqueId id;
  memcpy(&id, id128, sizeof(id));
  evql_exchange* x = new evql_exchange();
  x->ctx = ctx;
  x->nranks = nranks;
  x->rank = rank;
  if (ncclCommInitRank(&x->comm, nranks, id, rank) != ncclSuccess) {
    delete x;
    return fail(EVQL_EDEVICE, "ncclCommInitRank failed");
  }
  if (hipMalloc(reinterpret_cast<void**>(&x->d_scratch), (512 + 512 * kMaxExchangeRanks) * 8) !=
      hipSuccess) {
    ncclCommDestroy(x->comm);
    delete x;
    return fail(EVQL_EDEVICE, "hipMalloc failed");
  }
  x->tr.user = x;
  x->tr.all_gather_u64 = rccl_all_gather;
  x->tr.all_to_all_words = rccl_all_to_all;
  x->name = "rccl";
  *out = x;
  return EVQL_OK;
}

void evql_exchange_destroy(evql_exchange_t* x) {
  if (!x) return;
  if (x->comm) ncclCommDestroy(x->comm);
  if (x->d_scratch) hipFree(x->d_scratch);
  delete x;
}

const char* evql_exchange_backend(const evql_exchange_t* x) { return x ? x->name.c_str() : ""; }

int evql_query_exchange(evql_query_t* q, evql_exchange_t* x, int mode) {
  if (!q || !x) return fail(EVQL_EARG, "null argument");
  if (mode != EVQL_EXCHANGE_GATHER_ALL && mode != EVQL_EXCHANGE_BY_OWNER) {
    return fail(EVQL_EARG, "bad exchange mode");
  }
  if (q->kp.bare_scan) return fail(EVQL_EARG, "a bare scan holds no groups");
  try {
    if (hipSetDevice(q->ctx->device) != hipSuccess) return fail(EVQL_EDEVICE, "hipSetDevice failed");
    Status st = exchange(q, x, mode);
    if (!st.ok()) return fail(st.code, st.msg);
    return EVQL_OK;
  } catch (const std::exception& e) {
    return fail(EVQL_ERUNTIME, e.what());
  }
}

int evql_exchange_last_stats(const evql_exchange_t* x, evql_exchange_stats_t* out) {
  if (!x || !out) return fail(EVQL_EARG, "null argument");
  *out = x->stats;
  return EVQL_OK;
}

}  // extern "C"
