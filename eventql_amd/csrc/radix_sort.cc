// radix_sort.cc -- see radix_sort.h
#include "radix_sort.h"
#include <utility>

namespace evql {

Status radix_sort_passes(const uint64_t* keys_in, const uint32_t* idx_in, uint64_t n, uint64_t kmin,
                         uint32_t passes, RadixPassScratch* sc, hipStream_t s) {
  if (passes == 0) return Status();
  SortPassArgs a{};
  a.n = n;
  a.kmin = kmin;
  a.ntiles = uint32_t((n + kSortTile - 1) / kSortTile);
  if (!sc->hist.p) HIP_TRY(sc->hist.alloc(size_t(256) * a.ntiles * 4));
  if (!sc->totals.p) HIP_TRY(sc->totals.alloc(256 * 4));
  a.hist = sc->hist;
  a.totals = sc->totals;
  for (uint32_t p = 0; p < passes; ++p) {
    const uint32_t to = p & 1, from = to ^ 1;
    if (!sc->keys[to].p) HIP_TRY(sc->keys[to].alloc(n * 8));
    if (!sc->idx[to].p) HIP_TRY(sc->idx[to].alloc(n * 4));
    a.keys_in = p ? sc->keys[from].p : keys_in;
    a.idx_in = p ? sc->idx[from].p : idx_in;
    a.keys_out = sc->keys[to];
    a.idx_out = sc->idx[to];
    a.shift = 8 * p;
    HIP_TRY(launch_sort_hist(a, s));
    HIP_TRY(launch_sort_digit_scan(a, s));
    HIP_TRY(launch_sort_scatter(a, s));
  }
  return Status();
}

Status RadixSortScratch::alloc(uint64_t n) {
  const uint64_t ntiles = (n + kSortTile - 1) / kSortTile;
  HIP_TRY(pass.keys[0].alloc(n * 8));
  HIP_TRY(pass.idx[0].alloc(n * 4));
  HIP_TRY(pass.hist.alloc(size_t(256) * ntiles * 4));
  HIP_TRY(pass.totals.alloc(256 * 4));
  HIP_TRY(stats.alloc(4 * 8));
  return Status();
}

Status radix_sort_pairs(DevBuf<uint64_t>* keys, DevBuf<uint32_t>* idx, uint64_t n,
                        RadixSortScratch* sc, hipStream_t s, uint32_t* passes_run,
                        uint32_t* passes_skipped) {
  if (n >= (1ull << 32)) return Status::error(EVQL_EARG, "radix sort: too many pairs");
  HIP_TRY(hipMemsetAsync(sc->stats, 0, 3 * 8, s));
  HIP_TRY(launch_sort_key_stats(*keys, n, sc->stats, s));
  HIP_TRY(hipMemcpyAsync(sc->h_stats, sc->stats.p, 4 * 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  ++sc->launches;
  ++sc->waits;
  if (n <= 1 || sc->h_stats[2] == 0) {  // already in order
    *passes_skipped += 8;
    return Status();
  }
  const uint64_t kmin = ~sc->h_stats[0], kmax = sc->h_stats[1];
  uint32_t bits = 0;
  for (uint64_t range = kmax - kmin; range; range >>= 1) ++bits;
  const uint32_t passes = (bits + 7) / 8;
  // the caller's pair is side 1 of the ping-pong, the scratch's side 0
  RadixPassScratch& pp = sc->pass;
  pp.keys[1] = std::move(*keys);
  pp.idx[1] = std::move(*idx);
  Status st = radix_sort_passes(pp.keys[1], sc->idx_identity ? nullptr : pp.idx[1].p, n, kmin, passes, &pp, s);
  const uint32_t last = (passes - 1) & 1;
  if (last == 0) {
    std::swap(pp.keys[0], pp.keys[1]);
    std::swap(pp.idx[0], pp.idx[1]);
  }
  *keys = std::move(pp.keys[1]);
  *idx = std::move(pp.idx[1]);
  if (!st.ok()) return st;
  sc->launches += 3 * passes;
  sc->idx_identity = false;
  *passes_run += passes;
  *passes_skipped += 8 - passes;
  return Status();
}

}  // namespace evql
