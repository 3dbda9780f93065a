// radix_sort.cc -- see radix_sort.h
#include "radix_sort.h"
#include <utility>

namespace evql {

Status RadixSortScratch::alloc(uint64_t n) {
  const uint64_t ntiles = (n + kSortTile - 1) / kSortTile;
  HIP_TRY(keys_alt.alloc(n * 8));
  HIP_TRY(idx_alt.alloc(n * 4));
  HIP_TRY(hist.alloc(size_t(256) * ntiles * 4));
  HIP_TRY(totals.alloc(256 * 4));
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
  SortPassArgs a{};
  a.n = n;
  a.kmin = kmin;
  a.ntiles = uint32_t((n + kSortTile - 1) / kSortTile);
  a.hist = sc->hist;
  a.totals = sc->totals;
  for (uint32_t p = 0; p < passes; ++p) {
    a.keys_in = *keys;
    a.idx_in = sc->idx_identity ? nullptr : idx->p;
    a.keys_out = sc->keys_alt;
    a.idx_out = sc->idx_alt;
    a.shift = 8 * p;
    HIP_TRY(launch_sort_hist(a, s));
    HIP_TRY(launch_sort_digit_scan(a, s));
    HIP_TRY(launch_sort_scatter(a, s));
    sc->launches += 3;
    std::swap(*keys, sc->keys_alt);
    std::swap(*idx, sc->idx_alt);
    sc->idx_identity = false;
  }
  *passes_run += passes;
  *passes_skipped += 8 - passes;
  return Status();
}

}  // namespace evql
