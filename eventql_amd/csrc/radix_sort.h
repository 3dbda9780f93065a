// radix_sort.h -- one driver for the stable LSD radix sort of (u64 key, u32 index) pairs
// (launch_sort_hist / _digit_scan / _scatter, aot_kernels.h): key statistics first, then only
// the digit passes the keys need.
#pragma once
#include "runtime.h"

namespace evql {

struct RadixSortScratch {
  DevBuf<uint64_t> keys_alt;  // n: the other side of the ping-pong
  DevBuf<uint32_t> idx_alt;   // n
  DevBuf<uint32_t> hist;      // [256][ceil(n / kSortTile)]
  DevBuf<uint32_t> totals;    // [256]
  // [0..2] launch_sort_key_stats, zeroed by every sort; [3] the caller's: a status word its
  // own kernels raise, copied to the host with the statistics in the sort's one wait
  DevBuf<uint64_t> stats;
  uint64_t h_stats[4] = {0, 0, 0, 0};
  // in: `idx` holds nothing yet and stands for 0 .. n-1; out: still so (no pass ran)
  bool idx_identity = true;
  uint32_t launches = 0, waits = 0;
  Status alloc(uint64_t n);
};

// Sorts the n pairs (keys[i], idx[i]) by key, stable.  One host wait, for the key statistics:
// keys already non-descending run no pass at all, and no digit pass runs above the highest
// set bit of max - min.  Both buffers swap with the scratch's on an odd number of passes, so
// the sorted pairs are in *keys / *idx on return.  n < 2^32.
Status radix_sort_pairs(DevBuf<uint64_t>* keys, DevBuf<uint32_t>* idx, uint64_t n,
                        RadixSortScratch* scratch, hipStream_t s, uint32_t* passes_run,
                        uint32_t* passes_skipped);

}  // namespace evql
