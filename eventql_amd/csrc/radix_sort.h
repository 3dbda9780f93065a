// radix_sort.h -- the one driver of the stable LSD radix sort of (u64 key, u32 index) pairs
// (launch_sort_hist / _digit_scan / _scatter, aot_kernels.h): the digit passes, which every
// sort on the device runs through (results.cc sort_on_device, materialize.cc, chain_compact.cc
// sort_rows, merge_device.cc sort_by_word), and -- for callers whose statistics ride on no
// other wait -- the key statistics in front of them.
#pragma once
#include "runtime.h"

namespace evql {

// the two sides of the ping-pong: pass p writes side p & 1 and -- behind pass 0 -- reads the
// other one
struct RadixPassScratch {
  DevBuf<uint64_t> keys[2];  // n each
  DevBuf<uint32_t> idx[2];   // n each
  DevBuf<uint32_t> hist;     // [256][ceil(n / kSortTile)]
  DevBuf<uint32_t> totals;   // [256]
};

// `passes` digit passes of 8 bits, from bit 0 of key - kmin upwards: three launches each, no
// wait.  Pass 0 reads keys_in and idx_in (NULL: the identity 0 .. n-1), which may be side 1 of
// the scratch itself.  What the passes need and the scratch does not hold yet is allocated
// here: no pass, no allocation; one pass, side 0 alone.  The sorted pairs are in side
// (passes - 1) & 1.  n < 2^32.
Status radix_sort_passes(const uint64_t* keys_in, const uint32_t* idx_in, uint64_t n, uint64_t kmin,
                         uint32_t passes, RadixPassScratch* scratch, hipStream_t s);

struct RadixSortScratch {
  RadixPassScratch pass;
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
