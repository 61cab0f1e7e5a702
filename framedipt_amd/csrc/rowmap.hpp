// rowmap.hpp — the row map of the mapped accuracy entries (include/fdipt.h, "accuracy through a row map"): what
// lddt_mapped.hip, gdt_mapped.hip and interface_mapped.hip share - the range-checked read of an entry, the verdict on a map, and the
// pre-pass of the two entries that judge a pair's map in a launch of its own.  map[j] is the model row that corresponds to reference
// row j, or -1.
#pragma once
#include "common.hpp"

#define FD_MAP_BITS 32768                 // model rows per window of the duplicate check
#define FD_MAP_WORDS (FD_MAP_BITS / 32)   // 4 KB of LDS

// The model row of reference row j, or -1 where the map leaves it open, points outside the model or at a row the model's mask drops.
// An entry is range-checked at every read: the device data decide what is addressed, whatever the verdict on the map was.
__device__ __forceinline__ int fd_map_row(const int* mp, const float* mask_a, int n_a, int j) {
  const int r = mp[j];
  return (r >= 0 && r < n_a && mask_a[r] != 0.f) ? r : -1;
}

// The verdict on one map row mp[0 .. n): FDIPT_MAP_OUT_OF_RANGE for an entry < -1 or >= n_a, FDIPT_MAP_DUPLICATE for two j with the
// same entry >= 0.  Called by every thread of the block; returns the same bits in all of them.  The duplicates are found in a bit per
// model row in LDS (bits_sh: FD_MAP_WORDS words), filled with atomicOr on its words, a window of FD_MAP_BITS model rows at a time:
// integer atomics on LDS only, and the verdict does not depend on which thread meets a row first.
__device__ __forceinline__ int fd_map_check(const int* mp, int n, int n_a, unsigned* bits_sh, int* flag_sh) {
  const int tid = threadIdx.x;
  int flags = 0;
  if (tid == 0) *flag_sh = 0;
  for (int w0 = 0; w0 < n_a; w0 += FD_MAP_BITS) {
    const int w1 = n_a - w0 < FD_MAP_BITS ? n_a : w0 + FD_MAP_BITS, words = (w1 - w0 + 31) / 32;
    for (int w = tid; w < words; w += FD_THREADS) bits_sh[w] = 0u;
    __syncthreads();
    for (int j = tid; j < n; j += FD_THREADS) {
      const int r = mp[j];
      if (w0 == 0 && (r < -1 || r >= n_a)) flags |= FDIPT_MAP_OUT_OF_RANGE;
      if (r >= w0 && r < w1) {
        const unsigned bit = 1u << ((r - w0) & 31);
        if (atomicOr(&bits_sh[(r - w0) >> 5], bit) & bit) flags |= FDIPT_MAP_DUPLICATE;
      }
    }
    __syncthreads();
  }
  if (flags) atomicOr(flag_sh, flags);
  __syncthreads();
  return *flag_sh;
}

// The LDS of fd_map_judge.
struct FdMapLds {
  unsigned bits[FD_MAP_WORDS];
  int flag, count[2];
};

// The pre-pass of the entries that judge a pair's map in a launch of its own (lddt_mapped.hip, interface_mapped.hip), called by every
// thread of the pair's block: fd_map_check's verdict on mp[0 .. n), then the reference rows that exist (mask_b: n_reference) and those
// of them with a model row that exists (fd_map_row with mask_a: n_covered), both 0 under a verdict.  Every thread gets the same three
// numbers.  The counts are ballots summed with integer atomics on LDS: no order changes them.
__device__ __forceinline__ int fd_map_judge(const int* mp, const float* mask_a, const float* mask_b, int n, int n_a, FdMapLds& lds, int& n_covered,
                                            int& n_reference) {
  const int tid = threadIdx.x;
  if (tid < 2) lds.count[tid] = 0;
  const int verdict = fd_map_check(mp, n, n_a, lds.bits, &lds.flag);  // (with barriers: count is zero for everyone behind it)
  for (int j0 = 0; j0 < n; j0 += FD_THREADS) {
    const int j = j0 + tid;
    const bool ex = j < n && mask_b[j < n ? j : 0] != 0.f;
    const bool cov = ex && fd_map_row(mp, mask_a, n_a, j) >= 0;
    const unsigned long long be = __ballot(ex), bc = __ballot(cov);
    if ((tid & (FD_WAVE - 1)) == 0) {
      if (be) atomicAdd(&lds.count[1], __popcll(be));
      if (bc) atomicAdd(&lds.count[0], __popcll(bc));
    }
  }
  __syncthreads();
  n_covered = verdict ? 0 : lds.count[0];
  n_reference = verdict ? 0 : lds.count[1];
  return verdict;
}
