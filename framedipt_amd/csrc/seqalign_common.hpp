// seqalign_common.hpp — what the two sequence-alignment units share (seqalign.hip: fdipt_seq_align; seqalign_modes.hip:
// fdipt_seq_align_modes): the LDS layout of a wave, the wavefront fence, the slab offset of a diagonal and the launch plan.  The
// kernels differ (the modes choose their end cell and carry an origin); each unit states its score-only bytes per index.
#pragma once
#include "common.hpp"

#define SQ_NEG (-(1 << 30))  // unreachable; |reachable| < 2^27 and |every sum with it| < 2^31 under FDIPT_SEQ_MAX_HALF_UNITS
#define SQ_TABLE_BYTES 1792  // 21 * 21 int32, padded to a multiple of 16
#define SQ_LDS_MAX (160 * 1024)

struct SqLayout {
  int L1;          // indices i = 0 .. max_len_a, rounded up to a multiple of 4
  int LA, LB;      // letters of a and of b, rounded likewise
  int wave_bytes;  // of one wave's region, a multiple of 16
};
// per index: scores of M, X, Y, G; then (trace) G's state byte, or (score only) `extra` bytes: what rides with each of the four states
static inline __host__ __device__ SqLayout sq_layout(int max_a, int max_b, bool trace, int extra) {
  SqLayout l;
  l.L1 = (max_a + 1 + 3) & ~3, l.LA = (max_a + 3) & ~3, l.LB = (max_b + 3) & ~3;
  const int bytes = 4 * l.L1 * 4 + (trace ? l.L1 : l.L1 * extra) + l.LA + l.LB;
  l.wave_bytes = (bytes + 15) & ~15;
  return l;
}

// LDS writes of one step become visible to the other lanes' reads of the next: the wave runs in lockstep and its LDS operations complete
// in order, so what is needed is that the compiler keeps the order
__device__ __forceinline__ void sq_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// cells (i >= 1, j >= 1) of the diagonals before d = i + j, of a la x lb pair: where the direction bytes of diagonal d start in the slab
__device__ __forceinline__ int sq_diag_offset(int d, int la, int lb) {
  const int t = d - 2, mn = la < lb ? la : lb, mx = la < lb ? lb : la;
  if (t <= mn) return t * (t + 1) / 2;
  if (t <= mx) return mn * (mn + 1) / 2 + (t - mn) * mn;
  const int r = la + lb - 1 - t;
  return la * lb - r * (r + 1) / 2;
}

// waves of a block, its dynamic LDS, and the persistent waves of a launch over P pairs
static inline int sq_plan(int P, int max_a, int max_b, bool trace, int extra, int& wpb, size_t& lds) {
  const SqLayout lay = sq_layout(max_a, max_b, trace, extra);
  wpb = FD_THREADS / FD_WAVE;
  while (wpb > 1 && SQ_TABLE_BYTES + (size_t)wpb * lay.wave_bytes > 64 * 1024) wpb >>= 1;
  lds = SQ_TABLE_BYTES + (size_t)wpb * lay.wave_bytes;
  if (lds > SQ_LDS_MAX) return 0;
  const int blocks = (int)(SQ_LDS_MAX / lds) < 8 ? (int)(SQ_LDS_MAX / lds) : 8;
  const int per_cu = blocks * wpb < 16 ? blocks * wpb : 16;
  const long waves = (long)fd_cu_count() * per_cu;
  return (int)(waves < P ? waves : P);
}

// the slab rule of both entries: W slabs of max_len_a x max_len_b bytes, W lowered until they fit max_workspace_bytes, at least one
static inline size_t sq_workspace_bytes(int P, int max_len_a, int max_len_b, int traceback, size_t max_workspace_bytes, int extra) {
  if (!traceback || P < 1 || max_len_a < 1 || max_len_b < 1 || max_len_a > FDIPT_SEQ_MAX_ROWS || max_len_b > FDIPT_SEQ_MAX_ROWS) return 0;
  int wpb;
  size_t lds;
  const size_t slab = (size_t)max_len_a * max_len_b;
  size_t waves = (size_t)sq_plan(P, max_len_a, max_len_b, true, extra, wpb, lds);
  if (waves > max_workspace_bytes / slab) waves = max_workspace_bytes / slab;
  return (waves < 1 ? 1 : waves) * slab;
}
