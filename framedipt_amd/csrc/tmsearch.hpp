// tmsearch.hpp — the seed search tmscore.hip and tmalign.hip share (with the two parameters of section
// 7.9): for n pairs of rows in LDS, superpose a fragment, score all pairs, select the pairs inside the cut, superpose the selection,
// until the set stops changing; the result is the first seed in seed order that holds the largest score.  Fragment starts are `step`
// rows apart plus the last start; with d8sq > 0 the score runs over the pairs with d^2 <= d8sq only (the selection over all pairs).
// Plain float64 arithmetic in a fixed order: an including unit turns contraction off (#pragma clang fp contract) and includes
// common.hpp and horn.hpp before this file.
#pragma once

#define TM_MAX_PASSES 21  // the seed's own superposition and 20 refinements
#define TM_LEVELS 6
#define TM_CUT_LIMIT 1e4  // Angstrom: the widening of the cut ends here

struct TmTransform { double R[9], t[3]; };

// the best proper rotation of the rows of `set` and its translation
__device__ __forceinline__ void tm_superpose(const double* px, const double* py, const double* pz, const double* qx, const double* qy, const double* qz,
                                             const unsigned* set, int n, TmTransform& T) {
  double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, m = 0.0;
  unsigned word = 0;
  for (int i = 0; i < n; ++i) {
    if ((i & 31) == 0) word = set[(i >> 5) * FD_THREADS];
    if ((word >> (i & 31)) & 1u) {
      c[0] += px[i]; c[1] += py[i]; c[2] += pz[i];
      c[3] += qx[i]; c[4] += qy[i]; c[5] += qz[i];
      m += 1.0;
    }
  }
  const double inv_m = m > 0.0 ? 1.0 / m : 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) c[k] *= inv_m;
  double H[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < n; ++i) {
    if ((i & 31) == 0) word = set[(i >> 5) * FD_THREADS];
    if ((word >> (i & 31)) & 1u) {
      const double ax = px[i] - c[0], ay = py[i] - c[1], az = pz[i] - c[2], bx = qx[i] - c[3], by = qy[i] - c[4], bz = qz[i] - c[5];
      H[0] += ax * bx; H[1] += ax * by; H[2] += ax * bz;
      H[3] += ay * bx; H[4] += ay * by; H[5] += ay * bz;
      H[6] += az * bx; H[7] += az * by; H[8] += az * bz;
    }
  }
  double top, second, scale;
  fd_horn_rotation(H, T.R, top, second, scale);
  T.t[0] = -(T.R[0] * c[0] + T.R[1] * c[1] + T.R[2] * c[2]) + c[3];
  T.t[1] = -(T.R[3] * c[0] + T.R[4] * c[1] + T.R[5] * c[2]) + c[4];
  T.t[2] = -(T.R[6] * c[0] + T.R[7] * c[1] + T.R[8] * c[2]) + c[5];
}

__device__ __forceinline__ double tm_dist2(const TmTransform& T, double x, double y, double z, double u, double v, double w) {
  const double dx = T.R[0] * x + T.R[1] * y + T.R[2] * z + T.t[0] - u, dy = T.R[3] * x + T.R[4] * y + T.R[5] * z + T.t[1] - v,
               dz = T.R[6] * x + T.R[7] * y + T.R[8] * z + T.t[2] - w;
  return dx * dx + dy * dy + dz * dz;
}

__host__ __device__ inline size_t tm_search_lds_bytes(int rows) {
  // two masks of ceil(rows / 32) words per thread, the reduction's score and seed per thread
  return (size_t)2 * ((rows + 31) / 32) * FD_THREADS * 4 + (size_t)FD_THREADS * 12;
}

// The search over the n >= 3 pairs (px, py, pz)[i] with (qx, qy, qz)[i], by all FD_THREADS threads of the block (it holds barriers).
// `masks`: tm_search_lds_bytes(rows) bytes of LDS with W = ceil(rows / 32) >= ceil(n / 32), 8-byte aligned; `next_sh`, `passes_sh`: two
// ints of LDS.  Every thread owns a seed (fragment length, start) at a time and walks the pairs serially; all lanes read the same LDS
// address, a broadcast.  The selected set is a bit mask in LDS, word w of thread t at [w][t]; two masks per thread (the set superposed
// and the set being selected) make "the set did not change" exact.  The loop is flat: an iteration is one pass of whatever seed the
// lane holds, and a lane whose seed ends takes the next seed number from the counter.  Which lane serves which seed depends on timing;
// no output does.  Returns true in the one thread that holds the winner: there `best` is its score (negative: no seed scored),
// `best_seed` its number and `Tbest` the transform at which it reached it; `*passes_sh` is the number of passes of all seeds.
__device__ __forceinline__ bool tm_search(const double* px, const double* py, const double* pz, const double* qx, const double* qy, const double* qz, int n,
                                          double d0sq, double d_search, int step, double d8sq, unsigned* masks, int W, int* next_sh, int* passes_sh,
                                          double& best, int& best_seed, TmTransform& Tbest) {
  const int tid = threadIdx.x;
  unsigned *cur = masks + tid, *nxt = masks + (size_t)W * FD_THREADS + tid;
  double* red_s = (double*)(masks + (size_t)2 * W * FD_THREADS);
  int* red_seed = (int*)(red_s + FD_THREADS);
  // the fragment ladder: n >> k while it exceeds 4, then 4 (n itself below 4); seeds are numbered level-major, start-minor
  int len[TM_LEVELS], first[TM_LEVELS + 1], levels = 0;
  first[0] = 0;
  for (int k = 0; k < 5 && (n >> k) > 4; ++k) {
    len[levels] = n >> k;
    first[levels + 1] = first[levels] + (n - len[levels]) / step + 1 + ((n - len[levels]) % step != 0);
    ++levels;
  }
  len[levels] = n < 4 ? n : 4;
  first[levels + 1] = first[levels] + (n - len[levels]) / step + 1 + ((n - len[levels]) % step != 0);
  ++levels;
  const int n_seeds = first[levels], words = (n + 31) / 32;
  if (tid == 0) *next_sh = FD_THREADS, *passes_sh = 0;
  __syncthreads();

  best = -1.0, best_seed = 0x7fffffff;
  double seed_best = -1.0;
  int seed = tid, it = 0, my_passes = 0;
  TmTransform T;
#pragma unroll
  for (int k = 0; k < 9; ++k) Tbest.R[k] = 0.0;
  Tbest.t[0] = Tbest.t[1] = Tbest.t[2] = 0.0;
  bool fresh = true;
  while (seed < n_seeds) {
    if (fresh) {  // the seed's fragment is the first set
      int lv = 0;
      while (seed >= first[lv + 1]) ++lv;
      int s0 = (seed - first[lv]) * step;  // the last start of a level is n - len, whatever the step
      if (s0 > n - len[lv]) s0 = n - len[lv];
      const int s1 = s0 + len[lv];  // rows s0 .. s1 - 1
      for (int w = 0; w < words; ++w) {
        const int lo = w * 32, b0 = s0 > lo ? s0 - lo : 0, b1 = s1 - lo < 32 ? s1 - lo : 32;
        unsigned m = 0;
        if (b1 > b0) m = (b1 - b0 == 32 ? 0xffffffffu : ((1u << (b1 - b0)) - 1u)) << b0;
        cur[w * FD_THREADS] = m;
      }
      it = 0, seed_best = -1.0, fresh = false;
    }
    tm_superpose(px, py, pz, qx, qy, qz, cur, n, T);
    ++my_passes;
    // score all rows and select those inside the cut in one walk
    double cut = it == 0 ? d_search - 1.0 : d_search + 1.0, score;
    bool same;
    for (;;) {
      const double cut2 = cut * cut;
      int inside = 0;
      unsigned m = 0;
      score = 0.0, same = true;
      for (int i = 0; i < n; ++i) {
        const double d2 = tm_dist2(T, px[i], py[i], pz[i], qx[i], qy[i], qz[i]);
        if (!(d8sq > 0.0) || d2 <= d8sq) score += d0sq / (d0sq + d2);
        if (d2 < cut2) m |= 1u << (i & 31), ++inside;
        if ((i & 31) == 31 || i == n - 1) {
          same = same && m == cur[(i >> 5) * FD_THREADS];
          nxt[(i >> 5) * FD_THREADS] = m;
          m = 0;
        }
      }
      if (inside >= 3 || n <= 3 || !(cut < TM_CUT_LIMIT)) break;
      // fewer than 3 rows inside: the cut grows by 0.5 until the third smallest distance is inside (or the limit is reached: such
      // coordinates are no protein's, or not finite), found without walking the rows once per step; then the walk above runs again
      double m1 = 1.0 / 0.0, m2 = m1, m3 = m1;
      for (int i = 0; i < n; ++i) {
        const double d2 = tm_dist2(T, px[i], py[i], pz[i], qx[i], qy[i], qz[i]);
        if (d2 < m1) m3 = m2, m2 = m1, m1 = d2;
        else if (d2 < m2) m3 = m2, m2 = d2;
        else if (d2 < m3) m3 = d2;
      }
      do cut += 0.5;
      while (!(m3 < cut * cut) && cut < TM_CUT_LIMIT);
    }
    if (score > seed_best) {
      seed_best = score;
      if (score > best || (score == best && seed < best_seed)) best = score, best_seed = seed, Tbest = T;
    }
    ++it;
    if (same || it == TM_MAX_PASSES) {
      seed = atomicAdd(next_sh, 1);
      fresh = true;
    } else {
      unsigned* t = cur;
      cur = nxt, nxt = t;
    }
  }
  atomicAdd(passes_sh, my_passes);
  __syncthreads();  // (every thread is done with the masks: the reduction's arrays lie behind them)

  // the first seed that holds the largest score
  red_s[tid] = best, red_seed[tid] = best_seed;
  __syncthreads();
  int owner = 0;
  for (int t = 1; t < FD_THREADS; ++t)
    if (red_s[t] > red_s[owner] || (red_s[t] == red_s[owner] && red_seed[t] < red_seed[owner])) owner = t;
  return tid == owner;
}
