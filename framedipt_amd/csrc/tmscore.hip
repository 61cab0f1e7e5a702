// tmscore.hip — TM-score of samples on the device (include/fdipt.h, "TM-score"): Zhang & Skolnick's TMscore
// search over seed superpositions for a GIVEN residue correspondence (row i of one structure with row i of the other), for P pairs of
// structures, all in float64.  It is the number the reference takes from tmtools.tm_align where the alignment is the identity (a sample
// against its ground truth or its refold) and a lower bound of it elsewhere (the all-against-all matrix of hierarchy_diversity);
// TM-align's alignment search is not built.
//
// One launch, a block per pair, no workspace traffic:
//   (a) the block compacts the CA atoms of the rows where both masks are set into LDS in ascending row order (ballot + popcount per
//       wave, the four waves' counts through LDS), float32 widened to float64, six arrays of N doubles
//   (b) every thread owns a seed (fragment length, start) at a time and walks the rows serially: all lanes read the same LDS address
//       (a broadcast, no bank conflict).  A pass is: superpose the selected rows (centroids, covariance about them, Horn's 4 x 4
//       eigenproblem by Jacobi sweeps in registers: horn.hpp), score all n rows under the transform, select the rows inside the cut.
//       The selected set is a bit mask in LDS, word w of thread t at [w][t] (consecutive lanes, consecutive banks); two masks per thread
//       (the set superposed and the set being selected) make "the set did not change" exact.  No cross-lane operation in the search.
//       The loop is flat: an iteration is one pass of whatever seed the lane holds, a lane whose seed ends takes the next seed number
//       from a counter in LDS.  Which lane serves which seed depends on timing; no output does: a seed's result depends on the seed
//       alone, and the best seed is the largest score, the lowest seed number among equals.
//   (c) one ordered reduction over the threads' best seeds; the owner of the winner writes the pair's outputs.
// Contraction into fused multiply-adds is off in this unit: the sums are compared with a NumPy evaluation in the same order.
#include "common.hpp"

#pragma clang fp contract(off)

#include "horn.hpp"

#define TM_MAX_ROWS FDIPT_TM_MAX_ROWS
#define TM_MAX_PASSES 21  // the seed's own superposition and 20 refinements
#define TM_LEVELS 6
#define TM_CUT_LIMIT 1e4  // Angstrom: the widening of the cut ends here

__host__ __device__ inline size_t tm_lds_bytes(int N) {
  // six coordinate arrays, two masks of ceil(N / 32) words per thread, the reduction's score and seed per thread
  return (size_t)6 * N * 8 + (size_t)2 * ((N + 31) / 32) * FD_THREADS * 4 + (size_t)FD_THREADS * 12;
}

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

__global__ __launch_bounds__(FD_THREADS) void tm_score_kernel(FdiptTmArgs a) {
  extern __shared__ double tm_sh[];
  __shared__ int cnt_sh[FD_THREADS / FD_WAVE], next_sh, passes_sh;
  const int tid = threadIdx.x, lane = tid & (FD_WAVE - 1), wave = tid / FD_WAVE, N = a.N, W = (N + 31) / 32;
  const long p = blockIdx.x;
  double *px = tm_sh, *py = px + N, *pz = py + N, *qx = pz + N, *qy = qx + N, *qz = qy + N;
  unsigned* masks = (unsigned*)(qz + N);
  unsigned *cur = masks + tid, *nxt = masks + (size_t)W * FD_THREADS + tid;
  double* red_s = (double*)(masks + (size_t)2 * W * FD_THREADS);
  int* red_seed = (int*)(red_s + FD_THREADS);

  const int ia = a.pairs[2 * p], ib = a.pairs[2 * p + 1];
  const int Sb = a.prot_b ? a.S_b : a.S;
  if (ia < 0 || ia >= a.S || ib < 0 || ib >= Sb) {  // the device data decide what is addressed
    if (tid == 0) {
      a.tm[p] = __builtin_nan(""), a.d0[p] = 0.0, a.n_aligned[p] = 0, a.best_seed[p] = -1, a.passes[p] = 0, a.status[p] = FDIPT_TM_SKIPPED;
      for (int k = 0; k < 9; ++k) a.rotation[p * 9 + k] = (k % 4 == 0) ? 1.0 : 0.0;
      for (int k = 0; k < 3; ++k) a.translation[p * 3 + k] = 0.0;
    }
    return;
  }
  const float *xa = a.prot + ((long)ia * N * a.atoms + a.ca) * 3, *ma = a.mask + (long)ia * N;
  const float *xb = (a.prot_b ? a.prot_b + ((long)ib * N * a.atoms_b + a.ca) * 3 : a.prot + ((long)ib * N * a.atoms + a.ca) * 3);
  const float* mb = (a.prot_b ? a.mask_b : a.mask) + (long)ib * N;
  const long sa = (long)a.atoms * 3, sb = (long)(a.prot_b ? a.atoms_b : a.atoms) * 3;

  // ---- (a) ordered compaction into LDS
  int n = 0;
  for (int n0 = 0; n0 < N; n0 += FD_THREADS) {
    const int i = n0 + tid;
    const bool f = i < N && ma[i] != 0.f && mb[i] != 0.f;
    const unsigned long long bal = __ballot(f);
    if (lane == 0) cnt_sh[wave] = __popcll(bal);
    __syncthreads();
    int off = n, tot = 0;
#pragma unroll
    for (int v = 0; v < FD_THREADS / FD_WAVE; ++v) {
      if (v < wave) off += cnt_sh[v];
      tot += cnt_sh[v];
    }
    if (f) {  // (pos < N: at most one position per row)
      const int pos = off + __popcll(bal & ((1ull << lane) - 1ull));
      const float *u = xa + (long)i * sa, *v = xb + (long)i * sb;
      px[pos] = (double)u[0], py[pos] = (double)u[1], pz[pos] = (double)u[2];
      qx[pos] = (double)v[0], qy[pos] = (double)v[1], qz[pos] = (double)v[2];
    }
    n += tot;
    __syncthreads();
  }
  int L = n;
  if (a.norm_length && a.norm_length[p] > 0) L = a.norm_length[p];
  const double d0 = L > 21 ? 1.24 * cbrt((double)(L - 15)) - 1.8 : 0.5;
  const double d_search = fmin(fmax(d0, 4.5), 8.0), d0sq = d0 * d0;
  if (n < 3) {
    if (tid == 0) {
      a.tm[p] = __builtin_nan(""), a.d0[p] = d0, a.n_aligned[p] = n, a.best_seed[p] = -1, a.passes[p] = 0, a.status[p] = FDIPT_TM_TOO_SHORT;
      for (int k = 0; k < 9; ++k) a.rotation[p * 9 + k] = (k % 4 == 0) ? 1.0 : 0.0;
      for (int k = 0; k < 3; ++k) a.translation[p * 3 + k] = 0.0;
    }
    return;
  }
  // the fragment ladder: n >> k while it exceeds 4, then 4 (n itself below 4); seeds are numbered level-major, start-minor
  int len[TM_LEVELS], first[TM_LEVELS + 1], levels = 0;
  first[0] = 0;
  for (int k = 0; k < 5 && (n >> k) > 4; ++k) {
    len[levels] = n >> k;
    first[levels + 1] = first[levels] + n - len[levels] + 1;
    ++levels;
  }
  len[levels] = n < 4 ? n : 4;
  first[levels + 1] = first[levels] + n - len[levels] + 1;
  ++levels;
  const int n_seeds = first[levels], words = (n + 31) / 32;
  if (tid == 0) next_sh = FD_THREADS, passes_sh = 0;
  __syncthreads();

  // ---- (b) the search
  double best = -1.0, seed_best = -1.0;
  int best_seed = 0x7fffffff, seed = tid, it = 0, my_passes = 0;
  TmTransform T, Tbest;
#pragma unroll
  for (int k = 0; k < 9; ++k) Tbest.R[k] = 0.0;
  Tbest.t[0] = Tbest.t[1] = Tbest.t[2] = 0.0;
  bool fresh = true;
  while (seed < n_seeds) {
    if (fresh) {  // the seed's fragment is the first set
      int lv = 0;
      while (seed >= first[lv + 1]) ++lv;
      const int s0 = seed - first[lv], s1 = s0 + len[lv];  // rows s0 .. s1 - 1
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
        score += d0sq / (d0sq + d2);
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
      seed = atomicAdd(&next_sh, 1);
      fresh = true;
    } else {
      unsigned* t = cur;
      cur = nxt, nxt = t;
    }
  }
  atomicAdd(&passes_sh, my_passes);
  __syncthreads();  // (every thread is done with the masks: the reduction's arrays lie behind them)

  // ---- (c) the first seed that holds the largest score
  red_s[tid] = best, red_seed[tid] = best_seed;
  __syncthreads();
  int owner = 0;
  for (int t = 1; t < FD_THREADS; ++t)
    if (red_s[t] > red_s[owner] || (red_s[t] == red_s[owner] && red_seed[t] < red_seed[owner])) owner = t;
  if (tid == owner) {
    const bool found = best >= 0.0;  // (no seed of a pair with coordinates that are not finite scores)
    a.tm[p] = found ? best / (double)L : __builtin_nan(""), a.d0[p] = d0, a.n_aligned[p] = n, a.best_seed[p] = found ? best_seed : -1;
    a.passes[p] = passes_sh, a.status[p] = found ? 0 : FDIPT_TM_NOT_FINITE;
#pragma unroll
    for (int k = 0; k < 9; ++k) fd_st(a.rotation + p * 9 + k, found ? Tbest.R[k] : (k % 4 == 0 ? 1.0 : 0.0));
#pragma unroll
    for (int k = 0; k < 3; ++k) fd_st(a.translation + p * 3 + k, found ? Tbest.t[k] : 0.0);
  }
}

extern "C" size_t fdipt_sample_tm_score_workspace(int S, int N, int P) {
  (void)S, (void)N, (void)P;  // the search lives in LDS and registers; the entry keeps the argument for a later layout
  return 0;
}

extern "C" int fdipt_sample_tm_score(const FdiptTmArgs* a, fdipt_stream_t stream) {
  if (!a || a->S < 1 || a->N < 1 || a->P < 1 || (a->atoms != 37 && a->atoms != 5) || a->ca < 0 || a->ca >= 5) return FDIPT_EINVAL;
  if (!a->prot || !a->mask || !a->pairs || !a->tm || !a->rotation || !a->translation || !a->n_aligned || !a->d0 || !a->best_seed || !a->passes ||
      !a->status)
    return FDIPT_EINVAL;
  if (a->prot_b && (!a->mask_b || a->S_b < 1 || (a->atoms_b != 37 && a->atoms_b != 5))) return FDIPT_EINVAL;
  if (a->N > TM_MAX_ROWS) return FDIPT_ESIZE;
  if (a->workspace_bytes < fdipt_sample_tm_score_workspace(a->S, a->N, a->P)) return FDIPT_ESIZE;
  const size_t lds = tm_lds_bytes(a->N);
  static FdPerDevice attr_dev;
  const int dev_ = fd_device();
  if (!attr_dev.get(dev_)) {  // N = 1024: 113 KB, more than the default 64 KB of dynamic LDS
    if (hipFuncSetAttribute((const void*)tm_score_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tm_lds_bytes(TM_MAX_ROWS)) != hipSuccess)
      return FDIPT_ELAUNCH;
    attr_dev.set(dev_, 1);
  }
  hipLaunchKernelGGL(tm_score_kernel, dim3((unsigned)a->P), dim3(FD_THREADS), lds, (hipStream_t)stream, *a);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
