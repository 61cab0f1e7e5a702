// tmscore.hip — TM-score of samples on the device (include/fdipt.h, "TM-score"): Zhang & Skolnick's TMscore
// search over seed superpositions for a GIVEN residue correspondence (row i of one structure with row i of the other), for P pairs of
// structures, all in float64.  It is the number the reference takes from tmtools.tm_align where the alignment is the identity (a sample
// against its ground truth or its refold) and a lower bound of it elsewhere (the all-against-all matrix of hierarchy_diversity);
// TM-align's alignment search is not built.
//
// One launch, a block per pair, no workspace traffic:
//   (a) the block compacts the CA atoms of the rows where both masks are set into LDS in ascending row order (ballot + popcount per
//       wave, the four waves' counts through LDS), float32 widened to float64, six arrays of N doubles
//   (b) (tmsearch.hpp, shared with tmalign.hip) every thread owns a seed (fragment length, start) at a time and walks the rows serially: all lanes read the same LDS address
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
#include "tmsearch.hpp"

#define TM_MAX_ROWS FDIPT_TM_MAX_ROWS

__host__ __device__ inline size_t tm_lds_bytes(int N) {
  // six coordinate arrays, then the search's two masks of ceil(N / 32) words per thread and its reduction's score and seed per thread
  return (size_t)6 * N * 8 + tm_search_lds_bytes(N);
}

__global__ __launch_bounds__(FD_THREADS) void tm_score_kernel(FdiptTmArgs a) {
  extern __shared__ double tm_sh[];
  __shared__ int cnt_sh[FD_THREADS / FD_WAVE], next_sh, passes_sh;
  const int tid = threadIdx.x, lane = tid & (FD_WAVE - 1), wave = tid / FD_WAVE, N = a.N, W = (N + 31) / 32;
  const long p = blockIdx.x;
  double *px = tm_sh, *py = px + N, *pz = py + N, *qx = pz + N, *qy = qx + N, *qz = qy + N;
  unsigned* masks = (unsigned*)(qz + N);

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
  // ---- (b), (c) the search over every start (step 1), no d8 cut: tmsearch.hpp
  double best;
  int best_seed;
  TmTransform Tbest;
  if (tm_search(px, py, pz, qx, qy, qz, n, d0sq, d_search, 1, 0.0, masks, W, &next_sh, &passes_sh, best, best_seed, Tbest)) {
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
