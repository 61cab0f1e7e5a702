// gdt.hip — GDT-TS / GDT-HA of samples on the device (include/fdipt.h, "GDT-TS / GDT-HA"): for P pairs (model,
// reference) in row correspondence the number of rows within 0.5, 1, 2, 4 and 8 Angstrom under the identity (NONE: the frame of the
// fixed context, openfold's gdt on the raw coordinates), under one least-squares superposition of all rows (GLOBAL: superimpose, then
// gdt) or, per cutoff, under the best transform a seed search visits (SEARCH), all in float64.
//
// One launch, a block per pair, no workspace traffic.  The compaction and the LDS layout are tmscore.hip's: six coordinate arrays, two
// bit masks per thread, a reduction area - here five (count, item, pass) triples per thread - and behind it the row of every compacted
// position (res_within is indexed by row).
//   SEARCH: a work item is (refinement cutoff k, seed of tmsearch.hpp's ladder, every start), numbered k * n_seeds + seed.  The loop is
//       flat like tm_search's: an iteration is one pass of whatever item the lane holds - superpose the set (tm_superpose), walk the rows
//       once for the five counts and the next set (d^2 < cut^2, cut = c_k, widened as tm_search widens it) - and a lane whose item ends
//       takes the next number from a counter in LDS.  Every pass offers its five counts to the lane's five running maxima.  Five best
//       transforms per thread would be 60 doubles of registers or 122 KB of LDS, so a thread keeps (count, item, pass) only; after one
//       ordered reduction per cutoff (largest count, lowest item, earliest pass) lane j of the block replays the winner of cutoff j to
//       its pass and so obtains its transform.  Which lane serves which item depends on timing; no output does.
//   GLOBAL: thread 0 superposes all rows.  NONE: the identity.
//   Then the whole block walks the rows in parallel under the five transforms: res_within, and in NONE and GLOBAL the counts
//   (ballot + popcount, integer adds in LDS).
// Contraction into fused multiply-adds is off in this unit: the distances are compared with a NumPy evaluation in the same order.
#include "common.hpp"

#pragma clang fp contract(off)

#include "horn.hpp"
#include "tmsearch.hpp"

#define GDT_K FDIPT_GDT_CUTOFFS

__host__ __device__ inline size_t gdt_lds_bytes(int N) {
  // six coordinate arrays, two masks of ceil(N / 32) words per thread, five (count, item, pass) per thread, the row of every position:
  // 134 144 bytes at N = FDIPT_TM_MAX_ROWS (tm_lds_bytes: 117 760), of the 160 KB of a CU
  return (size_t)6 * N * 8 + (size_t)2 * ((N + 31) / 32) * FD_THREADS * 4 + (size_t)FD_THREADS * GDT_K * 3 * 4 + (size_t)N * 4;
}

// the rows of seed `seed` (level-major, start-minor; every start) as the set `cur`
__device__ __forceinline__ void gdt_seed_set(int seed, const int* len, const int* first, int words, unsigned* cur) {
  int lv = 0;
  while (seed >= first[lv + 1]) ++lv;
  const int s0 = seed - first[lv], s1 = s0 + len[lv];  // rows s0 .. s1 - 1
  for (int w = 0; w < words; ++w) {
    const int lo = w * 32, b0 = s0 > lo ? s0 - lo : 0, b1 = s1 - lo < 32 ? s1 - lo : 32;
    unsigned m = 0;
    if (b1 > b0) m = (b1 - b0 == 32 ? 0xffffffffu : ((1u << (b1 - b0)) - 1u)) << b0;
    cur[w * FD_THREADS] = m;
  }
}

// One pass of an item: superpose the set `cur`, form the five counts under the transform and select the rows inside the cut into `nxt`
// in one walk.  Fewer than 3 rows inside: the cut grows by 0.5 until the third smallest distance is inside (tm_search's rule), and the
// walk runs again.  Returns whether the set did not change.
__device__ __forceinline__ bool gdt_pass(const double* px, const double* py, const double* pz, const double* qx, const double* qy, const double* qz, int n,
                                         double cut, const unsigned* cur, unsigned* nxt, TmTransform& T, int (&cnt)[GDT_K]) {
  tm_superpose(px, py, pz, qx, qy, qz, cur, n, T);
  bool same;
  for (;;) {
    const double cut2 = cut * cut;
    int inside = 0;
    unsigned m = 0;
    same = true;
#pragma unroll
    for (int j = 0; j < GDT_K; ++j) cnt[j] = 0;
    for (int i = 0; i < n; ++i) {
      const double d2 = tm_dist2(T, px[i], py[i], pz[i], qx[i], qy[i], qz[i]);
      cnt[0] += d2 <= 0.25, cnt[1] += d2 <= 1.0, cnt[2] += d2 <= 4.0, cnt[3] += d2 <= 16.0, cnt[4] += d2 <= 64.0;
      if (d2 < cut2) m |= 1u << (i & 31), ++inside;
      if ((i & 31) == 31 || i == n - 1) {
        same = same && m == cur[(i >> 5) * FD_THREADS];
        nxt[(i >> 5) * FD_THREADS] = m;
        m = 0;
      }
    }
    if (inside >= 3 || n <= 3 || !(cut < TM_CUT_LIMIT)) break;
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
  return same;
}

// a pair without a result: scores NaN, no counts, the identity, every row of res_within 0 (all threads of the block)
__device__ __forceinline__ void gdt_no_result(const FdiptGdtArgs& a, long p, int n, int status) {
  for (int i = threadIdx.x; i < a.N; i += FD_THREADS) a.res_within[p * a.N + i] = 0;
  if (threadIdx.x == 0) {
    a.gdt_ts[p] = __builtin_nan(""), a.gdt_ha[p] = __builtin_nan(""), a.n_scored[p] = n, a.passes[p] = 0, a.status[p] = status;
    for (int j = 0; j < GDT_K; ++j) {
      a.counts[p * GDT_K + j] = 0, a.best_item[p * GDT_K + j] = -1, a.best_pass[p * GDT_K + j] = -1;
      for (int k = 0; k < 9; ++k) a.rotation[(p * GDT_K + j) * 9 + k] = (k % 4 == 0) ? 1.0 : 0.0;
      for (int k = 0; k < 3; ++k) a.translation[(p * GDT_K + j) * 3 + k] = 0.0;
    }
  }
}

__global__ __launch_bounds__(FD_THREADS) void gdt_kernel(FdiptGdtArgs a) {
  extern __shared__ double gdt_sh[];
  __shared__ int cnt_sh[FD_THREADS / FD_WAVE], next_sh, passes_sh, bad_sh, count_sh[GDT_K], item_sh[GDT_K], pass_sh[GDT_K];
  __shared__ double T_sh[GDT_K][12];
  const int tid = threadIdx.x, lane = tid & (FD_WAVE - 1), wave = tid / FD_WAVE, N = a.N, W = (N + 31) / 32;
  const long p = blockIdx.x;
  double *px = gdt_sh, *py = px + N, *pz = py + N, *qx = pz + N, *qy = qx + N, *qz = qy + N;
  unsigned* masks = (unsigned*)(qz + N);
  int* red = (int*)(masks + (size_t)2 * W * FD_THREADS);  // [3][GDT_K][FD_THREADS]: count, item, pass
  int* row_of = red + 3 * GDT_K * FD_THREADS;

  const int ia = a.pairs[2 * p], ib = a.pairs[2 * p + 1];
  const int Sb = a.prot_b ? a.S_b : a.S;
  if (ia < 0 || ia >= a.S || ib < 0 || ib >= Sb) {  // the device data decide what is addressed
    gdt_no_result(a, p, 0, FDIPT_GDT_SKIPPED);
    return;
  }
  const float *xa = a.prot + ((long)ia * N * a.atoms + a.ca) * 3, *ma = a.mask + (long)ia * N;
  const float *xb = (a.prot_b ? a.prot_b + ((long)ib * N * a.atoms_b + a.ca) * 3 : a.prot + ((long)ib * N * a.atoms + a.ca) * 3);
  const float* mb = (a.prot_b ? a.mask_b : a.mask) + (long)ib * N;
  const long sa = (long)a.atoms * 3, sb = (long)(a.prot_b ? a.atoms_b : a.atoms) * 3;

  if (tid == 0) bad_sh = 0, next_sh = FD_THREADS, passes_sh = 0;
  if (tid < GDT_K) count_sh[tid] = 0, item_sh[tid] = -1, pass_sh[tid] = -1;
  __syncthreads();
  // ---- ordered compaction into LDS (tmscore.hip (a)), with the row of every position
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
      row_of[pos] = i;
      if (!(isfinite(u[0]) && isfinite(u[1]) && isfinite(u[2]) && isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]))) bad_sh = 1;
    } else if (i < N) {
      a.res_within[p * N + i] = 0;
    }
    n += tot;
    __syncthreads();
  }
  if (n < (a.mode == FDIPT_GDT_NONE ? 1 : 3) || bad_sh) {
    gdt_no_result(a, p, n, bad_sh ? FDIPT_GDT_NOT_FINITE : FDIPT_GDT_TOO_SHORT);
    return;
  }
  int L = n;
  if (a.norm_length && a.norm_length[p] > 0) L = a.norm_length[p];

  unsigned *cur = masks + tid, *nxt = masks + (size_t)W * FD_THREADS + tid;
  const int words = (n + 31) / 32;
  TmTransform T;
  if (a.mode == FDIPT_GDT_SEARCH) {
    // the fragment ladder of tm_search with step 1: n >> k while it exceeds 4, then 4 (n itself below 4)
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
    const int n_seeds = first[levels], n_items = GDT_K * n_seeds;

    int bc[GDT_K], bi[GDT_K], bp[GDT_K], cnt[GDT_K];
#pragma unroll
    for (int j = 0; j < GDT_K; ++j) bc[j] = -1, bi[j] = 0x7fffffff, bp[j] = 0;
    int item = tid, it = 0, my_passes = 0;
    double cut = 0.0;
    bool fresh = true;
    while (item < n_items) {
      if (fresh) {  // the seed's fragment is the first set
        gdt_seed_set(item % n_seeds, len, first, words, cur);
        cut = 0.5 * (double)(1 << (item / n_seeds));
        it = 0, fresh = false;
      }
      const bool same = gdt_pass(px, py, pz, qx, qy, qz, n, cut, cur, nxt, T, cnt);
      ++my_passes;
#pragma unroll
      for (int j = 0; j < GDT_K; ++j)
        if (cnt[j] > bc[j] || (cnt[j] == bc[j] && item < bi[j])) bc[j] = cnt[j], bi[j] = item, bp[j] = it;
      ++it;
      if (same || it == TM_MAX_PASSES) {
        item = atomicAdd(&next_sh, 1);
        fresh = true;
      } else {
        unsigned* t = cur;
        cur = nxt, nxt = t;
      }
    }
    atomicAdd(&passes_sh, my_passes);
#pragma unroll
    for (int j = 0; j < GDT_K; ++j) red[j * FD_THREADS + tid] = bc[j], red[(GDT_K + j) * FD_THREADS + tid] = bi[j], red[(2 * GDT_K + j) * FD_THREADS + tid] = bp[j];
    __syncthreads();  // (every thread is done with its masks)
    if (tid < GDT_K) {
      // the winner of cutoff tid: the largest count, the lowest item among equals (an item lives in one thread, which kept its
      // earliest pass), replayed to its pass for the transform
      const int *rc = red + tid * FD_THREADS, *ri = red + (GDT_K + tid) * FD_THREADS, *rp = red + (2 * GDT_K + tid) * FD_THREADS;
      int owner = 0;
      for (int t = 1; t < FD_THREADS; ++t)
        if (rc[t] > rc[owner] || (rc[t] == rc[owner] && ri[t] < ri[owner])) owner = t;
      const int w_item = ri[owner], w_pass = rp[owner];
      cur = masks + tid, nxt = masks + (size_t)W * FD_THREADS + tid;
      gdt_seed_set(w_item % n_seeds, len, first, words, cur);
      cut = 0.5 * (double)(1 << (w_item / n_seeds));
      for (it = 0;; ++it) {
        gdt_pass(px, py, pz, qx, qy, qz, n, cut, cur, nxt, T, cnt);
        if (it == w_pass) break;
        unsigned* t = cur;
        cur = nxt, nxt = t;
      }
      count_sh[tid] = rc[owner], item_sh[tid] = w_item, pass_sh[tid] = w_pass;
#pragma unroll
      for (int k = 0; k < 9; ++k) T_sh[tid][k] = T.R[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) T_sh[tid][9 + k] = T.t[k];
    }
  } else {
    if (tid == 0) {
      if (a.mode == FDIPT_GDT_GLOBAL) {
        for (int w = 0; w < words; ++w) cur[w * FD_THREADS] = (w == words - 1 && (n & 31)) ? (1u << (n & 31)) - 1u : 0xffffffffu;
        tm_superpose(px, py, pz, qx, qy, qz, cur, n, T);
        passes_sh = 1;
      } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) T.R[k] = (k % 4 == 0) ? 1.0 : 0.0;
        T.t[0] = T.t[1] = T.t[2] = 0.0;
      }
      for (int j = 0; j < GDT_K; ++j) {
#pragma unroll
        for (int k = 0; k < 9; ++k) T_sh[j][k] = T.R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) T_sh[j][9 + k] = T.t[k];
      }
    }
  }
  __syncthreads();

  // ---- the rows in parallel under the five transforms: res_within; outside SEARCH the counts
  for (int p0 = 0; p0 < n; p0 += FD_THREADS) {
    const int pos = p0 + tid;
    int bits = 0;
#pragma unroll
    for (int j = 0; j < GDT_K; ++j) {
      bool in = false;
      if (pos < n) {
#pragma unroll
        for (int k = 0; k < 9; ++k) T.R[k] = T_sh[j][k];
#pragma unroll
        for (int k = 0; k < 3; ++k) T.t[k] = T_sh[j][9 + k];
        const double c = 0.5 * (double)(1 << j);
        in = tm_dist2(T, px[pos], py[pos], pz[pos], qx[pos], qy[pos], qz[pos]) <= c * c;
      }
      bits |= (int)in << j;
      if (a.mode != FDIPT_GDT_SEARCH) {
        const unsigned long long bal = __ballot(in);
        if (lane == 0 && bal) atomicAdd(&count_sh[j], __popcll(bal));
      }
    }
    if (pos < n) a.res_within[p * N + row_of[pos]] = bits;
  }
  __syncthreads();
  if (tid < GDT_K) {
    a.counts[p * GDT_K + tid] = count_sh[tid], a.best_item[p * GDT_K + tid] = item_sh[tid], a.best_pass[p * GDT_K + tid] = pass_sh[tid];
    for (int k = 0; k < 9; ++k) fd_st(a.rotation + (p * GDT_K + tid) * 9 + k, T_sh[tid][k]);
    for (int k = 0; k < 3; ++k) fd_st(a.translation + (p * GDT_K + tid) * 3 + k, T_sh[tid][9 + k]);
  }
  if (tid == 0) {
    const double den = 4.0 * (double)L;
    a.gdt_ts[p] = (double)(count_sh[1] + count_sh[2] + count_sh[3] + count_sh[4]) / den;
    a.gdt_ha[p] = (double)(count_sh[0] + count_sh[1] + count_sh[2] + count_sh[3]) / den;
    a.n_scored[p] = n, a.passes[p] = passes_sh, a.status[p] = 0;
  }
}

extern "C" size_t fdipt_sample_gdt_workspace(int S, int N, int P) {
  (void)S, (void)N, (void)P;  // the search lives in LDS and registers; the entry keeps the argument for a later layout
  return 0;
}

extern "C" int fdipt_sample_gdt(const FdiptGdtArgs* a, fdipt_stream_t stream) {
  if (!a || a->S < 1 || a->N < 1 || a->P < 1 || (a->atoms != 37 && a->atoms != 5) || a->ca < 0 || a->ca >= 5) return FDIPT_EINVAL;
  if (a->mode != FDIPT_GDT_NONE && a->mode != FDIPT_GDT_GLOBAL && a->mode != FDIPT_GDT_SEARCH) return FDIPT_EINVAL;
  if (!a->prot || !a->mask || !a->pairs || !a->gdt_ts || !a->gdt_ha || !a->counts || !a->n_scored || !a->rotation || !a->translation || !a->best_item ||
      !a->best_pass || !a->passes || !a->res_within || !a->status)
    return FDIPT_EINVAL;
  if (a->prot_b && (!a->mask_b || a->S_b < 1 || (a->atoms_b != 37 && a->atoms_b != 5))) return FDIPT_EINVAL;
  if (a->N > FDIPT_TM_MAX_ROWS) return FDIPT_ESIZE;
  if (a->workspace_bytes < fdipt_sample_gdt_workspace(a->S, a->N, a->P)) return FDIPT_ESIZE;
  const size_t lds = gdt_lds_bytes(a->N);
  static FdPerDevice attr_dev;
  const int dev_ = fd_device();
  if (!attr_dev.get(dev_)) {  // N = 1024: 131 KB, more than the default 64 KB of dynamic LDS
    if (hipFuncSetAttribute((const void*)gdt_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)gdt_lds_bytes(FDIPT_TM_MAX_ROWS)) != hipSuccess)
      return FDIPT_ELAUNCH;
    attr_dev.set(dev_, 1);
  }
  hipLaunchKernelGGL(gdt_kernel, dim3((unsigned)a->P), dim3(FD_THREADS), lds, (hipStream_t)stream, *a);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
