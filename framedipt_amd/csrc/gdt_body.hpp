// gdt_body.hpp — the kernel of the GDT entries as a device function with a MAPPED switch: gdt.hip instantiates it for structures in row
// correspondence (fdipt_sample_gdt, whose top comment describes the kernel), gdt_mapped.hip for a model read through a row map
// (fdipt_sample_gdt_mapped).  MAPPED: the block first gives the verdict on its pair's map (rowmap.hpp); the compaction at load walks the
// reference's rows j and reads the model's row map[j]; everything behind the load is the same code.  The un-mapped instantiation
// compiles to what it was before the switch existed.
#pragma once
#include "rowmap.hpp"

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

// the LDS of the map's verdict in the MAPPED instantiation: a bit per model row, the verdict, the number of existing reference rows
template <bool MAPPED>
__device__ __forceinline__ unsigned* gdt_map_lds() {
  if constexpr (MAPPED) {
    __shared__ unsigned map_sh[FDIPT_TM_MAX_ROWS / 32 + 2];
    return map_sh;
  } else {
    return nullptr;
  }
}
// a MAPPED pair without a result has no counts of rows either
template <bool MAPPED>
__device__ __forceinline__ void gdt_map_counts(const FdiptRowMap& m, long p, int covered, int reference) {
  if constexpr (MAPPED) {
    if (threadIdx.x == 0) m.n_covered[p] = covered, m.n_reference[p] = reference;
  }
}

template <bool MAPPED>
__device__ __forceinline__ void gdt_body(const FdiptGdtArgs& a, const FdiptRowMap& m) {
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
    gdt_map_counts<MAPPED>(m, p, 0, 0);
    return;
  }
  const int Na = MAPPED ? m.N_a : N;  // the model's rows
  const float *xa = a.prot + ((long)ia * Na * a.atoms + a.ca) * 3, *ma = a.mask + (long)ia * Na;
  const float *xb = (a.prot_b ? a.prot_b + ((long)ib * N * a.atoms_b + a.ca) * 3 : a.prot + ((long)ib * N * a.atoms + a.ca) * 3);
  const float* mb = (a.prot_b ? a.mask_b : a.mask) + (long)ib * N;
  const long sa = (long)a.atoms * 3, sb = (long)(a.prot_b ? a.atoms_b : a.atoms) * 3;

  if (tid == 0) bad_sh = 0, next_sh = FD_THREADS, passes_sh = 0;
  if (tid < GDT_K) count_sh[tid] = 0, item_sh[tid] = -1, pass_sh[tid] = -1;
  __syncthreads();
  const int* mp = nullptr;
  unsigned* map_sh = gdt_map_lds<MAPPED>();
  int* ref_sh = MAPPED ? (int*)map_sh + FDIPT_TM_MAX_ROWS / 32 + 1 : nullptr;
  if constexpr (MAPPED) {  // the verdict on the pair's map, the same in every thread
    mp = m.map + p * N;
    if (tid == 0) *ref_sh = 0;
    const int verdict = fd_map_check(mp, N, Na, map_sh, (int*)map_sh + FDIPT_TM_MAX_ROWS / 32);
    if (verdict) {
      gdt_no_result(a, p, 0, verdict);
      gdt_map_counts<MAPPED>(m, p, 0, 0);
      return;
    }
  }
  // ---- ordered compaction into LDS (tmscore.hip (a)), with the row of every position
  int n = 0;
  for (int n0 = 0; n0 < N; n0 += FD_THREADS) {
    const int i = n0 + tid;
    bool f;
    int ri = i;  // the model's row of row i
    if constexpr (MAPPED) {
      const bool ex = i < N && mb[i < N ? i : 0] != 0.f;
      if (ex) ri = fd_map_row(mp, ma, Na, i);
      f = ex && ri >= 0;
      const unsigned long long be = __ballot(ex);
      if (lane == 0 && be) atomicAdd(ref_sh, __popcll(be));
    } else {
      f = i < N && ma[i] != 0.f && mb[i] != 0.f;
    }
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
      const float *u = xa + (long)ri * sa, *v = xb + (long)i * sb;
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
    if constexpr (MAPPED) gdt_map_counts<MAPPED>(m, p, n, *ref_sh);
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
  if constexpr (MAPPED) gdt_map_counts<MAPPED>(m, p, n, *ref_sh);
}

