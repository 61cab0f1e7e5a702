// structsearch.hip — the novelty search (include/fdipt.h, "structure search"): Q queries against a packed,
// ragged set of D CA traces under the alignment search of section 7.9, the top_k entries per query.  The search of a pair is
// tma_pair of tmalign_body.hpp, the body tm_align_kernel runs: a pair's outputs depend on its set rows only, so the scores equal
// fdipt_sample_tm_align's on the same pairs bit for bit, whatever the bucket.
//
// The caller's plan lists the entries bucket by bucket.  On one stream, no host round trip in between:
//   init     every pair's scores NaN, its status 0 (FDIPT_SEARCH_TOO_LONG beyond the row limit), the lists empty, the floors min_score
//   score    per bucket: a block per (query, entry); dynamic LDS tma_layout(N_q, cap of the bucket), not that of the longest entry; the
//            entry comes from the packed array without a mask or an atom stride; scores, n_aligned, rmsd and status only.  With prune the
//            block leaves once it knows n1 and n2 if its length bound lies strictly below the query's floor
//   merge    per bucket, after its score launch: a block per query selects the top_k of (the list held, the bucket's scores) in the total
//            order (ranked score descending, entry ascending) by top_k ordered arg-max rounds, and sets the floor.  No atomics on
//            doubles, nothing depends on block scheduling
//   finish   a block per query: the hits' numbers gathered from the pair arrays, the counts from the statuses
//   detail   a block per hit with every output of the body on
// fdipt_structure_search_inits with FDIPT_TMA_INITS_ALL: the score and detail launches are ss_score5_kernel and ss_detail5_kernel, the same blocks with the body's
// INITS5 switch on, and the workspace's init_tm and init_dp hold five entries per hit.
// Contraction into fused multiply-adds is off in this unit, as in tmalign.hip.
#include "common.hpp"

#pragma clang fp contract(off)

#include "horn.hpp"
#include "tmsearch.hpp"
#include "tmalign_body.hpp"

#define SS_MAX_K FDIPT_SEARCH_MAX_K

// the workspace: the ranked scores of the lists [Q,k], the floors [Q]; with details what the body writes and the entry does not return
struct SsWork {
  size_t top_score, floor, tm, rmsd, d0_a, d0_b, init_tm, n_aligned, status, init_dp, total;
};
static inline SsWork ss_work(int Q, int k, int details, int inits = 3) {
  SsWork w;
  const size_t qk = (size_t)Q * k;
  size_t o = 0;
  w.top_score = o, o += qk * 8;
  w.floor = o, o += (size_t)Q * 8;
  w.tm = w.rmsd = w.d0_a = w.d0_b = w.init_tm = w.n_aligned = w.status = w.init_dp = o;
  if (details) {
    w.tm = o, o += qk * 8;
    w.rmsd = o, o += qk * 8;
    w.d0_a = o, o += qk * 8;
    w.d0_b = o, o += qk * 8;
    w.init_tm = o, o += qk * inits * 8;
    w.n_aligned = o, o += qk * 4;
    w.status = o, o += qk * 4;
    w.init_dp = o, o += qk * inits * 4;
  }
  w.total = (o + 7) / 8 * 8;
  return w;
}

__global__ __launch_bounds__(FD_THREADS) void ss_init_kernel(FdiptSearchArgs a, double* top_score, double* floor) {
  const double nan = __builtin_nan("");
  const long pairs = (long)a.Q * a.D, step = (long)gridDim.x * FD_THREADS;
  for (long i = (long)blockIdx.x * FD_THREADS + threadIdx.x; i < pairs; i += step) {
    const int e = (int)(i % a.D);
    const long rows = a.db_offsets[e + 1] - a.db_offsets[e];
    a.scores_q[i] = a.scores_t[i] = a.pair_rmsd[i] = nan, a.pair_n_aligned[i] = 0;
    a.pair_status[i] = rows > FDIPT_TMA_MAX_ROWS ? FDIPT_SEARCH_TOO_LONG : 0;
    if (i < (long)a.Q * a.top_k) a.hit[i] = -1, top_score[i] = nan;
    if (i < a.Q) floor[i] = a.min_score;
  }
  // (Q x top_k may exceed Q x D: top_k beyond the number of entries)
  for (long i = pairs + (long)blockIdx.x * FD_THREADS + threadIdx.x; i < (long)a.Q * a.top_k; i += step) a.hit[i] = -1, top_score[i] = nan;
}

// the length bound of a pair against the query's floor
struct SsBound {
  const double* floor;
  int rank_by, prune;
  __device__ __forceinline__ int operator()(int n1, int n2) const {
    if (!prune) return 0;
    const double m = (double)(n1 < n2 ? n1 : n2), bound = rank_by == FDIPT_SEARCH_RANK_TARGET ? m / (double)n2 : m / (double)n1;
    return bound < *floor ? FDIPT_SEARCH_PRUNED : 0;
  }
};

template <bool INITS5>
__device__ __forceinline__ void ss_score_block(const FdiptSearchArgs& a, const double* floor, int start, int count, int cap) {
  extern __shared__ double tma_sh[];
  __shared__ int cnt_sh[FD_THREADS / FD_WAVE], next_sh, passes_sh, count_sh;
  const int q = blockIdx.x / count, e = a.plan_entries[start + blockIdx.x % count];
  if (q >= a.Q || e < 0 || e >= a.D) return;  // the device data decide what is addressed
  const long p = (long)q * a.D + e;
  const TmaOut o{nullptr, a.scores_q, a.scores_t, nullptr, nullptr, a.pair_rmsd, nullptr, nullptr, nullptr, nullptr, a.pair_n_aligned, nullptr, nullptr, a.pair_status, 0};
  const long r0 = a.db_offsets[e], r1 = a.db_offsets[e + 1];
  if (r0 < 0 || r1 < r0 || r1 > a.R || r1 - r0 > cap) {
    tma_leave<false>(o, p, FDIPT_TMA_SKIPPED, 0, 0.0, 0.0, -1);
    return;
  }
  const TmaSource A{a.prot + ((long)q * a.N_q * a.atoms + a.ca) * 3, a.mask + (long)q * a.N_q, (long)a.atoms * 3, a.N_q};
  const TmaSource B{a.db_ca + r0 * 3, nullptr, 3, (int)(r1 - r0)};
  tma_pair<false, false, INITS5>(A, B, a.N_q, cap, o, p, tma_sh, cnt_sh, &next_sh, &passes_sh, &count_sh, SsBound{floor + q, a.rank_by, a.prune});
}

__global__ __launch_bounds__(FD_THREADS) void ss_score_kernel(FdiptSearchArgs a, const double* floor, int start, int count, int cap) {
  ss_score_block<false>(a, floor, start, count, cap);
}
__global__ __launch_bounds__(FD_THREADS) void ss_score5_kernel(FdiptSearchArgs a, const double* floor, int start, int count, int cap) {
  ss_score_block<true>(a, floor, start, count, cap);
}

// (s, e) ranks before (t, f): the order of the hits
__device__ __forceinline__ bool ss_before(double s, int e, double t, int f) { return s > t || (s == t && e < f); }

__global__ __launch_bounds__(FD_THREADS) void ss_merge_kernel(FdiptSearchArgs a, double* top_score, double* floor, int start, int count) {
  __shared__ double old_s[SS_MAX_K], new_s[SS_MAX_K], red_s[FD_THREADS];
  __shared__ int old_e[SS_MAX_K], new_e[SS_MAX_K], red_e[FD_THREADS];
  const int tid = threadIdx.x, q = blockIdx.x, k = a.top_k;
  const double* ranked = (a.rank_by == FDIPT_SEARCH_RANK_TARGET ? a.scores_t : a.scores_q) + (long)q * a.D;
  if (tid < k) old_s[tid] = top_score[(long)q * k + tid], old_e[tid] = a.hit[(long)q * k + tid], new_s[tid] = __builtin_nan(""), new_e[tid] = -1;
  __syncthreads();
  double prev_s = 1.0 / 0.0;
  int prev_e = -1;
  for (int r = 0; r < k; ++r) {  // round r: the best candidate that ranks strictly behind round r - 1's
    double best_s = 0.0;
    int best_e = -1;
    for (int i = tid; i < count + k; i += FD_THREADS) {
      double s;
      int e;
      if (i < count) {
        e = a.plan_entries[start + i];
        if (e < 0 || e >= a.D) continue;
        s = ranked[e];
        if (!(s >= a.min_score)) continue;  // (NaN never ranks)
      } else {
        e = old_e[i - count], s = old_s[i - count];
        if (e < 0) continue;
      }
      if (ss_before(prev_s, prev_e, s, e) && (best_e < 0 || ss_before(s, e, best_s, best_e))) best_s = s, best_e = e;
    }
    red_s[tid] = best_s, red_e[tid] = best_e;
    __syncthreads();
    for (int h = FD_THREADS / 2; h > 0; h >>= 1) {
      if (tid < h && red_e[tid + h] >= 0 && (red_e[tid] < 0 || ss_before(red_s[tid + h], red_e[tid + h], red_s[tid], red_e[tid])))
        red_s[tid] = red_s[tid + h], red_e[tid] = red_e[tid + h];
      __syncthreads();
    }
    prev_s = red_s[0], prev_e = red_e[0];
    __syncthreads();  // (red is written again in the next round)
    if (prev_e < 0) break;
    if (tid == 0) new_s[r] = prev_s, new_e[r] = prev_e;
  }
  __syncthreads();
  if (tid < k) top_score[(long)q * k + tid] = new_s[tid], a.hit[(long)q * k + tid] = new_e[tid];
  if (tid == 0) floor[q] = new_e[k - 1] >= 0 ? fmax(a.min_score, new_s[k - 1]) : a.min_score;
}

__global__ __launch_bounds__(FD_THREADS) void ss_finish_kernel(FdiptSearchArgs a, const double* top_score) {
  __shared__ int counts[3];
  const int tid = threadIdx.x, q = blockIdx.x, k = a.top_k;
  if (tid < 3) counts[tid] = 0;
  __syncthreads();
  int pruned = 0, skipped = 0, scored = 0;
  for (int e = tid; e < a.D; e += FD_THREADS) {
    const int st = a.pair_status[(long)q * a.D + e];
    const bool ran = !(st & (FDIPT_SEARCH_PRUNED | FDIPT_SEARCH_TOO_LONG)) && (st != 0 || a.scores_t[(long)q * a.D + e] == a.scores_t[(long)q * a.D + e]);
    pruned += (st & FDIPT_SEARCH_PRUNED) != 0, skipped += (st & FDIPT_SEARCH_TOO_LONG) != 0, scored += ran;
  }
  atomicAdd(&counts[0], scored), atomicAdd(&counts[1], pruned), atomicAdd(&counts[2], skipped);
  __syncthreads();
  if (tid == 0) a.n_scored[q] = counts[0], a.n_pruned[q] = counts[1], a.n_skipped[q] = counts[2], a.pdb_tm[q] = top_score[(long)q * k];
  if (tid < k) {
    const long p = (long)q * k + tid;
    const int e = a.hit[p];
    const long s = (long)q * a.D + (e < 0 ? 0 : e);
    const double nan = __builtin_nan("");
    a.tm_q[p] = e < 0 ? nan : a.scores_q[s], a.tm_t[p] = e < 0 ? nan : a.scores_t[s], a.rmsd[p] = e < 0 ? nan : a.pair_rmsd[s];
    a.n_aligned[p] = e < 0 ? 0 : a.pair_n_aligned[s], a.status[p] = e < 0 ? 0 : a.pair_status[s];
  }
}

template <bool INITS5>
__device__ __forceinline__ void ss_detail_block(const FdiptSearchArgs& a, const TmaOut& o) {
  extern __shared__ double tma_sh[];
  __shared__ int cnt_sh[FD_THREADS / FD_WAVE], next_sh, passes_sh, count_sh;
  const long p = blockIdx.x;
  const int q = (int)(p / a.top_k), e = a.hit[p], cap = a.detail_cap;
  tma_clear<true, INITS5>(o, p, cap);
  if (e < 0 || e >= a.D) {  // no hit: NaN scores, the identity, nothing aligned
    tma_leave<true>(o, p, 0, 0, 0.0, 0.0, -1);
    return;
  }
  const long r0 = a.db_offsets[e], r1 = a.db_offsets[e + 1];
  if (r0 < 0 || r1 < r0 || r1 > a.R || r1 - r0 > cap) {
    tma_leave<true>(o, p, FDIPT_TMA_SKIPPED, 0, 0.0, 0.0, -1);
    return;
  }
  const TmaSource A{a.prot + ((long)q * a.N_q * a.atoms + a.ca) * 3, a.mask + (long)q * a.N_q, (long)a.atoms * 3, a.N_q};
  const TmaSource B{a.db_ca + r0 * 3, nullptr, 3, (int)(r1 - r0)};
  tma_pair<true, false, INITS5>(A, B, a.N_q, cap, o, p, tma_sh, cnt_sh, &next_sh, &passes_sh, &count_sh, TmaNoEarly());
}

__global__ __launch_bounds__(FD_THREADS) void ss_detail_kernel(FdiptSearchArgs a, TmaOut o) { ss_detail_block<false>(a, o); }
__global__ __launch_bounds__(FD_THREADS) void ss_detail5_kernel(FdiptSearchArgs a, TmaOut o) { ss_detail_block<true>(a, o); }

extern "C" size_t fdipt_structure_search_workspace(int Q, int top_k, int details) {
  if (Q < 1 || top_k < 1) return 0;
  return ss_work(Q, top_k, details, 5).total;  // (sized for either mode: 32 bytes per hit more than the default needs)
}

extern "C" int fdipt_structure_search_inits(const FdiptSearchArgs* a, int32_t inits, fdipt_stream_t stream) {
  if (!a || a->Q < 1 || a->N_q < 1 || a->D < 1 || (a->atoms != 37 && a->atoms != 5) || a->ca < 0 || a->ca >= 5) return FDIPT_EINVAL;
  if (a->top_k < 1 || a->top_k > SS_MAX_K || (a->rank_by != FDIPT_SEARCH_RANK_QUERY && a->rank_by != FDIPT_SEARCH_RANK_TARGET) || a->n_buckets < 0 || a->R < 0)
    return FDIPT_EINVAL;
  if (!a->prot || !a->mask || !a->db_ca || !a->db_offsets || !a->hit || !a->tm_q || !a->tm_t || !a->n_aligned || !a->rmsd || !a->status || !a->n_scored ||
      !a->n_pruned || !a->n_skipped || !a->pdb_tm || !a->scores_q || !a->scores_t || !a->pair_n_aligned || !a->pair_rmsd || !a->pair_status)
    return FDIPT_EINVAL;
  if (a->n_buckets > 0 && (!a->plan_entries || !a->bucket_start || !a->bucket_cap || a->bucket_start[0] != 0)) return FDIPT_EINVAL;
  for (int b = 0; b < a->n_buckets; ++b)
    if (a->bucket_start[b + 1] < a->bucket_start[b] || a->bucket_cap[b] < 1 || a->bucket_cap[b] > TMA_MAX_ROWS) return FDIPT_EINVAL;
  if (a->details && (!a->detail_tm_q || !a->detail_tm_t || !a->rotation || !a->translation || !a->alignment || !a->best_init || a->detail_cap < 1 ||
                     a->detail_cap > TMA_MAX_ROWS))
    return FDIPT_EINVAL;
  if (inits != FDIPT_TMA_INITS_DEFAULT && inits != FDIPT_TMA_INITS_ALL) return FDIPT_EINVAL;
  if (a->N_q > TMA_MAX_ROWS) return FDIPT_ESIZE;
  const bool five = inits == FDIPT_TMA_INITS_ALL;
  const long limit = 0x7fffffffL;
  if ((long)a->Q * a->D >= limit || (a->details && (long)a->Q * a->top_k * a->detail_cap >= limit)) return FDIPT_ESIZE;
  for (int b = 0; b < a->n_buckets; ++b)
    if ((long)a->Q * (a->bucket_start[b + 1] - a->bucket_start[b]) >= limit) return FDIPT_ESIZE;
  const SsWork w = ss_work(a->Q, a->top_k, a->details, five ? 5 : 3);
  if (!a->workspace || a->workspace_bytes < fdipt_structure_search_workspace(a->Q, a->top_k, a->details)) return FDIPT_ESIZE;
  static FdPerDevice attr_dev;
  const int dev_ = fd_device();
  if (!attr_dev.get(dev_)) {  // up to 131 KB, more than the default 64 KB of dynamic LDS
    const int most = (int)tma_layout(TMA_MAX_ROWS, TMA_MAX_ROWS).total, most5 = (int)tma_layout(TMA_MAX_ROWS, TMA_MAX_ROWS, true).total;
    if (hipFuncSetAttribute((const void*)ss_score_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, most) != hipSuccess ||
        hipFuncSetAttribute((const void*)ss_detail_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, most) != hipSuccess ||
        hipFuncSetAttribute((const void*)ss_score5_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, most5) != hipSuccess ||
        hipFuncSetAttribute((const void*)ss_detail5_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, most5) != hipSuccess)
      return FDIPT_ELAUNCH;
    attr_dev.set(dev_, 1);
  }
  hipStream_t st = (hipStream_t)stream;
  char* work = (char*)a->workspace;
  double *top_score = (double*)(work + w.top_score), *floor = (double*)(work + w.floor);
  const long cells = (long)a->Q * (a->D > a->top_k ? a->D : a->top_k);
  const unsigned init_blocks = (unsigned)((cells + FD_THREADS - 1) / FD_THREADS < 4096 ? (cells + FD_THREADS - 1) / FD_THREADS : 4096);
  hipLaunchKernelGGL(ss_init_kernel, dim3(init_blocks), dim3(FD_THREADS), 0, st, *a, top_score, floor);
  FD_CHECK_LAUNCH();
  for (int b = 0; b < a->n_buckets; ++b) {
    const int start = a->bucket_start[b], count = a->bucket_start[b + 1] - start, cap = a->bucket_cap[b];
    if (count == 0) continue;
    const dim3 grid((unsigned)((long)a->Q * count));
    const size_t lds = tma_layout(a->N_q, cap, five).total;
    if (five) hipLaunchKernelGGL(ss_score5_kernel, grid, dim3(FD_THREADS), lds, st, *a, (const double*)floor, start, count, cap);
    else hipLaunchKernelGGL(ss_score_kernel, grid, dim3(FD_THREADS), lds, st, *a, (const double*)floor, start, count, cap);
    FD_CHECK_LAUNCH();
    hipLaunchKernelGGL(ss_merge_kernel, dim3((unsigned)a->Q), dim3(FD_THREADS), 0, st, *a, top_score, floor, start, count);
    FD_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(ss_finish_kernel, dim3((unsigned)a->Q), dim3(FD_THREADS), 0, st, *a, (const double*)top_score);
  FD_CHECK_LAUNCH();
  if (a->details) {
    const TmaOut o{(double*)(work + w.tm), a->detail_tm_q, a->detail_tm_t, a->rotation, a->translation, (double*)(work + w.rmsd), (double*)(work + w.d0_a),
                   (double*)(work + w.d0_b), (double*)(work + w.init_tm), a->alignment, (int*)(work + w.n_aligned), (int*)(work + w.init_dp), a->best_init,
                   (int*)(work + w.status), a->detail_cap};
    const dim3 grid((unsigned)((long)a->Q * a->top_k));
    const size_t lds = tma_layout(a->N_q, a->detail_cap, five).total;
    if (five) hipLaunchKernelGGL(ss_detail5_kernel, grid, dim3(FD_THREADS), lds, st, *a, o);
    else hipLaunchKernelGGL(ss_detail_kernel, grid, dim3(FD_THREADS), lds, st, *a, o);
    FD_CHECK_LAUNCH();
  }
  return FDIPT_OK;
}

extern "C" int fdipt_structure_search(const FdiptSearchArgs* a, fdipt_stream_t stream) {
  return fdipt_structure_search_inits(a, FDIPT_TMA_INITS_DEFAULT, stream);
}
