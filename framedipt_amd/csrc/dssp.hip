// dssp.hip — secondary structure of samples on the device (include/fdipt.h, "secondary structure"): Kabsch &
// Sander's hydrogen-bond patterns in the simplified alphabet coil / helix / strand, the numbers the reference takes from
// md.compute_dssp(traj, simplified=True) (framedipt/analysis/metrics.py:calc_mdtraj_metrics), for B samples, all in float64.
//
// One launch, a block per sample, the phases separated by __syncthreads; per-row data lives in the workspace, not in LDS:
//   (0) the rows that exist are compacted in order by wave 0 (ballot + popcount); N, CA, C, O widened to float64; breaks, their
//       running count, the amide hydrogen
//   (1) a thread per donor scans its acceptors in ascending index and keeps the two slots (strict <: the lower index wins a tie)
//   (2) turn bits per row
//   (3) a thread per row i: every bridge (i, j) holds a hydrogen bond whose donor is i or i + 1 and whose acceptor is j - 1 or j, so
//       the pair test runs over the <= DS_SLOTS candidates the two slots of these donors name, and the bridges of row i are kept in
//       fixed slots, ascending in j.  No atomics, no order that depends on timing.
//   (4) thread 0: ladders (maximal diagonal runs, found from their first bridge) in the order (first i, first j, type, last j), then
//       the greedy bulge pass; a merged-away ladder is marked dead.  The inner loop stops at the first B that starts 6 or more rows
//       past A's end: the list ascends in first i and A's end only grows by merging.
//   (5) strand, alpha, 3-10, pi in this order, each one parallel decision on the state the phase before left
//   (6) counts (integers), fractions, the outputs at the original row indices
// Contraction into fused multiply-adds is off in this unit: the energies are compared bit for bit with a NumPy evaluation.
#include "common.hpp"

#pragma clang fp contract(off)

#define DS_SLOTS FDIPT_DSSP_BRIDGES_PER_ROW
#define DS_Q (-27.888)    // kcal/mol: 332 x 0.42 x 0.20
#define DS_E_MIN (-9.9)
#define DS_E_BOND (-0.5)
#define DS_CA_CUTOFF 9.0
#define DS_BREAK_CN 2.5
#define DS_D_MIN 0.5
#define DS_PARALLEL 1
#define DS_ANTI 2
// per-row state of phase 5
#define DS_NONE 0
#define DS_E 2
#define DS_ALPHA 3
#define DS_310 4
#define DS_PI 5

// the workspace of one sample: doubles, then ints, then bytes
struct DsWs {
  double* x;             // [N][15]: N, CA, C, O, H of the compacted rows
  double* en;            // [N][2]: the two slots' energies (0: empty)
  int* acc;              // [N][2]: their acceptors, compacted indices (-1: empty)
  int* map;              // [N]: compacted row -> row of the input
  int* before;           // [N + 2]: before[k] = breaks before the rows < k
  int* nbr;              // [N]: bridges (k, .) of row k
  int* bridge;           // [N][DS_SLOTS]: j * 4 + type, ascending
  int* lad;              // [DS_SLOTS N][5]: type (0: merged away), ib, ie, jb, je
  unsigned char* flag;   // [N]: the row of the input exists; then: a break before the compacted row
  unsigned char* turn;   // [N]: bit m - 3 = turn_m
  unsigned char* state;  // [N]
};
__host__ __device__ inline size_t ds_doubles(size_t N) { return 17 * N; }
__host__ __device__ inline size_t ds_ints(size_t N) { return (5 + 6 * (size_t)DS_SLOTS) * N + 2; }
__host__ __device__ inline size_t ds_stride(size_t N) { return (ds_doubles(N) * 8 + ds_ints(N) * 4 + 3 * N + 7) / 8 * 8; }
__device__ __forceinline__ DsWs ds_ws(void* base, int b, int N) {
  DsWs w;
  const size_t n = (size_t)N;
  w.x = (double*)((char*)base + (size_t)b * ds_stride(n));
  w.en = w.x + 15 * n;
  w.acc = (int*)(w.en + 2 * n);
  w.map = w.acc + 2 * n;
  w.before = w.map + n;
  w.nbr = w.before + n + 2;
  w.bridge = w.nbr + n;
  w.lad = w.bridge + DS_SLOTS * n;
  w.flag = (unsigned char*)(w.lad + 5 * DS_SLOTS * n);
  w.turn = w.flag + n;
  w.state = w.turn + n;
  return w;
}

__device__ __forceinline__ double ds_dist(const double* p, const double* q) {
  const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
  return sqrt(dx * dx + dy * dy + dz * dz);
}
// HB(d, a): a is one of d's two acceptors and its energy is below -0.5; d, a any integers
__device__ __forceinline__ bool ds_hb(const DsWs& w, int n, int d, int a) {
  if (d < 0 || d >= n || a < 0) return false;
  return (w.acc[2 * (long)d] == a && w.en[2 * (long)d] < DS_E_BOND) || (w.acc[2 * (long)d + 1] == a && w.en[2 * (long)d + 1] < DS_E_BOND);
}
// rows a..b follow each other: none of the rows a + 1 .. b has a break before it (0 <= a <= b < n)
__device__ __forceinline__ bool ds_unbroken(const DsWs& w, int a, int b) { return w.before[b + 1] == w.before[a + 1]; }
// the bridge type of the pair (i, j), 1 <= i, i + 3 <= j <= n - 2, both with unbroken neighbours; parallel wins
__device__ __forceinline__ int ds_bridge_type(const DsWs& w, int n, int i, int j) {
  if ((ds_hb(w, n, i + 1, j) && ds_hb(w, n, j, i - 1)) || (ds_hb(w, n, j + 1, i) && ds_hb(w, n, i, j - 1))) return DS_PARALLEL;
  if ((ds_hb(w, n, i + 1, j - 1) && ds_hb(w, n, j + 1, i - 1)) || (ds_hb(w, n, j, i) && ds_hb(w, n, i, j))) return DS_ANTI;
  return 0;
}
__device__ __forceinline__ bool ds_is_bridge(const DsWs& w, int n, int i, int j, int type) {
  if (i < 0 || i >= n || j < 0 || j >= n) return false;
  const int cnt = w.nbr[i], key = j * 4 + type;
  for (int s = 0; s < cnt; ++s)
    if (w.bridge[(long)i * DS_SLOTS + s] == key) return true;
  return false;
}
// (jb, type, je) of one ladder before those of another: the order inside one first i
__device__ __forceinline__ bool ds_ladder_before(const int* p, const int* q) {
  if (p[3] != q[3]) return p[3] < q[3];
  if (p[0] != q[0]) return p[0] < q[0];
  return p[4] < q[4];
}

__global__ __launch_bounds__(FD_THREADS) void dssp_kernel(FdiptDsspArgs a) {
  __shared__ int n_sh, listed_sh, ladders_sh, status_sh, count_sh[4];  // count_sh: helix, strand, hydrogen bonds, bridges
  const int tid = threadIdx.x, lane = tid & (FD_WAVE - 1), N = a.N, b = blockIdx.x;
  const long row0 = (long)b * N;
  const DsWs w = ds_ws(a.workspace, b, N);
  const int atom_of[4] = {0, 1, 2, 4};  // N, CA, C, O in atom37 columns

  // (0) rows that exist, compacted in order
  if (tid < 4) count_sh[tid] = 0;
  if (tid == 0) status_sh = 0, ladders_sh = 0;
  for (int r = tid; r < N; r += FD_THREADS) {
    const float* p = a.prot + (row0 + r) * (long)a.atoms * 3;
    bool ex = a.res_mask[row0 + r] != 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float* q = p + 3 * atom_of[k];
      ex = ex && (q[0] != 0.f || q[1] != 0.f || q[2] != 0.f);
    }
    w.flag[r] = ex;
  }
  __syncthreads();
  if (tid < FD_WAVE) {
    int offset = 0;
    for (int base = 0; base < N; base += FD_WAVE) {
      const int r = base + lane;
      const bool f = r < N && w.flag[r];
      const unsigned long long mask = __ballot(f);
      if (f) w.map[offset + __popcll(mask & ((1ull << lane) - 1ull))] = r;
      offset += __popcll(mask);
    }
    if (lane == 0) n_sh = offset;
  }
  __syncthreads();
  const int n = n_sh;
  for (int k = tid; k < n; k += FD_THREADS) {
    const float* p = a.prot + (row0 + w.map[k]) * (long)a.atoms * 3;
#pragma unroll
    for (int c = 0; c < 12; ++c) w.x[(long)k * 15 + c] = (double)p[3 * atom_of[c / 3] + c % 3];
  }
  __syncthreads();
  for (int k = tid; k < n; k += FD_THREADS) {
    double* x = w.x + (long)k * 15;
    bool brk = k == 0;
    if (!brk) {
      const double* prev = x - 15;
      brk = a.chain_idx[row0 + w.map[k]] != a.chain_idx[row0 + w.map[k - 1]] || ds_dist(prev + 6, x) > DS_BREAK_CN;
      if (!brk) {  // H = N + (C - O) / |C - O| of the row before
        const double cx = prev[6] - prev[9], cy = prev[7] - prev[10], cz = prev[8] - prev[11];
        const double len = sqrt(cx * cx + cy * cy + cz * cz);
        x[12] = x[0] + cx / len;
        x[13] = x[1] + cy / len;
        x[14] = x[2] + cz / len;
      }
    }
    if (brk) x[12] = x[0], x[13] = x[1], x[14] = x[2];
    w.flag[k] = brk;  // (flag[k] as "row k of the input exists" was last read before the barrier above; k < n <= N)
  }
  __syncthreads();
  if (tid < FD_WAVE) {
    int offset = 0;
    if (lane == 0) w.before[0] = 0;
    for (int base = 0; base < n; base += FD_WAVE) {
      const int k = base + lane;
      const bool f = k < n && w.flag[k];
      const unsigned long long mask = __ballot(f);
      if (k < n) w.before[k + 1] = offset + __popcll(mask & ((2ull << lane) - 1ull));
      offset += __popcll(mask);
    }
  }
  __syncthreads();

  // (1) the two best acceptors of every donor
  for (int d = tid; d < n; d += FD_THREADS) {
    int a0 = -1, a1 = -1;
    double e0 = 0.0, e1 = 0.0;
    if (a.is_proline[row0 + w.map[d]] == 0) {
      double xd[15];
#pragma unroll
      for (int c = 0; c < 15; ++c) xd[c] = w.x[(long)d * 15 + c];
      for (int j = 0; j < n; ++j) {
        if (j == d || j == d - 1) continue;
        const double* xa = w.x + (long)j * 15;
        if (!(ds_dist(xd + 3, xa + 3) < DS_CA_CUTOFF)) continue;
        const double d_ho = ds_dist(xd + 12, xa + 9), d_hc = ds_dist(xd + 12, xa + 6), d_nc = ds_dist(xd, xa + 6), d_no = ds_dist(xd, xa + 9);
        double e;
        if (fmin(fmin(d_ho, d_hc), fmin(d_nc, d_no)) < DS_D_MIN) {
          e = DS_E_MIN;
        } else {
          e = DS_Q * (((1.0 / d_ho - 1.0 / d_hc) + 1.0 / d_nc) - 1.0 / d_no);
          e = round(e * 1000.0) / 1000.0;
          if (e < DS_E_MIN) e = DS_E_MIN;
        }
        if (e < e0) {
          a1 = a0, e1 = e0;
          a0 = j, e0 = e;
        } else if (e < e1) {
          a1 = j, e1 = e;
        }
      }
    }
    w.acc[2 * (long)d] = a0, w.acc[2 * (long)d + 1] = a1;
    w.en[2 * (long)d] = e0, w.en[2 * (long)d + 1] = e1;
  }
  __syncthreads();

  // (2) turns, (3) the bridges of every row; the state of phase 5 starts empty
  for (int i = tid; i < n; i += FD_THREADS) {
    unsigned char bits = 0;
#pragma unroll
    for (int m = 3; m <= 5; ++m)
      if (i + m < n && ds_hb(w, n, i + m, i) && ds_unbroken(w, i, i + m)) bits |= 1u << (m - 3);
    w.turn[i] = bits;
    w.state[i] = DS_NONE;
    int keys[DS_SLOTS], cnt = 0, bonds = 0;
    for (int s = 0; s < 2; ++s) bonds += w.acc[2 * (long)i + s] >= 0 && w.en[2 * (long)i + s] < DS_E_BOND;
    if (i >= 1 && i <= n - 2 && ds_unbroken(w, i - 1, i + 1)) {
      for (int c = 0; c < 8; ++c) {  // donor i or i + 1, slot 0 or 1, acceptor j or j - 1
        const int d = i + (c >> 2), s = (c >> 1) & 1;
        const int acc = w.acc[2 * (long)d + s];
        if (acc < 0 || !(w.en[2 * (long)d + s] < DS_E_BOND)) continue;
        const int j = acc + (c & 1);
        if (j < i + 3 || j > n - 2 || !ds_unbroken(w, j - 1, j + 1)) continue;
        const int type = ds_bridge_type(w, n, i, j);
        if (!type) continue;
        const int key = j * 4 + type;
        int at = 0;
        while (at < cnt && keys[at] < key) ++at;
        if (at < cnt && keys[at] == key) continue;
        if (cnt == DS_SLOTS) {  // (cannot happen: 2 donors x 2 slots x 2 acceptors)
          atomicOr(&status_sh, FDIPT_DSSP_BRIDGE_OVERFLOW);
          continue;
        }
        for (int t = cnt; t > at; --t) keys[t] = keys[t - 1];
        keys[at] = key;
        ++cnt;
      }
    }
    w.nbr[i] = cnt;
    for (int s = 0; s < cnt; ++s) w.bridge[(long)i * DS_SLOTS + s] = keys[s];
    if (bonds) atomicAdd(&count_sh[2], bonds);
    if (cnt) atomicAdd(&count_sh[3], cnt);
  }
  __syncthreads();

  // (4) ladders in order, the bulge pass
  if (tid == 0) {
    const long cap = (long)DS_SLOTS * N;
    long total = 0;
    bool full = false;
    for (int i = 1; i <= n - 2 && !full; ++i) {
      const int cnt = w.nbr[i];
      int mine[DS_SLOTS][5], m = 0;
      for (int s = 0; s < cnt; ++s) {
        const int key = w.bridge[(long)i * DS_SLOTS + s], j = key >> 2, type = key & 3, step = type == DS_PARALLEL ? 1 : -1;
        if (ds_is_bridge(w, n, i - 1, j - step, type)) continue;  // not the first bridge of its run
        int k = 0;
        while (ds_is_bridge(w, n, i + k + 1, j + step * (k + 1), type)) ++k;
        const int far = j + step * k;
        const int cand[5] = {type, i, i + k, j < far ? j : far, j < far ? far : j};
        int at = 0;
        while (at < m && ds_ladder_before(mine[at], cand)) ++at;
        for (int t = m; t > at; --t)
          for (int c = 0; c < 5; ++c) mine[t][c] = mine[t - 1][c];
        for (int c = 0; c < 5; ++c) mine[at][c] = cand[c];
        ++m;
      }
      if (total + m > cap) {
        full = true;
        break;
      }
      for (int t = 0; t < m; ++t)
        for (int c = 0; c < 5; ++c) w.lad[(total + t) * 5 + c] = mine[t][c];
      total += m;
    }
    if (full) status_sh |= FDIPT_DSSP_LADDER_OVERFLOW;
    long alive = total;
    for (long p = 0; p < total; ++p) {
      int* A = w.lad + p * 5;
      if (!A[0]) continue;
      for (long q = p + 1; q < total; ++q) {
        int* B = w.lad + q * 5;
        const int gap_i = B[1] - A[2];
        if (gap_i >= 6) break;
        if (!B[0] || B[0] != A[0] || gap_i <= 0) continue;
        const int g = A[0] == DS_PARALLEL ? B[3] - A[4] : A[3] - B[4];
        if (g <= 0 || !((g < 6 && gap_i < 3) || g < 3)) continue;
        const int i_lo = A[1] < B[1] ? A[1] : B[1], i_hi = A[2] > B[2] ? A[2] : B[2];
        const int j_lo = A[3] < B[3] ? A[3] : B[3], j_hi = A[4] > B[4] ? A[4] : B[4];
        if (!ds_unbroken(w, i_lo, i_hi) || !ds_unbroken(w, j_lo, j_hi)) continue;
        A[2] = B[2], A[3] = j_lo, A[4] = j_hi;
        B[0] = 0;
        --alive;
      }
    }
    listed_sh = (int)total;
    ladders_sh = (int)alive;
  }
  __syncthreads();

  // (5) classes: strand, alpha (overrides strand), 3-10, pi
  const int total = listed_sh;
  for (int p = tid; p < total; p += FD_THREADS) {
    const int* L = w.lad + (long)p * 5;
    if (!L[0]) continue;
    for (int k = L[1]; k <= L[2]; ++k) w.state[k] = DS_E;
    for (int k = L[3]; k <= L[4]; ++k) w.state[k] = DS_E;
  }
  __syncthreads();
  for (int i = tid + 1; i < n; i += FD_THREADS)
    if ((w.turn[i - 1] & 2) && (w.turn[i] & 2))
      for (int k = i; k < i + 4; ++k) w.state[k] = DS_ALPHA;  // (turn_4(i): i + 4 < n)
  __syncthreads();
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int m = pass ? 5 : 3, code = pass ? DS_PI : DS_310, bit = pass ? 4 : 1;
    for (int i = tid + 1; i < n; i += FD_THREADS) {
      if (!((w.turn[i - 1] & bit) && (w.turn[i] & bit))) continue;
      bool empty = true;  // (a row another thread turns into `code` meanwhile decides the same)
      for (int k = i; k < i + m; ++k) {
        const int s = w.state[k];
        empty = empty && (s == DS_NONE || s == code);
      }
      if (empty)
        for (int k = i; k < i + m; ++k) w.state[k] = code;
    }
    __syncthreads();
  }

  // (6) the outputs at the original rows, counts, fractions
  for (int r = tid; r < N; r += FD_THREADS) {
    a.ss[row0 + r] = FDIPT_DSSP_ABSENT;
    a.acceptor[(row0 + r) * 2] = a.acceptor[(row0 + r) * 2 + 1] = -1;
    a.acceptor_energy[(row0 + r) * 2] = a.acceptor_energy[(row0 + r) * 2 + 1] = 0.0;
  }
  __syncthreads();
  int helix = 0, strand = 0;
  for (int k = tid; k < n; k += FD_THREADS) {
    const int s = w.state[k], cls = s == DS_E ? FDIPT_DSSP_STRAND : s >= DS_ALPHA ? FDIPT_DSSP_HELIX : FDIPT_DSSP_COIL;
    const long r = row0 + w.map[k];
    helix += cls == FDIPT_DSSP_HELIX;
    strand += cls == FDIPT_DSSP_STRAND;
    a.ss[r] = (unsigned char)cls;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const int acc = w.acc[2 * (long)k + s2];
      a.acceptor[r * 2 + s2] = acc >= 0 ? w.map[acc] : -1;
      a.acceptor_energy[r * 2 + s2] = w.en[2 * (long)k + s2];
    }
  }
  if (helix) atomicAdd(&count_sh[0], helix);
  if (strand) atomicAdd(&count_sh[1], strand);
  __syncthreads();
  if (tid == 0) {
    const int h = count_sh[0], e = count_sh[1], status = status_sh;
    const double rows = status ? 0.0 : (double)n, bad = status ? 0.0 : 1.0;  // (0 / 0 = NaN: no row, or an overflow)
    a.helix_percent[b] = bad * h / rows;
    a.strand_percent[b] = bad * e / rows;
    a.coil_percent[b] = bad * (n - h - e) / rows;
    a.non_coil_percent[b] = bad * (h + e) / rows;
    a.n_rows[b] = n;
    a.n_hbonds[b] = count_sh[2];
    a.n_bridges[b] = count_sh[3];
    a.n_ladders[b] = ladders_sh;
    a.status[b] = status;
  }
}

extern "C" size_t fdipt_sample_dssp_workspace(int B, int N) {
  if (B < 1 || N < 1) return 0;
  return (size_t)B * ds_stride((size_t)N);
}

extern "C" int fdipt_sample_dssp(const FdiptDsspArgs* a, fdipt_stream_t stream) {
  if (!a || a->B < 1 || a->N < 1 || (a->atoms != 37 && a->atoms != 5)) return FDIPT_EINVAL;
  if (!a->prot || !a->res_mask || !a->chain_idx || !a->is_proline || !a->ss || !a->helix_percent || !a->strand_percent || !a->coil_percent ||
      !a->non_coil_percent || !a->n_rows || !a->n_hbonds || !a->n_bridges || !a->n_ladders || !a->acceptor || !a->acceptor_energy ||
      !a->status || !a->workspace)
    return FDIPT_EINVAL;
  if ((long)DS_SLOTS * a->N * 5 > 0x7fffffffL) return FDIPT_ESIZE;  // (the ladder list is addressed with ints times 5)
  if (a->workspace_bytes < fdipt_sample_dssp_workspace(a->B, a->N)) return FDIPT_ESIZE;
  hipLaunchKernelGGL(dssp_kernel, dim3((unsigned)a->B), dim3(FD_THREADS), 0, (hipStream_t)stream, *a);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
