// tmalign_body.hpp — the alignment search of one pair of CA traces by one block, shared by tmalign.hip (P listed pairs of two dense
// arrays) and structsearch.hip (queries against a packed, ragged structure set); DESIGN.md section 7.9 is the contract, section 7.15 the
// second user.  tma_pair<FULL, MASK_B>(...) is the former body of tm_align_kernel: compaction, Sec, I1, the three iterated initial
// alignments, the d8 filter and the final searches per length.  It is parametrised by how the second trace is loaded (MASK_B: rows
// chosen by a mask with an atom stride, else every row of a packed CA array) and by which outputs are written (FULL: all of
// FdiptTmAlignArgs; else tm_a, tm_b, n_aligned, rmsd and status), and it asks `early(n1, n2)` for status bits to leave with once both
// row counts are known (the length bound of the structure search).  The layout is sized by the launch's (Na, Nb); the traces hold
// A.rows <= Na and B.rows <= Nb rows.  INITS5 (a third switch, false in every instantiation of the default mode, which it leaves
// unchanged) adds the two fragment starts of section 7.9's addendum behind I1 - I3: I4, the best of a grid of local superpositions
// (candidates one after another on the whole block: one thread's tma_superpose of the fragment, tma_dp, tma_gather, one thread's
// tma_fast), and I5, I1's thread-per-offset walk over the shorter of the two traces' longest unbroken runs; init_tm and init_dp then
// hold five entries per pair and the layout one more map.  An including unit turns contraction off and includes common.hpp, horn.hpp
// and tmsearch.hpp first.
#pragma once

#define TMA_MAX_ROWS FDIPT_TMA_MAX_ROWS
#define TMA_C2_LIMIT 1e6  // Angstrom^2: the widening of Fast's cut ends here
#define TMA_DP_ITERATIONS 30
#define TMA_SEC_C 0
#define TMA_SEC_T 1
#define TMA_SEC_H 2
#define TMA_SEC_E 3
#define TMA_FRAG_C0 4.25    // Angstrom: the first cut of Frag
#define TMA_FRAG_GROWTH 1.1
#define TMA_FRAG_ROUNDS 64

__host__ __device__ inline int tma_dir_stride(int Nb) { return ((Nb + 15) / 16) | 1; }  // words per row, odd: rows spread over the banks

struct TmaLayout {
  size_t x, y, pairs, val, slots, shared, map, rows, bytes, total;
  int K;
};
// doubles first, then the region the directions and the search's masks share, then shorts, then bytes
// (`five`: the layout of INITS5, one more map of Nb shorts for I4's best candidate)
__host__ __device__ inline TmaLayout tma_layout(int Na, int Nb, bool five = false) {
  TmaLayout l;
  l.K = Na < Nb ? Na : Nb;
  size_t o = 0;
  l.x = o, o += (size_t)3 * Na * 8;
  l.y = o, o += (size_t)3 * Nb * 8;
  l.pairs = o, o += (size_t)6 * l.K * 8;
  l.val = o, o += (size_t)2 * (Na + 1) * 8;
  l.slots = o, o += (size_t)3 * sizeof(TmTransform) + 8;
  const size_t dirs = (size_t)Na * tma_dir_stride(Nb) * 4, search = tm_search_lds_bytes(l.K);
  l.shared = o, o += ((dirs > search ? dirs : search) + 7) / 8 * 8;
  l.map = o, o += (size_t)(five ? 3 : 2) * Nb * 2;
  l.rows = o, o += (size_t)(Na + Nb) * 2;
  l.bytes = o, o += (size_t)2 * (Na + 1) + Na + Nb;
  l.total = (o + 7) / 8 * 8;
  return l;
}

struct TmaTrace { const double *x, *y, *z; };

// positions of the set flags of one chunk of FD_THREADS items in ascending order, behind `base` (two barriers)
__device__ __forceinline__ int tma_positions(bool f, int base, int* cnt_sh, int& total) {
  const int lane = threadIdx.x & (FD_WAVE - 1), wave = threadIdx.x / FD_WAVE;
  const unsigned long long bal = __ballot(f);
  if (lane == 0) cnt_sh[wave] = __popcll(bal);
  __syncthreads();
  int off = base, tot = 0;
#pragma unroll
  for (int v = 0; v < FD_THREADS / FD_WAVE; ++v) {
    if (v < wave) off += cnt_sh[v];
    tot += cnt_sh[v];
  }
  __syncthreads();
  total = tot;
  return off + __popcll(bal & ((1ull << lane) - 1ull));
}

// superpose the pairs (a[j + koff], b[j]), j0 <= j < j1, that lie within c2 under Tp (all of them without `select`)
__device__ __forceinline__ void tma_superpose(const TmaTrace& a, const TmaTrace& b, int koff, int j0, int j1, bool select, const TmTransform& Tp, double c2,
                                              TmTransform& T) {
  double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, m = 0.0;
  for (int j = j0; j < j1; ++j) {
    const int i = j + koff;
    if (!select || tm_dist2(Tp, a.x[i], a.y[i], a.z[i], b.x[j], b.y[j], b.z[j]) <= c2) {
      c[0] += a.x[i]; c[1] += a.y[i]; c[2] += a.z[i];
      c[3] += b.x[j]; c[4] += b.y[j]; c[5] += b.z[j];
      m += 1.0;
    }
  }
  const double inv_m = m > 0.0 ? 1.0 / m : 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) c[k] *= inv_m;
  double H[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int j = j0; j < j1; ++j) {
    const int i = j + koff;
    if (!select || tm_dist2(Tp, a.x[i], a.y[i], a.z[i], b.x[j], b.y[j], b.z[j]) <= c2) {
      const double ax = a.x[i] - c[0], ay = a.y[i] - c[1], az = a.z[i] - c[2], bx = b.x[j] - c[3], by = b.y[j] - c[4], bz = b.z[j] - c[5];
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

// Fast of the pairs (a[j + koff], b[j]), j0 <= j < j1: the largest of up to three scores and the transform of the first that reached it
__device__ __forceinline__ double tma_fast(const TmaTrace& a, const TmaTrace& b, int koff, int j0, int j1, double d0sq, double ds, TmTransform& Tb) {
  const int k = j1 - j0;
  double best = -1.0, c2 = 0.0;
  TmTransform T, Tp;
#pragma unroll
  for (int q = 0; q < 9; ++q) Tp.R[q] = Tb.R[q] = 0.0;
  Tp.t[0] = Tp.t[1] = Tp.t[2] = Tb.t[0] = Tb.t[1] = Tb.t[2] = 0.0;
  for (int pass = 0; pass < 3; ++pass) {
    tma_superpose(a, b, koff, j0, j1, pass > 0, Tp, c2, T);
    double next = pass == 0 ? ds * ds : ds * ds + 1.0, score = 0.0;
    int inside = 0;
    for (int j = j0; j < j1; ++j) {
      const int i = j + koff;
      const double d2 = tm_dist2(T, a.x[i], a.y[i], a.z[i], b.x[j], b.y[j], b.z[j]);
      score += d0sq / (d0sq + d2);
      inside += d2 <= next;
    }
    if (pass == 0 || score > best) best = score, Tb = T;
    if (pass == 2) break;
    if (inside < 3 && k > 3) {  // the cut grows in steps of 0.5 until the third smallest distance is inside; then count again
      double m1 = 1.0 / 0.0, m2 = m1, m3 = m1;
      for (int j = j0; j < j1; ++j) {
        const int i = j + koff;
        const double d2 = tm_dist2(T, a.x[i], a.y[i], a.z[i], b.x[j], b.y[j], b.z[j]);
        if (d2 < m1) m3 = m2, m2 = m1, m1 = d2;
        else if (d2 < m2) m3 = m2, m2 = d2;
        else if (d2 < m3) m3 = d2;
      }
      // next + 0.5 n for the smallest n >= 1 with m3 inside, n at most the first at which the cut reaches the limit: n from one
      // division, corrected by one step either way for its rounding
      double n = fmax(ceil((m3 - next) * 2.0), 1.0);
      if (n > 1.0 && m3 <= next + 0.5 * (n - 1.0)) n -= 1.0;
      if (!(m3 <= next + 0.5 * n)) n += 1.0;
      const double most = ceil((TMA_C2_LIMIT - next) * 2.0);
      next += 0.5 * (n <= most ? n : most);
      inside = 0;
      for (int j = j0; j < j1; ++j) {
        const int i = j + koff;
        inside += tm_dist2(T, a.x[i], a.y[i], a.z[i], b.x[j], b.y[j], b.z[j]) <= next;
      }
    }
    if (inside == k) break;
    Tp = T, c2 = next;
  }
  return best;
}

__device__ __forceinline__ int tma_sec_of(const TmaTrace& t, int i, int n) {
  if (i < 2 || i > n - 3) return TMA_SEC_C;
  auto d2 = [&](int p, int q) {
    const double dx = t.x[p] - t.x[q], dy = t.y[p] - t.y[q], dz = t.z[p] - t.z[q];
    return dx * dx + dy * dy + dz * dz;
  };
  const double v[6] = {d2(i - 2, i), d2(i - 2, i + 1), d2(i - 2, i + 2), d2(i - 1, i + 1), d2(i - 1, i + 2), d2(i, i + 2)};
  const double hc[6] = {5.45, 5.18, 6.37, 5.45, 5.18, 5.45}, ec[6] = {6.1, 10.4, 13.0, 6.1, 10.4, 6.1};
  bool h = true, e = true;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    h = h && (hc[k] - 2.1) * (hc[k] - 2.1) < v[k] && v[k] < (hc[k] + 2.1) * (hc[k] + 2.1);
    e = e && (ec[k] - 1.42) * (ec[k] - 1.42) < v[k] && v[k] < (ec[k] + 1.42) * (ec[k] + 1.42);
  }
  return h ? TMA_SEC_H : e ? TMA_SEC_E : v[2] < 64.0 ? TMA_SEC_T : TMA_SEC_C;
}

// I4's step between fragment starts on a trace of n rows
__device__ __forceinline__ int tma_jump(int n) {
  const int j = n > 250 ? 45 : n > 200 ? 35 : n > 150 ? 25 : 15;
  return j < n / 3 ? j : n / 3;
}

// Frag by one thread: out[0], out[1] = the first row and the rows of the longest run of the trace whose successive squared distances lie
// strictly below c^2, the first among equals; c grows by one multiplication per round until the run has min(4, n / 3) rows, and after
// TMA_FRAG_ROUNDS rounds the run is the whole trace
__device__ __forceinline__ void tma_frag(const TmaTrace& t, int n, int* out) {
  const int need = n / 3 < 4 ? n / 3 : 4;
  double c = TMA_FRAG_C0;
  int start = 0, rows = n;
  for (int round = 0; round < TMA_FRAG_ROUNDS; ++round) {
    int best_s = 0, best_r = 1, s0 = 0;
    for (int i = 1; i < n; ++i) {
      const double dx = t.x[i] - t.x[i - 1], dy = t.y[i] - t.y[i - 1], dz = t.z[i] - t.z[i - 1];
      if (!(dx * dx + dy * dy + dz * dz < c * c)) s0 = i;
      if (i - s0 + 1 > best_r) best_s = s0, best_r = i - s0 + 1;
    }
    if (best_r >= need) {
      start = best_s, rows = best_r;
      break;
    }
    c = c * TMA_FRAG_GROWTH;
  }
  out[0] = start, out[1] = rows;
}

struct TmaShared {
  TmaTrace X, Y, PA, PB;           // the traces and the gathered pairs
  double* val;                     // [2][Na + 1]
  unsigned char* pth;              // [2][Na + 1]
  unsigned* dirs;                  // [n1][stride], shared with the search's masks
  short* map;                      // [Nb]: the compacted row of x per compacted row of y, or -1
  const unsigned char *sec_a, *sec_b;
  int n1, n2, stride, vstride;
};

// one cell of the programme: row i (1-based) of thread-owned state at column j = d - i
struct TmaRow {
  double tx, ty, tz, left, diag;
  unsigned word;
  int sec;
  bool left_on;
};

// DP(score, g) by the whole block; score(i, j) = (dsq > 0 ? dsq / (dsq + |T x_i - y_j|^2) : 0) + (Sec equal ? bonus : 0).  Leaves the
// map in sh.map and returns the number of aligned pairs.
__device__ __forceinline__ int tma_dp(const TmaShared& sh, const TmTransform* Tsh, double dsq, double bonus, double g, int* count_sh) {
  const int tid = threadIdx.x, n1 = sh.n1, n2 = sh.n2;
  TmaRow row[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int i = tid + 1 + r * FD_THREADS;
    row[r].tx = row[r].ty = row[r].tz = 0.0;
    row[r].left = row[r].diag = 0.0, row[r].word = 0, row[r].left_on = false, row[r].sec = 0;
    if (i <= n1) {
      row[r].sec = sh.sec_a[i - 1];
      if (dsq > 0.0) {
        const double x = sh.X.x[i - 1], y = sh.X.y[i - 1], z = sh.X.z[i - 1];
        row[r].tx = Tsh->R[0] * x + Tsh->R[1] * y + Tsh->R[2] * z + Tsh->t[0];
        row[r].ty = Tsh->R[3] * x + Tsh->R[4] * y + Tsh->R[5] * z + Tsh->t[1];
        row[r].tz = Tsh->R[6] * x + Tsh->R[7] * y + Tsh->R[8] * z + Tsh->t[2];
      }
    }
  }
  if (tid == 0) sh.val[0] = sh.val[sh.vstride] = 0.0, sh.pth[0] = sh.pth[sh.vstride] = 0;  // row 0 of both buffers
  for (int j = tid; j < n2; j += FD_THREADS) sh.map[j] = -1;
  __syncthreads();
  for (int d = 2; d <= n1 + n2; ++d) {
    const double* vin = sh.val + ((d - 1) & 1) * sh.vstride;
    const unsigned char* pin = sh.pth + ((d - 1) & 1) * sh.vstride;
    double* vout = sh.val + (d & 1) * sh.vstride;
    unsigned char* pout = sh.pth + (d & 1) * sh.vstride;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int i = tid + 1 + r * FD_THREADS, j = d - i;
      if (i <= n1 && j >= 1 && j <= n2) {
        const double up = vin[i - 1];
        const bool up_on = pin[i - 1] != 0;
        double s = 0.0;
        if (dsq > 0.0) {
          const double dx = row[r].tx - sh.Y.x[j - 1], dy = row[r].ty - sh.Y.y[j - 1], dz = row[r].tz - sh.Y.z[j - 1];
          s = dsq / (dsq + (dx * dx + dy * dy + dz * dz));
        }
        s += row[r].sec == sh.sec_b[j - 1] ? bonus : 0.0;
        const double dg = row[r].diag + s, h = up + (up_on ? g : 0.0), v = row[r].left + (row[r].left_on ? g : 0.0);
        const bool on = dg >= h && dg >= v;
        const double value = on ? dg : (v >= h ? v : h);
        row[r].word |= (on ? 0u : (v >= h ? 1u : 2u)) << (2 * ((j - 1) & 15));
        if (((j - 1) & 15) == 15 || j == n2) sh.dirs[(i - 1) * sh.stride + ((j - 1) >> 4)] = row[r].word, row[r].word = 0;
        row[r].diag = up, row[r].left = value, row[r].left_on = on;
        vout[i] = value, pout[i] = on;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {  // the traceback
    int i = n1, j = n2, count = 0;
    while (i > 0 && j > 0) {
      const unsigned code = (sh.dirs[(i - 1) * sh.stride + ((j - 1) >> 4)] >> (2 * ((j - 1) & 15))) & 3u;
      if (code == 0) sh.map[j - 1] = (short)(i - 1), --i, --j, ++count;
      else if (code == 1) --j;
      else --i;
    }
    *count_sh = count;
  }
  __syncthreads();
  return *count_sh;
}

// the pairs of `map` (those within d8sq under *Tsh where `filter`, the others are dropped from the map) into PA / PB; returns their number
__device__ __forceinline__ int tma_gather(const TmaShared& sh, short* map, bool filter, const TmTransform* Tsh, double d8sq, int* cnt_sh) {
  int k = 0;
  double* ax = (double*)sh.PA.x; double* ay = (double*)sh.PA.y; double* az = (double*)sh.PA.z;
  double* bx = (double*)sh.PB.x; double* by = (double*)sh.PB.y; double* bz = (double*)sh.PB.z;
  for (int j0 = 0; j0 < sh.n2; j0 += FD_THREADS) {
    const int j = j0 + threadIdx.x;
    int i = j < sh.n2 ? map[j] : -1;
    if (filter && i >= 0) {
      TmTransform T = *Tsh;
      if (tm_dist2(T, sh.X.x[i], sh.X.y[i], sh.X.z[i], sh.Y.x[j], sh.Y.y[j], sh.Y.z[j]) > d8sq) map[j] = -1, i = -1;
    }
    int total;
    const int pos = tma_positions(i >= 0, k, cnt_sh, total);
    if (i >= 0) {  // (pos < K: the map is monotone, at most min(n1, n2) pairs)
      ax[pos] = sh.X.x[i], ay[pos] = sh.X.y[i], az[pos] = sh.X.z[i];
      bx[pos] = sh.Y.x[j], by[pos] = sh.Y.y[j], bz[pos] = sh.Y.z[j];
    }
    k += total;
  }
  __syncthreads();
  return k;
}

struct TmaSource {
  const float* ca;    // the CA atom of row 0
  const float* mask;  // [rows] or nullptr (MASK_B false: every row is set)
  long stride;        // floats between the CA atoms of two rows
  int rows;
};

// where a pair's outputs go: element p of each array (the arrays FULL does not need may be nullptr)
struct TmaOut {
  double *tm, *tm_a, *tm_b, *rotation, *translation, *rmsd, *d0_a, *d0_b, *init_tm;
  int *alignment, *n_aligned, *init_dp, *best_init, *status;
  long align_stride;  // ints per pair of `alignment`
};

struct TmaNoEarly {
  __device__ __forceinline__ int operator()(int, int) const { return 0; }
};

// Prepares the outputs of pair p as the search's first lines do (FULL only): what a block that returns before tma_pair leaves behind.
template <bool FULL, bool INITS5 = false>
__device__ __forceinline__ void tma_clear(const TmaOut& o, long p, int Nb_rows) {
  constexpr int NI = INITS5 ? 5 : 3;
  if constexpr (FULL) {
    for (int j = threadIdx.x; j < Nb_rows; j += FD_THREADS) o.alignment[p * o.align_stride + j] = -1;
    if (threadIdx.x < NI) o.init_tm[p * NI + threadIdx.x] = -1.0, o.init_dp[p * NI + threadIdx.x] = 0;
  }
}

// what a pair that is not searched, or not to the end, leaves behind
template <bool FULL>
__device__ __forceinline__ void tma_leave(const TmaOut& o, long p, int status, int n_aligned, double d0a, double d0b, int best_init) {
  if (threadIdx.x == 0) {
    const double nan = __builtin_nan("");
    if constexpr (FULL) {
      o.tm[p] = o.tm_a[p] = o.tm_b[p] = o.rmsd[p] = nan, o.n_aligned[p] = n_aligned, o.d0_a[p] = d0a, o.d0_b[p] = d0b;
      o.best_init[p] = best_init, o.status[p] = status;
      for (int k = 0; k < 9; ++k) o.rotation[p * 9 + k] = (k % 4 == 0) ? 1.0 : 0.0;
      for (int k = 0; k < 3; ++k) o.translation[p * 3 + k] = 0.0;
    } else {
      o.tm_a[p] = o.tm_b[p] = o.rmsd[p] = nan, o.n_aligned[p] = n_aligned, o.status[p] = status;
    }
  }
}

// The search of one pair by the whole block.  `tma_sh`: tma_layout(Na, Nb, INITS5).total bytes of LDS, 8-byte aligned; cnt_sh:
// FD_THREADS / FD_WAVE ints; next_sh, passes_sh, count_sh: one int each.  The caller has run tma_clear<FULL, INITS5>.
template <bool FULL, bool MASK_B, bool INITS5, class Early>
__device__ __forceinline__ void tma_pair(const TmaSource& A, const TmaSource& B, int Na, int Nb, const TmaOut& o, long p, double* tma_sh, int* cnt_sh,
                                         int* next_sh, int* passes_sh, int* count_sh, Early early) {
  const int tid = threadIdx.x;
  constexpr int NI = INITS5 ? 5 : 3;
  const TmaLayout lay = tma_layout(Na, Nb, INITS5);
  char* base = (char*)tma_sh;
  double *xx = (double*)(base + lay.x), *yy = (double*)(base + lay.y), *pp = (double*)(base + lay.pairs);
  TmTransform* slots = (TmTransform*)(base + lay.slots);  // 0: the running transform, 1: the best alignment's, 2: T0 of I3
  double* s_sh = (double*)(slots + 3);                     // the running search's score
  unsigned* shared = (unsigned*)(base + lay.shared);
  short *map = (short*)(base + lay.map), *best_map = map + Nb;
  short *rows_a = (short*)(base + lay.rows), *rows_b = rows_a + Na;
  unsigned char* pth = (unsigned char*)(base + lay.bytes);
  unsigned char *sec_a = pth + 2 * (Na + 1), *sec_b = sec_a + Na;

  // ---- the two traces, compacted separately
  int n1 = 0, n2 = 0;
  bool finite = true;
  for (int n0 = 0; n0 < A.rows; n0 += FD_THREADS) {
    const int i = n0 + tid;
    const bool f = i < A.rows && A.mask[i] != 0.f;
    int total;
    const int pos = tma_positions(f, n1, cnt_sh, total);
    if (f) {  // (pos < Na: at most one position per row)
      const float* u = A.ca + (long)i * A.stride;
      xx[pos] = (double)u[0], xx[Na + pos] = (double)u[1], xx[2 * Na + pos] = (double)u[2], rows_a[pos] = (short)i;
      finite = finite && isfinite(u[0]) && isfinite(u[1]) && isfinite(u[2]);
    }
    n1 += total;
  }
  if constexpr (MASK_B) {
    for (int n0 = 0; n0 < B.rows; n0 += FD_THREADS) {
      const int i = n0 + tid;
      const bool f = i < B.rows && B.mask[i] != 0.f;
      int total;
      const int pos = tma_positions(f, n2, cnt_sh, total);
      if (f) {
        const float* u = B.ca + (long)i * B.stride;
        yy[pos] = (double)u[0], yy[Nb + pos] = (double)u[1], yy[2 * Nb + pos] = (double)u[2], rows_b[pos] = (short)i;
        finite = finite && isfinite(u[0]) && isfinite(u[1]) && isfinite(u[2]);
      }
      n2 += total;
    }
  } else {  // every row is set: row i is compacted row i
    for (int i = tid; i < B.rows; i += FD_THREADS) {
      const float* u = B.ca + (long)i * B.stride;
      yy[i] = (double)u[0], yy[Nb + i] = (double)u[1], yy[2 * Nb + i] = (double)u[2], rows_b[i] = (short)i;
      finite = finite && isfinite(u[0]) && isfinite(u[1]) && isfinite(u[2]);
    }
    n2 = B.rows;
  }
  const double d0a = n1 > 21 ? 1.24 * cbrt((double)(n1 - 15)) - 1.8 : 0.5, d0b = n2 > 21 ? 1.24 * cbrt((double)(n2 - 15)) - 1.8 : 0.5;
  if (n1 < 5 || n2 < 5) {
    tma_leave<FULL>(o, p, FDIPT_TMA_TOO_SHORT, 0, d0a, d0b, -1);
    return;
  }
  if (const int bits = early(n1, n2)) {  // (uniform over the block: a function of n1, n2 and values no launch mate writes)
    tma_leave<FULL>(o, p, bits, 0, d0a, d0b, -1);
    return;
  }
  if (!__syncthreads_and(finite)) {  // (also the barrier behind the compaction)
    tma_leave<FULL>(o, p, FDIPT_TMA_NOT_FINITE, 0, d0a, d0b, -1);
    return;
  }
  TmaShared sh;
  sh.X = TmaTrace{xx, xx + Na, xx + 2 * Na}, sh.Y = TmaTrace{yy, yy + Nb, yy + 2 * Nb};
  sh.PA = TmaTrace{pp, pp + lay.K, pp + 2 * lay.K}, sh.PB = TmaTrace{pp + 3 * lay.K, pp + 4 * lay.K, pp + 5 * lay.K};
  sh.val = (double*)(base + lay.val), sh.pth = pth, sh.dirs = shared, sh.map = map, sh.sec_a = sec_a, sh.sec_b = sec_b;
  sh.n1 = n1, sh.n2 = n2, sh.stride = tma_dir_stride(Nb), sh.vstride = Na + 1;
  const int Ls = n1 < n2 ? n1 : n2, W = (lay.K + 31) / 32;
  const double d0s = (Ls <= 19 ? 0.168 : 1.24 * cbrt((double)(Ls - 15)) - 1.8) + 0.8, ds = fmin(fmax(d0s, 4.5), 8.0);
  const double d8 = 1.5 * pow((double)Ls, 0.3) + 3.5, d0ssq = d0s * d0s, d8sq = d8 * d8;

  // ---- Sec
  for (int i = tid; i < n1; i += FD_THREADS) sec_a[i] = (unsigned char)tma_sec_of(sh.X, i, n1);
  for (int j = tid; j < n2; j += FD_THREADS) sec_b[j] = (unsigned char)tma_sec_of(sh.Y, j, n2);

  // ---- I1: the best offset of the gapless threading by Fast, the lowest offset among equals; its transform into slot 2
  const int m = Ls / 2 > 5 ? Ls / 2 : 5, k_lo = -(n2 - m), n_off = n1 - m - k_lo + 1;
  double f1 = -1.0;
  int k1 = 0;
  {
    double mine = -1.0;
    int mine_k = 0x7fffffff;
    TmTransform Tmine, T;
#pragma unroll
    for (int q = 0; q < 9; ++q) Tmine.R[q] = 0.0;
    Tmine.t[0] = Tmine.t[1] = Tmine.t[2] = 0.0;
    for (int oo = tid; oo < n_off; oo += FD_THREADS) {
      const int k = k_lo + oo, j0 = k < 0 ? -k : 0, j1 = n1 - k < n2 ? n1 - k : n2;
      const double f = tma_fast(sh.X, sh.Y, k, j0, j1, d0ssq, ds, T);
      if (f > mine) mine = f, mine_k = k, Tmine = T;
    }
    double* red_s = (double*)shared;
    int* red_k = (int*)(red_s + FD_THREADS);
    red_s[tid] = mine, red_k[tid] = mine_k;
    __syncthreads();
    int owner = 0;
    for (int t = 1; t < FD_THREADS; ++t)
      if (red_s[t] > red_s[owner] || (red_s[t] == red_s[owner] && red_k[t] < red_k[owner])) owner = t;
    f1 = red_s[owner], k1 = red_k[owner];
    if (tid == owner) slots[2] = Tmine;
    __syncthreads();
  }

  double best_tm = -1.0;
  int best_init = -1;
  for (int which = 0; which < NI; ++which) {
    // ---- the initial alignment into the map
    int k;
    if (which == 0) {
      for (int j = tid; j < n2; j += FD_THREADS) map[j] = (short)(j + k1 >= 0 && j + k1 < n1 ? j + k1 : -1);
      __syncthreads();
    } else if (which == 1) {
      tma_dp(sh, slots, 0.0, 1.0, -1.0, count_sh);
    } else if (!INITS5 || which == 2) {
      const double d01 = d0s + 1.5;
      tma_dp(sh, slots + 2, d01 * d01, 0.5, -1.0, count_sh);
    }
    if constexpr (INITS5) {
      if (which == 3) {
        // ---- I4: the candidates (length, i, j) one after another; slot 0 holds the fragment's transform, best_map + Nb the best map
        short* map4 = best_map + Nb;
        const double d01 = d0s + 1.5;
        const int ja = tma_jump(n1), jb = tma_jump(n2);
        double best_f = -1.0;
        bool have = false;
        for (int pass = 0; pass < 2; ++pass) {
          const int l = pass == 0 ? (Ls / 3 < 20 ? Ls / 3 : 20) : (Ls / 2 < 100 ? Ls / 2 : 100);
          if (l < 3) continue;
          for (int i = 0; i + l <= n1; i += ja)
            for (int j = 0; j + l <= n2; j += jb) {
              if (tid == 0) {
                TmTransform T;
                tma_superpose(sh.X, sh.Y, i - j, j, j + l, false, slots[1], 0.0, T);
                slots[0] = T;
              }
              __syncthreads();
              int kc = tma_dp(sh, slots, d01 * d01, 0.0, 0.0, count_sh);
              if (kc < 3) continue;
              kc = tma_gather(sh, map, false, slots, 0.0, cnt_sh);
              if (tid == 0) {
                TmTransform T;
                *s_sh = tma_fast(sh.PA, sh.PB, 0, 0, kc, d0ssq, ds, T);
              }
              __syncthreads();
              const double f = *s_sh;
              if (!have || f > best_f) {  // the first in candidate order among equals
                have = true, best_f = f;
                for (int r = tid; r < n2; r += FD_THREADS) map4[r] = map[r];
              }
              __syncthreads();  // (the score is read; the next candidate writes it and the map)
            }
        }
        if (!have) continue;
        for (int r = tid; r < n2; r += FD_THREADS) map[r] = map4[r];
        __syncthreads();
      } else if (which == 4) {
        // ---- I5: Frag of both traces by one thread each, then I1's walk over the donor's fragment
        int* frag_sh = (int*)shared;
        if (tid == 0) tma_frag(sh.X, n1, frag_sh);
        if (tid == FD_WAVE) tma_frag(sh.Y, n2, frag_sh + 2);
        __syncthreads();
        const int sx = frag_sh[0], Lx = frag_sh[1], sy = frag_sh[2], Ly = frag_sh[3];
        __syncthreads();  // (the reduction's arrays lie there)
        const bool from_x = Lx < Ly || (Lx == Ly && n1 <= n2);
        const int L = Lx < Ly ? Lx : Ly, other = from_x ? n2 : n1;
        int r0 = from_x ? sx : sy, r1 = r0 + L;  // the fragment: rows r0 .. r1 - 1 of the donor
        if (L == Ls) r1 = r0 + (89 * Ls) / 100 + 1, r0 += Ls / 10;
        const int fifths = (2 * (L < other ? L : other)) / 5, mn = fifths > 3 ? fifths : 3;
        const int xa = from_x ? r0 : 0, xb = from_x ? r1 : n1, ya = from_x ? 0 : r0, yb = from_x ? n2 : r1;
        const int k5_lo = xa - yb + 1, n5_off = xb - ya - k5_lo;  // every offset with a pair
        double mine = -1.0;
        int mine_k = 0x7fffffff;
        TmTransform T;
        for (int oo = tid; oo < n5_off; oo += FD_THREADS) {
          const int kk = k5_lo + oo, j0 = ya > xa - kk ? ya : xa - kk, j1 = yb < xb - kk ? yb : xb - kk;
          if (j1 - j0 < mn) continue;
          const double f = tma_fast(sh.X, sh.Y, kk, j0, j1, d0ssq, ds, T);
          if (f > mine) mine = f, mine_k = kk;
        }
        double* red_s = (double*)shared;
        int* red_k = (int*)(red_s + FD_THREADS);
        red_s[tid] = mine, red_k[tid] = mine_k;
        __syncthreads();
        int owner = 0;
        for (int t = 1; t < FD_THREADS; ++t)
          if (red_s[t] > red_s[owner] || (red_s[t] == red_s[owner] && red_k[t] < red_k[owner])) owner = t;
        const double f5 = red_s[owner];
        const int k5 = red_k[owner];
        __syncthreads();
        if (!(f5 >= 0.0)) continue;  // no offset qualifies
        const int j0 = ya > xa - k5 ? ya : xa - k5, j1 = yb < xb - k5 ? yb : xb - k5;
        for (int j = tid; j < n2; j += FD_THREADS) map[j] = (short)(j >= j0 && j < j1 ? j + k5 : -1);
        __syncthreads();
      }
    }
    k = tma_gather(sh, map, false, slots, 0.0, cnt_sh);
    if (which == 1 && k >= 3) {  // F2 and T2 by one thread; T0 = T2 where F2 leads
      if (tid == 0) {
        TmTransform T2;
        if (!(f1 >= tma_fast(sh.PA, sh.PB, 0, 0, k, d0ssq, ds, T2))) slots[2] = T2;
      }
      __syncthreads();
    }
    if (k < 3) continue;
    // ---- the iteration
    int dps = 0;
    double old = 0.0;
    for (int round = -1; round < 2 * TMA_DP_ITERATIONS; ++round) {  // -1: the initial alignment itself
      const int it = round < 0 ? 0 : round % TMA_DP_ITERATIONS;
      if (round >= 0) {
        k = tma_dp(sh, slots, d0ssq, 0.0, round < TMA_DP_ITERATIONS ? -0.6 : 0.0, count_sh);
        ++dps;
        if (k >= 3) k = tma_gather(sh, map, false, slots, 0.0, cnt_sh);
      }
      bool leave_loop = k < 3;
      if (!leave_loop) {
        double s;
        int seed;
        TmTransform T;
        if (tm_search(sh.PA.x, sh.PA.y, sh.PA.z, sh.PB.x, sh.PB.y, sh.PB.z, k, d0ssq, ds, 40, d8sq, shared, W, next_sh, passes_sh, s, seed, T))
          slots[0] = T, *s_sh = s;
        __syncthreads();
        const double tm = *s_sh / (double)Ls;
        if constexpr (FULL)
          if (round < 0 && tid == 0) o.init_tm[p * NI + which] = tm;
        if (tm > best_tm) {
          best_tm = tm, best_init = which;
          for (int j = tid; j < n2; j += FD_THREADS) best_map[j] = map[j];
          if (tid == 0) slots[1] = slots[0];
        }
        if (round >= 0) {
          leave_loop = it > 0 && fabs(old - tm) < 1e-6;
          old = tm;
        }
        __syncthreads();
      }
      if (leave_loop) {  // the gap value's loop ends; the next one starts (or the iteration is over)
        if (round < 0 || round >= TMA_DP_ITERATIONS) break;
        round = TMA_DP_ITERATIONS - 1;
      }
    }
    if constexpr (FULL)
      if (tid == 0) o.init_dp[p * NI + which] = dps;
  }

  // ---- final: drop the pairs beyond d8, score per normalisation length
  const int k = tma_gather(sh, best_map, true, slots + 1, d8sq, cnt_sh);
  if constexpr (FULL)
    for (int j = tid; j < n2; j += FD_THREADS) o.alignment[p * o.align_stride + rows_b[j]] = best_map[j] >= 0 ? (int)rows_a[best_map[j]] : -1;
  if (k < 3) {
    tma_leave<FULL>(o, p, FDIPT_TMA_NO_ALIGNMENT, k, d0a, d0b, best_init);
    return;
  }
  double s;
  int seed;
  TmTransform T;
  if (tm_search(sh.PA.x, sh.PA.y, sh.PA.z, sh.PB.x, sh.PB.y, sh.PB.z, k, d0b * d0b, fmin(fmax(d0b, 4.5), 8.0), 1, 0.0, shared, W, next_sh, passes_sh, s, seed,
                T)) {
    double sum = 0.0;
    for (int i = 0; i < k; ++i) sum += tm_dist2(T, sh.PA.x[i], sh.PA.y[i], sh.PA.z[i], sh.PB.x[i], sh.PB.y[i], sh.PB.z[i]);
    o.tm_b[p] = s / (double)n2, o.rmsd[p] = sqrt(sum / (double)k), o.n_aligned[p] = k, o.status[p] = 0;
    if (n1 == n2) o.tm_a[p] = s / (double)n1;
    if constexpr (FULL) {
      o.tm[p] = s / (double)n2, o.d0_a[p] = d0a, o.d0_b[p] = d0b, o.best_init[p] = best_init;
#pragma unroll
      for (int q = 0; q < 9; ++q) fd_st(o.rotation + p * 9 + q, T.R[q]);
#pragma unroll
      for (int q = 0; q < 3; ++q) fd_st(o.translation + p * 3 + q, T.t[q]);
    }
  }
  if (n1 != n2) {
    __syncthreads();  // (the first search's reduction is read; the second one writes the masks)
    if (tm_search(sh.PA.x, sh.PA.y, sh.PA.z, sh.PB.x, sh.PB.y, sh.PB.z, k, d0a * d0a, fmin(fmax(d0a, 4.5), 8.0), 1, 0.0, shared, W, next_sh, passes_sh, s, seed,
                  T))
      o.tm_a[p] = s / (double)n1;
  }
}
