// seqalign_body.hpp — sequence alignment with affine gaps (Gotoh, three states) for P pairs of sequences: the one kernel body and the
// host helpers of fdipt_seq_align (seqalign.hip) and fdipt_seq_align_modes (seqalign_modes.hip; section 7.20).
// int32 arithmetic in half units, exact.
//
// One wave per pair, persistent: wave w takes pairs w, w + W, ...; no atomics, no wave waits on another, so no output depends on W.
// The wave walks the anti-diagonals d = i + j; lanes take the cells of a diagonal in chunks of 64.  The live cells sit in LDS, indexed by
// i, IN PLACE: before diagonal d, M/X/Y[i] hold cell (i, d-1-i) and G[i] holds max(M, X, Y) of cell (i, d-2-i) - what M[i+1, d-1-i] adds
// its table entry to.  A cell reads index i-1 and i and writes index i, so a diagonal's chunks run from the highest i down (chunk k reads
// nothing chunk k+1 wrote, and writes nothing chunk k+1 still has to read) and inside a chunk every read precedes every write: four
// buffers, where a rotation would need nine (M of a cell reads all three states two diagonals back).  The 21 x 21 table and the pair's
// letters sit in LDS too.  Several waves share a block while their buffers fit 64 KB; at 2048 letters a block is one wave.
// traceback: a byte per cell (2 bits each: the predecessor state of M, of X, of Y) goes to the wave's slab in the workspace, diagonal by
// diagonal and packed, so a chunk's 64 bytes are contiguous; lane 0 walks the path back, counts it and writes the map.
// score only: the path's counts (identical | aligned in one word, gap runs in 16 bits) ride with every state under the same choices.
//
// A compile-time POLICY says what an entry asks of the body.  The policies fork at the five places marked (1) .. (5); beside them
// local's fresh start (in the recurrence and as the walk back's stop), the boundary handling of the walk back and the span outputs
// (which exist outside SQ_PLAIN only) are noted inline:
// * SQ_PLAIN (fdipt_seq_align): global; the end cell is (la, lb), no state carries an origin, NO_ALIGNED is never set;
// * SQ_ENDS (semi-global; global through the modes entry, which is no flag): a free left end makes the cells of column 0 (A_LEFT) or
//   row 0 (B_LEFT) corners, M = 0; the end cell is chosen among (la, lb), the last column (A_RIGHT) and the last row (B_RIGHT);
// * SQ_LOCAL: no boundary scores; M adds its table entry to max(0, G), and the fresh start (G <= 0) is M's predecessor code 3; the end
//   cell is the inner cell with the best M.
// Where the end cell is a choice, every lane keeps a running best over the candidates it meets - the cells of the last row as it
// computes them, every inner cell's M (local) - and after the last diagonal over the last column, which survives in LDS because index i
// holds cell (i, lb) then (the cell (la, lb) is always a candidate).  A butterfly reduces the bests under the policy's key; a candidate
// is one cell, met by one lane, so the winner is unique and nothing depends on the order.  The bests are reset for every pair a wave
// serves.  Score only, beside the counts every state then carries its origin (begin_a << 12 | begin_b), set at a corner or a fresh
// start and inherited under the same choices; a lane's best carries the counts and the origin of its candidate, and the winning lane
// writes.
#pragma once
#include "common.hpp"

#define SQ_NEG (-(1 << 30))  // unreachable; |reachable| < 2^27 and |every sum with it| < 2^31 under FDIPT_SEQ_MAX_HALF_UNITS
#define SQ_NONE (-2147483647 - 1)
#define SQ_TABLE_BYTES 1792  // 21 * 21 int32, padded to a multiple of 16
#define SQ_LDS_MAX (160 * 1024)

enum { SQ_PLAIN, SQ_ENDS, SQ_LOCAL };
// (1) score only, per index: a count word and a 16-bit run count for each of M, X, Y, G; outside SQ_PLAIN an origin word as well
constexpr int sq_extra(int policy) { return policy == SQ_PLAIN ? 24 : 40; }

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

// a candidate end cell: state st of cell (i, d - i) with score s; score only: its counts, gap runs and origin
struct SqBest {
  int s, d, i, st;
  unsigned c, r, o;
};
// the end-cell keys.  local: score descending, then i + j ascending, then i ascending; else: score, i + j and i descending, then M, X, Y
template <bool LOCAL>
__device__ __forceinline__ bool sq_better(int s, int d, int i, int st, const SqBest& b) {
  if (s != b.s) return s > b.s;
  if (LOCAL) return d != b.d ? d < b.d : i < b.i;
  if (d != b.d) return d > b.d;
  return i != b.i ? i > b.i : st < b.st;
}
template <bool LOCAL>
__device__ __forceinline__ void sq_offer(SqBest& b, int s, int d, int i, int st, unsigned c, unsigned r, unsigned o) {
  if (sq_better<LOCAL>(s, d, i, st, b)) b.s = s, b.d = d, b.i = i, b.st = st, b.c = c, b.r = r, b.o = o;
}

// Args: FdiptSeqAlignArgs (SQ_PLAIN) or FdiptSeqAlignModeArgs, whose free_ends and span outputs are touched outside SQ_PLAIN only
template <int POLICY, bool TRACE, class Args>
__device__ __forceinline__ void seq_align_body(const Args& a, int W, int wpb) {
  constexpr bool PLAIN = POLICY == SQ_PLAIN, ENDS = POLICY == SQ_ENDS, LOCAL = POLICY == SQ_LOCAL;
  constexpr int EXTRA = sq_extra(POLICY);
  extern __shared__ __attribute__((aligned(16))) char sq_smem[];
  int* T = (int*)sq_smem;
  const int tid = threadIdx.x, lane = tid & (FD_WAVE - 1), wave = tid / FD_WAVE;
  for (int k = tid; k < FDIPT_SEQ_LETTERS * FDIPT_SEQ_LETTERS; k += blockDim.x) T[k] = a.table[k];
  __syncthreads();  // the only block barrier: from here on a wave is on its own

  const SqLayout lay = sq_layout(a.max_len_a, a.max_len_b, TRACE, EXTRA);
  const int L1 = lay.L1;
  char* base = sq_smem + SQ_TABLE_BYTES + (size_t)wave * lay.wave_bytes;
  int *Ms = (int*)base, *Xs = Ms + L1, *Ys = Xs + L1, *Gs = Ys + L1;
  char* more = (char*)(Gs + L1);
  unsigned char* Gd = (unsigned char*)more;                                     // TRACE: the state G took
  unsigned *Mc = (unsigned*)more, *Xc = Mc + L1, *Yc = Xc + L1, *Gc = Yc + L1;  // score only: identical << 16 | aligned
  unsigned *Mo = Gc + L1, *Xo = Mo + L1, *Yo = Xo + L1, *Go = Yo + L1;          // score only, not PLAIN: begin_a << 12 | begin_b
  unsigned short *Mr = (unsigned short*)(PLAIN ? Mo : Go + L1), *Xr = Mr + L1, *Yr = Xr + L1, *Gr = Yr + L1;  // score only: gap runs
  unsigned char* sa = (unsigned char*)more + (TRACE ? L1 : L1 * EXTRA);
  unsigned char* sb = sa + lay.LA;

  const int w = blockIdx.x * wpb + wave;
  if (w >= W) return;  // (the last block's spare waves: a slab belongs to one wave)
  const int Sb = a.seq_b ? a.S_b : a.S_a, Nb = a.seq_b ? a.N_b : a.N_a;
  const int32_t* seq_b = a.seq_b ? a.seq_b : a.seq_a;
  const int32_t* len_b = a.seq_b ? a.len_b : a.len_a;
  unsigned char* slab = TRACE ? (unsigned char*)a.workspace + (size_t)w * a.max_len_a * a.max_len_b : nullptr;
  const int o = a.open_gap, e = a.extend_gap;
  int fe = 0;
  if constexpr (ENDS) fe = a.free_ends;
  const bool a_left = fe & FDIPT_SEQ_FREE_A_LEFT, a_right = fe & FDIPT_SEQ_FREE_A_RIGHT;
  const bool b_left = fe & FDIPT_SEQ_FREE_B_LEFT, b_right = fe & FDIPT_SEQ_FREE_B_RIGHT;

  for (long p = w; p < a.P; p += W) {
    sq_wave_sync();  // (the walk of the last pair has read its letters)
    const int ia = a.pairs[2 * p], ib = a.pairs[2 * p + 1];
    const bool found = ia >= 0 && ia < a.S_a && ib >= 0 && ib < Sb;
    int la = found ? a.len_a[ia] : -1, lb = found ? len_b[ib] : -1;
    int status = 0;
    if (la < 0 || lb < 0 || la > a.max_len_a || lb > a.max_len_b || la > a.N_a || lb > Nb) status = FDIPT_SEQ_SKIPPED;
    else if (la == 0 || lb == 0) status = FDIPT_SEQ_EMPTY;
    // the result without a path: zeros, a map of -1, a span of zeros
    auto write_empty = [&](int st) {
      if (TRACE)
        for (int j = lane; j < Nb; j += FD_WAVE) a.alignment[p * Nb + j] = -1;
      if (lane == 0) {
        a.score[p] = 0, a.n_aligned[p] = 0, a.n_identical[p] = 0, a.n_gaps_a[p] = 0, a.n_gaps_b[p] = 0, a.n_gap_runs[p] = 0, a.status[p] = st;
        if constexpr (!PLAIN) a.begin_a[p] = 0, a.end_a[p] = 0, a.begin_b[p] = 0, a.end_b[p] = 0;
      }
    };
    if (status) {  // (wave-uniform)
      write_empty(status);
      continue;
    }
    bool bad = false;
    for (int i = lane; i < la; i += FD_WAVE) {
      int c = a.seq_a[(long)ia * a.N_a + i];
      if (c < 0 || c >= FDIPT_SEQ_LETTERS) c = FDIPT_SEQ_LETTERS - 1, bad = true;
      sa[i] = (unsigned char)c;
    }
    for (int j = lane; j < lb; j += FD_WAVE) {
      int c = seq_b[(long)ib * Nb + j];
      if (c < 0 || c >= FDIPT_SEQ_LETTERS) c = FDIPT_SEQ_LETTERS - 1, bad = true;
      sb[j] = (unsigned char)c;
    }
    if (__ballot(bad) != 0ull) status |= FDIPT_SEQ_BAD_LETTER;

    SqBest best = {SQ_NONE, -1, -1, 0, 0u, 0u, 0u};  // reset for every pair
    for (int d = 0; d <= la + lb; ++d) {
      const int lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
      const int off = TRACE && d >= 2 ? sq_diag_offset(d, la, lb) - (d - lb > 1 ? d - lb : 1) : 0;  // + i: the cell's byte
      for (int k = (hi - lo) / FD_WAVE; k >= 0; --k) {
        const int i = lo + k * FD_WAVE + lane, j = d - i;
        const bool on = i <= hi, inner = on && i >= 1 && j >= 1;
        sq_wave_sync();
        int m = !LOCAL && d == 0 ? 0 : SQ_NEG, x = SQ_NEG, y = SQ_NEG, g = SQ_NEG, gs = 0;
        unsigned mc = 0, xc = 0, yc = 0, gc = 0, mr = 0, xr = 1, yr = 1, gr = 0, mo = 0, xo = 0, yo = 0, go = 0;
        unsigned dir = 0;
        if (inner) {
          const int m1 = Ms[i - 1], x1 = Xs[i - 1], y1 = Ys[i - 1], m0 = Ms[i], x0 = Xs[i], y0 = Ys[i];
          const int ca = sa[i - 1], cb = sb[j - 1];
          // G of cell (i, j-1), for M[i+1, j] two diagonals on
          g = m0, gs = 0;
          if (x0 > g) g = x0, gs = 1;
          if (y0 > g) g = y0, gs = 2;
          const int g1 = Gs[i - 1], gd1 = TRACE ? Gd[i - 1] : 0;  // (read with the rest: a read under `fresh` waits on its own)
          const bool fresh = LOCAL && g1 <= 0;                    // the fresh start wins the tie
          const int dm = fresh ? 3 : gd1;
          m = (fresh ? 0 : g1) + T[ca * FDIPT_SEQ_LETTERS + cb];
          int dx = 0, dy = 0;
          x = m1 + o;
          if (x1 + e > x) x = x1 + e, dx = 1;
          if (y1 + o > x) x = y1 + o, dx = 2;
          y = m0 + o;
          if (x0 + o > y) y = x0 + o, dy = 1;
          if (y0 + e > y) y = y0 + e, dy = 2;
          dir = (unsigned)(dm | dx << 2 | dy << 4);
          if (!TRACE) {
            const unsigned c0[3] = {Mc[i], Xc[i], Yc[i]}, r0[3] = {Mr[i], Xr[i], Yr[i]};
            const unsigned c1[3] = {Mc[i - 1], Xc[i - 1], Yc[i - 1]}, r1[3] = {Mr[i - 1], Xr[i - 1], Yr[i - 1]};
            gc = gs == 0 ? c0[0] : gs == 1 ? c0[1] : c0[2], gr = gs == 0 ? r0[0] : gs == 1 ? r0[1] : r0[2];
            mc = (fresh ? 0u : Gc[i - 1]) + 1u + (ca == cb && ca != FDIPT_SEQ_LETTERS - 1 ? 0x10000u : 0u), mr = fresh ? 0u : Gr[i - 1];
            xc = dx == 0 ? c1[0] : dx == 1 ? c1[1] : c1[2], xr = (dx == 0 ? r1[0] : dx == 1 ? r1[1] : r1[2]) + (dx != 1);
            yc = dy == 0 ? c0[0] : dy == 1 ? c0[1] : c0[2], yr = (dy == 0 ? r0[0] : dy == 1 ? r0[1] : r0[2]) + (dy != 2);
            if constexpr (!PLAIN) {  // the origins, under the same choices
              const unsigned o0[3] = {Mo[i], Xo[i], Yo[i]}, o1[3] = {Mo[i - 1], Xo[i - 1], Yo[i - 1]};
              go = gs == 0 ? o0[0] : gs == 1 ? o0[1] : o0[2], mo = fresh ? (unsigned)((i - 1) << 12 | (j - 1)) : Go[i - 1];
              xo = dx == 0 ? o1[0] : dx == 1 ? o1[1] : o1[2], yo = dy == 0 ? o0[0] : dy == 1 ? o0[1] : o0[2];
            }
          }
          if (LOCAL) sq_offer<LOCAL>(best, m, d, i, 0, mc, mr, mo);  // (3) every inner M
        } else if (on && !LOCAL) {  // (2) row 0 and column 0 (PLAIN: no flag)
          if (j == 0 && i > 0) {
            if (a_left) m = 0, mo = (unsigned)(i << 12);  // a corner
            else x = o + (i - 1) * e;
          }
          if (i == 0 && j > 0) {
            if (b_left) {  // the corners (0, j) and (0, j-1)
              m = 0, mo = (unsigned)j, g = 0, gs = 0, go = (unsigned)(j - 1);
            } else {
              y = o + (j - 1) * e;
              // G of cell (0, j-1): M at the corner, Y beyond it
              g = j == 1 ? 0 : o + (j - 2) * e, gs = j == 1 ? 0 : 2, gr = j == 1 ? 0 : 1;
            }
          }
        }
        if (ENDS && b_right && on && i == la && j < lb) {  // (3) a candidate of the last row
          int s = m, st = 0;
          if (x > s) s = x, st = 1;
          if (y > s) s = y, st = 2;
          sq_offer<LOCAL>(best, s, d, i, st, st == 0 ? mc : st == 1 ? xc : yc, st == 0 ? mr : st == 1 ? xr : yr, st == 0 ? mo : st == 1 ? xo : yo);
        }
        sq_wave_sync();  // every read of the chunk is done
        if (on) {
          Ms[i] = m, Xs[i] = x, Ys[i] = y, Gs[i] = g;
          if (TRACE) {
            Gd[i] = (unsigned char)gs;
            if (inner) slab[off + i] = (unsigned char)dir;
          } else {
            Mc[i] = mc, Xc[i] = xc, Yc[i] = yc, Gc[i] = gc;
            if constexpr (!PLAIN) Mo[i] = mo, Xo[i] = xo, Yo[i] = yo, Go[i] = go;
            Mr[i] = (unsigned short)mr, Xr[i] = (unsigned short)xr, Yr[i] = (unsigned short)yr, Gr[i] = (unsigned short)gr;
          }
        }
      }
    }
    sq_wave_sync();
    // (4) the end cell.  Afterwards every lane holds its key in `win`
    SqBest win;
    if constexpr (PLAIN) {  // index la holds cell (la, lb)
      win.s = Ms[la], win.st = 0, win.d = la + lb, win.i = la;
      if (Xs[la] > win.s) win.s = Xs[la], win.st = 1;
      if (Ys[la] > win.s) win.s = Ys[la], win.st = 2;
    } else {
      if (!LOCAL)  // the last column: index i holds cell (i, lb); the cell (la, lb) always, the others with A_RIGHT
        for (int i = lane; i <= la; i += FD_WAVE) {
          if (i < la && !a_right) continue;
          int s = Ms[i], st = 0;
          if (Xs[i] > s) s = Xs[i], st = 1;
          if (Ys[i] > s) s = Ys[i], st = 2;
          unsigned c = 0, r = 0, og = 0;
          if (!TRACE) c = st == 0 ? Mc[i] : st == 1 ? Xc[i] : Yc[i], r = st == 0 ? Mr[i] : st == 1 ? Xr[i] : Yr[i], og = st == 0 ? Mo[i] : st == 1 ? Xo[i] : Yo[i];
          sq_offer<LOCAL>(best, s, i + lb, i, st, c, r, og);
        }
      // the wave's best: the lane that met it also holds its counts, in `best`
      win = best;
#pragma unroll
      for (int mask = 1; mask < FD_WAVE; mask <<= 1) {
        const int s = __shfl_xor(win.s, mask, FD_WAVE), d = __shfl_xor(win.d, mask, FD_WAVE), i = __shfl_xor(win.i, mask, FD_WAVE), st = __shfl_xor(win.st, mask, FD_WAVE);
        if (sq_better<LOCAL>(s, d, i, st, win)) win.s = s, win.d = d, win.i = i, win.st = st;
      }
      if (LOCAL && win.s <= 0) {  // (wave-uniform) the empty local result; elsewhere (la, lb) was a candidate
        write_empty(status | FDIPT_SEQ_NO_ALIGNED);
        continue;
      }
    }
    const int ei = win.i, ej = win.d - win.i;
    // (5) the counts and the origin: walked back by lane 0, or score only what rode with the end cell's state
    int bi = 0, bj = 0, aligned = 0, identical = 0, runs = 0;
    bool writer = lane == 0;
    if (TRACE) {
      for (int j = ej + lane; j < Nb; j += FD_WAVE) a.alignment[p * Nb + j] = -1;  // (rows begin_b .. end_b-1 are the walk's)
      __threadfence();  // the slab's bytes, written by every lane, are lane 0's to read
      if (lane == 0) {
        int32_t* map = a.alignment + p * Nb;
        int i = ei, j = ej, cur = win.st;
        while (i > 0 && j > 0) {
          const int d = i + j;
          const int byte = slab[sq_diag_offset(d, la, lb) - (d - lb > 1 ? d - lb : 1) + i];
          const int prev = (byte >> (2 * cur)) & 3;
          if (cur == 0) {
            const int ca = sa[i - 1], cb = sb[j - 1];
            ++aligned, identical += ca == cb && ca != FDIPT_SEQ_LETTERS - 1;
            map[j - 1] = i - 1, --i, --j;
            if (LOCAL && prev == 3) break;  // the fresh start: the origin
          } else if (cur == 1) {
            runs += prev != 1, --i;
          } else {
            runs += prev != 2, map[j - 1] = -1, --j;
          }
          cur = prev;
        }
        if (!LOCAL) {  // on the boundary: a corner is the origin; a leading gap that is not free is walked and counted
          if (j == 0 && i > 0 && !a_left) ++runs, i = 0;
          else if (i == 0 && j > 0 && !b_left) {
            ++runs;
            for (; j > 0; --j) map[j - 1] = -1;
          }
        }
        bi = i, bj = j;
      }
      if constexpr (!PLAIN) {  // (PLAIN: begin_b is 0)
        bj = __shfl(bj, 0, FD_WAVE);
        for (int j = lane; j < bj; j += FD_WAVE) a.alignment[p * Nb + j] = -1;
      }
    } else if constexpr (PLAIN) {
      if (lane == 0) {
        const unsigned c = win.st == 0 ? Mc[la] : win.st == 1 ? Xc[la] : Yc[la];
        aligned = (int)(c & 0xffffu), identical = (int)(c >> 16), runs = win.st == 0 ? Mr[la] : win.st == 1 ? Xr[la] : Yr[la];
      }
    } else {
      writer = best.d == win.d && best.i == win.i;  // the one lane that met the winning cell
      aligned = (int)(best.c & 0xffffu), identical = (int)(best.c >> 16), runs = (int)best.r, bi = (int)(best.o >> 12), bj = (int)(best.o & 0xfffu);
    }
    if (writer) {
      a.score[p] = win.s, a.n_aligned[p] = aligned, a.n_identical[p] = identical;
      a.n_gaps_a[p] = ej - bj - aligned, a.n_gaps_b[p] = ei - bi - aligned, a.n_gap_runs[p] = runs;
      if constexpr (!PLAIN) a.begin_a[p] = bi, a.end_a[p] = ei, a.begin_b[p] = bj, a.end_b[p] = ej;
      a.status[p] = PLAIN || aligned ? status : status | FDIPT_SEQ_NO_ALIGNED;
    }
  }
}

// ---- the host side of both entries ----

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

// the argument checks both entries make
template <class Args>
static int sq_check_args(const Args* a) {
  if (!a || a->S_a < 1 || a->N_a < 1 || a->P < 1 || !a->seq_a || !a->len_a || !a->pairs || !a->table) return FDIPT_EINVAL;
  if (a->seq_b && (a->S_b < 1 || a->N_b < 1 || !a->len_b)) return FDIPT_EINVAL;
  if (!a->score || !a->n_aligned || !a->n_identical || !a->n_gaps_a || !a->n_gaps_b || !a->n_gap_runs || !a->status) return FDIPT_EINVAL;
  if (a->traceback && !a->alignment) return FDIPT_EINVAL;
  if (a->open_gap > 0 || a->extend_gap > 0 || a->open_gap < -FDIPT_SEQ_MAX_HALF_UNITS || a->extend_gap < -FDIPT_SEQ_MAX_HALF_UNITS) return FDIPT_EINVAL;
  if (a->max_len_a < 0 || a->max_len_b < 0) return FDIPT_EINVAL;
  if (a->max_len_a > FDIPT_SEQ_MAX_ROWS || a->max_len_b > FDIPT_SEQ_MAX_ROWS) return FDIPT_ESIZE;
  if (a->max_len_a > a->N_a || a->max_len_b > (a->seq_b ? a->N_b : a->N_a)) return FDIPT_EINVAL;
  return FDIPT_OK;
}

// the plan of a launch, its persistent waves W lowered to the slabs the caller's workspace holds
template <class Args>
static int sq_plan_launch(const Args* a, int extra, int& W, int& wpb, size_t& lds) {
  W = sq_plan(a->P, a->max_len_a, a->max_len_b, a->traceback != 0, extra, wpb, lds);
  if (W < 1) return FDIPT_ESIZE;
  const size_t slab = (size_t)a->max_len_a * a->max_len_b;
  if (a->traceback && slab) {
    if (!a->workspace || a->workspace_bytes < slab) return FDIPT_ESIZE;
    if ((size_t)W > a->workspace_bytes / slab) W = (int)(a->workspace_bytes / slab);
  }
  return FDIPT_OK;
}

// launches `kernel`; `attr_dev`: the kernel's own flag that its dynamic-LDS cap is raised on a device
template <class Args>
static int sq_launch(void (*kernel)(Args, int, int), FdPerDevice& attr_dev, const Args* a, int W, int wpb, size_t lds, hipStream_t stream) {
  const int dev_ = fd_device();
  if (lds > 64 * 1024 && !attr_dev.get(dev_)) {
    if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, SQ_LDS_MAX) != hipSuccess) return FDIPT_ELAUNCH;
    attr_dev.set(dev_, 1);
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)cdiv(W, wpb)), dim3((unsigned)(wpb * FD_WAVE)), lds, stream, *a, W, wpb);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
