// seqalign.hip — global sequence alignment with affine gaps (Gotoh, three states) for P pairs of sequences: fdipt_seq_align
// (include/fdipt.h, "sequence alignment").  int32 arithmetic in half units, exact.
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
#include "seqalign_common.hpp"

#define SQ_EXTRA 24  // score only, per index: a count word and a 16-bit run count for each of M, X, Y, G

template <bool TRACE>
__global__ __launch_bounds__(FD_THREADS) void seq_align_kernel(FdiptSeqAlignArgs a, int W, int wpb) {
  extern __shared__ __attribute__((aligned(16))) char sq_smem[];
  int* T = (int*)sq_smem;
  const int tid = threadIdx.x, lane = tid & (FD_WAVE - 1), wave = tid / FD_WAVE;
  for (int k = tid; k < FDIPT_SEQ_LETTERS * FDIPT_SEQ_LETTERS; k += blockDim.x) T[k] = a.table[k];
  __syncthreads();  // the only block barrier: from here on a wave is on its own

  const SqLayout lay = sq_layout(a.max_len_a, a.max_len_b, TRACE, SQ_EXTRA);
  const int L1 = lay.L1;
  char* base = sq_smem + SQ_TABLE_BYTES + (size_t)wave * lay.wave_bytes;
  int *Ms = (int*)base, *Xs = Ms + L1, *Ys = Xs + L1, *Gs = Ys + L1;
  char* more = (char*)(Gs + L1);
  unsigned char* Gd = (unsigned char*)more;                                     // TRACE: the state G took
  unsigned *Mc = (unsigned*)more, *Xc = Mc + L1, *Yc = Xc + L1, *Gc = Yc + L1;  // score only: identical << 16 | aligned
  unsigned short *Mr = (unsigned short*)(Gc + L1), *Xr = Mr + L1, *Yr = Xr + L1, *Gr = Yr + L1;  // score only: gap runs
  unsigned char* sa = (unsigned char*)more + (TRACE ? L1 : 4 * L1 * 4 + 4 * L1 * 2);
  unsigned char* sb = sa + lay.LA;

  const int w = blockIdx.x * wpb + wave;
  if (w >= W) return;  // (the last block's spare waves: a slab belongs to one wave)
  const int Sb = a.seq_b ? a.S_b : a.S_a, Nb = a.seq_b ? a.N_b : a.N_a;
  const int32_t* seq_b = a.seq_b ? a.seq_b : a.seq_a;
  const int32_t* len_b = a.seq_b ? a.len_b : a.len_a;
  unsigned char* slab = TRACE ? (unsigned char*)a.workspace + (size_t)w * a.max_len_a * a.max_len_b : nullptr;
  const int o = a.open_gap, e = a.extend_gap;

  for (long p = w; p < a.P; p += W) {
    sq_wave_sync();  // (the walk of the last pair has read its letters)
    const int ia = a.pairs[2 * p], ib = a.pairs[2 * p + 1];
    const bool found = ia >= 0 && ia < a.S_a && ib >= 0 && ib < Sb;
    int la = found ? a.len_a[ia] : -1, lb = found ? len_b[ib] : -1;
    int status = 0;
    if (la < 0 || lb < 0 || la > a.max_len_a || lb > a.max_len_b || la > a.N_a || lb > Nb) status = FDIPT_SEQ_SKIPPED;
    else if (la == 0 || lb == 0) status = FDIPT_SEQ_EMPTY;
    if (status) {  // (wave-uniform)
      if (TRACE)
        for (int j = lane; j < Nb; j += FD_WAVE) a.alignment[p * Nb + j] = -1;
      if (lane == 0)
        a.score[p] = 0, a.n_aligned[p] = 0, a.n_identical[p] = 0, a.n_gaps_a[p] = 0, a.n_gaps_b[p] = 0, a.n_gap_runs[p] = 0, a.status[p] = status;
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

    for (int d = 0; d <= la + lb; ++d) {
      const int lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
      const int off = TRACE && d >= 2 ? sq_diag_offset(d, la, lb) - (d - lb > 1 ? d - lb : 1) : 0;  // + i: the cell's byte
      for (int k = (hi - lo) / FD_WAVE; k >= 0; --k) {
        const int i = lo + k * FD_WAVE + lane, j = d - i;
        const bool on = i <= hi, inner = on && i >= 1 && j >= 1;
        sq_wave_sync();
        int m = d == 0 ? 0 : SQ_NEG, x = SQ_NEG, y = SQ_NEG, g = SQ_NEG, gs = 0;
        unsigned mc = 0, xc = 0, yc = 0, gc = 0, mr = 0, xr = 1, yr = 1, gr = 0;
        unsigned dir = 0;
        if (inner) {
          const int m1 = Ms[i - 1], x1 = Xs[i - 1], y1 = Ys[i - 1], m0 = Ms[i], x0 = Xs[i], y0 = Ys[i];
          const int ca = sa[i - 1], cb = sb[j - 1];
          // G of cell (i, j-1), for M[i+1, j] two diagonals on
          g = m0, gs = 0;
          if (x0 > g) g = x0, gs = 1;
          if (y0 > g) g = y0, gs = 2;
          const int dm = TRACE ? Gd[i - 1] : 0;
          m = Gs[i - 1] + T[ca * FDIPT_SEQ_LETTERS + cb];
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
            mc = Gc[i - 1] + 1u + (ca == cb && ca != FDIPT_SEQ_LETTERS - 1 ? 0x10000u : 0u), mr = Gr[i - 1];
            xc = dx == 0 ? c1[0] : dx == 1 ? c1[1] : c1[2], xr = (dx == 0 ? r1[0] : dx == 1 ? r1[1] : r1[2]) + (dx != 1);
            yc = dy == 0 ? c0[0] : dy == 1 ? c0[1] : c0[2], yr = (dy == 0 ? r0[0] : dy == 1 ? r0[1] : r0[2]) + (dy != 2);
          }
        } else if (on) {  // row 0 and column 0
          if (j == 0 && i > 0) x = o + (i - 1) * e;
          if (i == 0 && j > 0) {
            y = o + (j - 1) * e;
            // G of cell (0, j-1): M at the corner, Y beyond it
            g = j == 1 ? 0 : o + (j - 2) * e, gs = j == 1 ? 0 : 2, gr = j == 1 ? 0 : 1;
          }
        }
        sq_wave_sync();  // every read of the chunk is done
        if (on) {
          Ms[i] = m, Xs[i] = x, Ys[i] = y, Gs[i] = g;
          if (TRACE) {
            Gd[i] = (unsigned char)gs;
            if (inner) slab[off + i] = (unsigned char)dir;
          } else {
            Mc[i] = mc, Xc[i] = xc, Yc[i] = yc, Gc[i] = gc;
            Mr[i] = (unsigned short)mr, Xr[i] = (unsigned short)xr, Yr[i] = (unsigned short)yr, Gr[i] = (unsigned short)gr;
          }
        }
      }
    }
    sq_wave_sync();
    // the end cell: index la
    const int me = Ms[la], xe = Xs[la], ye = Ys[la];
    int score = me, cur = 0;
    if (xe > score) score = xe, cur = 1;
    if (ye > score) score = ye, cur = 2;
    int aligned = 0, identical = 0, runs = 0;
    if (TRACE) {
      for (int j = lb + lane; j < Nb; j += FD_WAVE) a.alignment[p * Nb + j] = -1;  // (rows 0 .. lb-1 are the walk's)
      __threadfence();  // the slab's bytes, written by every lane, are lane 0's to read
      if (lane == 0) {
        int32_t* map = a.alignment + p * Nb;
        int i = la, j = lb;
        while (i > 0 && j > 0) {
          const int d = i + j;
          const int byte = slab[sq_diag_offset(d, la, lb) - (d - lb > 1 ? d - lb : 1) + i];
          const int prev = (byte >> (2 * cur)) & 3;
          if (cur == 0) {
            const int ca = sa[i - 1], cb = sb[j - 1];
            ++aligned, identical += ca == cb && ca != FDIPT_SEQ_LETTERS - 1;
            map[j - 1] = i - 1, --i, --j;
          } else if (cur == 1) {
            runs += prev != 1, --i;
          } else {
            runs += prev != 2, map[j - 1] = -1, --j;
          }
          cur = prev;
        }
        if (i > 0 || j > 0) ++runs;  // the leading gap: X down column 0 or Y along row 0
        for (; j > 0; --j) map[j - 1] = -1;
      }
    } else if (lane == 0) {
      const unsigned c = cur == 0 ? Mc[la] : cur == 1 ? Xc[la] : Yc[la];
      aligned = (int)(c & 0xffffu), identical = (int)(c >> 16), runs = cur == 0 ? Mr[la] : cur == 1 ? Xr[la] : Yr[la];
    }
    if (lane == 0) {
      a.score[p] = score, a.n_aligned[p] = aligned, a.n_identical[p] = identical, a.n_gaps_a[p] = lb - aligned, a.n_gaps_b[p] = la - aligned;
      a.n_gap_runs[p] = runs, a.status[p] = status;
    }
  }
}

extern "C" size_t fdipt_seq_align_workspace_bytes(int P, int max_len_a, int max_len_b, int traceback, size_t max_workspace_bytes) {
  return sq_workspace_bytes(P, max_len_a, max_len_b, traceback, max_workspace_bytes, SQ_EXTRA);
}

template <bool TRACE>
static int sq_launch(const FdiptSeqAlignArgs* a, int W, int wpb, size_t lds, hipStream_t stream) {
  static FdPerDevice attr_dev;
  const int dev_ = fd_device();
  if (lds > 64 * 1024 && !attr_dev.get(dev_)) {
    if (hipFuncSetAttribute((const void*)seq_align_kernel<TRACE>, hipFuncAttributeMaxDynamicSharedMemorySize, SQ_LDS_MAX) != hipSuccess) return FDIPT_ELAUNCH;
    attr_dev.set(dev_, 1);
  }
  hipLaunchKernelGGL(seq_align_kernel<TRACE>, dim3((unsigned)cdiv(W, wpb)), dim3((unsigned)(wpb * FD_WAVE)), lds, stream, *a, W, wpb);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}

extern "C" int fdipt_seq_align(const FdiptSeqAlignArgs* a, fdipt_stream_t stream) {
  if (!a || a->S_a < 1 || a->N_a < 1 || a->P < 1 || !a->seq_a || !a->len_a || !a->pairs || !a->table) return FDIPT_EINVAL;
  if (a->seq_b && (a->S_b < 1 || a->N_b < 1 || !a->len_b)) return FDIPT_EINVAL;
  if (!a->score || !a->n_aligned || !a->n_identical || !a->n_gaps_a || !a->n_gaps_b || !a->n_gap_runs || !a->status) return FDIPT_EINVAL;
  if (a->traceback && !a->alignment) return FDIPT_EINVAL;
  if (a->open_gap > 0 || a->extend_gap > 0 || a->open_gap < -FDIPT_SEQ_MAX_HALF_UNITS || a->extend_gap < -FDIPT_SEQ_MAX_HALF_UNITS) return FDIPT_EINVAL;
  if (a->max_len_a < 0 || a->max_len_b < 0) return FDIPT_EINVAL;
  if (a->max_len_a > FDIPT_SEQ_MAX_ROWS || a->max_len_b > FDIPT_SEQ_MAX_ROWS) return FDIPT_ESIZE;
  if (a->max_len_a > a->N_a || a->max_len_b > (a->seq_b ? a->N_b : a->N_a)) return FDIPT_EINVAL;
  int wpb;
  size_t lds;
  int W = sq_plan(a->P, a->max_len_a, a->max_len_b, a->traceback != 0, SQ_EXTRA, wpb, lds);
  if (W < 1) return FDIPT_ESIZE;
  const size_t slab = (size_t)a->max_len_a * a->max_len_b;
  if (a->traceback && slab) {
    if (!a->workspace || a->workspace_bytes < slab) return FDIPT_ESIZE;
    if ((size_t)W > a->workspace_bytes / slab) W = (int)(a->workspace_bytes / slab);
  }
  return a->traceback ? sq_launch<true>(a, W, wpb, lds, (hipStream_t)stream) : sq_launch<false>(a, W, wpb, lds, (hipStream_t)stream);
}
