// lddt_body.hpp — the pair and reduce kernels of the superposition-free accuracy entries as device functions with a MAPPED switch:
// lddt.hip instantiates them for structures in row correspondence (fdipt_sample_lddt), lddt_mapped.hip for a model read through a row
// map (fdipt_sample_lddt_mapped).  The un-mapped instantiations compile to what they were before the switch existed.
//
// Two launches on one stream, nothing between them on the host:
//   pair kernel    a block serves FD_WAVES rows of one pair, a wave per row i.  The rows j of both structures pass through LDS in tiles
//                  of TILE rows (256 at <= 4 atoms per row, 64 at 37: a block's LDS stays below 64 KB, two blocks and more per CU); lane
//                  l takes j = l, l + 64, ... ascending.  Row i's atoms sit in LDS too (37 atoms of two structures do not fit a lane's
//                  registers), its two frames in registers.  Per tile and atom u of row i the lanes count the scored pairs (u, v) and
//                  the four threshold counts in 16-bit fields of three words, a butterfly sums them and lane u keeps atom u's totals.
//                  FAPE and dRMSD ride on the same tiles: each lane's terms in ascending j, one butterfly at the end.
//   reduce kernel  a block per pair: row i to thread i % 256, a thread's rows ascending, butterfly inside a wave, the waves in index
//                  order (fd_block_sum): the pair's integer totals and the three float sums.
// Integers only for lDDT: its scores are formed from the counts as the reference forms them, so no order of anything changes a bit.
// No floating-point atomics: rows appended behind a structure and a pair's batch mates change no bit.
//
// MAPPED: the rows are the reference's (N = N_b); the staging loop and the row-i prologue read the model's row map[j] - a gather of one
// row of atoms * 12 bytes per map entry - and an atom carries two bits, LD_IN_REF (it exists in the reference) and LD_IN_BOTH (and is
// present in the gathered model).  FAPE, dRMSD and the threshold counts ask for LD_IN_BOTH; the scored count asks for it under
// FDIPT_MAP_IGNORE and for LD_IN_REF under FDIPT_MAP_PENALISE.  A verdict on the map (lddt_mapped.hip's pre-pass) sits behind the
// workspace of the un-mapped entry; the blocks of a pair with a bad map return as those of a pair with a bad index do.
#pragma once
#include "rowmap.hpp"

#pragma clang fp contract(off)  // the distances keep the evaluation order of the reference's expressions

#define LD_EPS 1e-10        // lddt's eps: inside its square roots and in its two denominators
#define LD_FRAME_EPS 1e-8   // from_3_points
#define LD_FAPE_EPS 1e-4    // backbone_loss's eps: under compute_fape's square root and in its denominators
#define LD_FAPE_CLAMP 10.0  // clamp_distance
#define LD_FAPE_UNIT 10.0   // loss_unit_distance
// flags of a row in the workspace
#define LD_ROW_SCORE 1
#define LD_ROW_FRAME 2
#define LD_ROW_POINT 4
#define LD_ROW_DRMSD 8
#define LD_ROW_EMPTY 16  // a score row without a scored pair
// bits of an atom in the mapped instantiations (the un-mapped ones keep one bool: the atom takes part)
#define LD_IN_REF 1
#define LD_IN_BOTH 2

static inline int ld_set_atoms(int mode) { return mode == FDIPT_LDDT_CA ? 1 : mode == FDIPT_LDDT_BACKBONE ? 4 : 37; }
// the column of atom k of the set in a layout of `atoms` atoms per row
template <int K>
__device__ __forceinline__ int ld_column(int atoms, int k) {
  if constexpr (K == 1) return atoms == 1 ? 0 : 1;
  else if constexpr (K == 4) return k == 3 ? 4 : k;
  else return k;
}

// one structure of a pair: its coordinates and atom mask from row 0 on
struct LdStructure {
  const float* x;
  const unsigned char* m;
  int atoms;
};
// atom `col` of `row`: its coordinates, and whether it exists
__device__ __forceinline__ bool ld_atom(const LdStructure& s, int row, int col, float (&v)[3]) {
  const long at = (long)row * s.atoms + col;
  const float* p = s.x + at * 3;
  v[0] = p[0];
  v[1] = p[1];
  v[2] = p[2];
  return s.m ? s.m[at] != 0 : (v[0] != 0.f || v[1] != 0.f || v[2] != 0.f);
}
// atom `col` of the model's row `row`; MAPPED: `row` is the model row of a reference row, or -1 (no atom, zeros)
template <bool MAPPED>
__device__ __forceinline__ bool ld_model_atom(const LdStructure& s, int row, int col, float (&v)[3]) {
  if constexpr (MAPPED) {
    if (row < 0) {
      v[0] = v[1] = v[2] = 0.f;
      return false;
    }
  }
  return ld_atom(s, row, col, v);
}
// what an atom carries from whether it is present in the model (a) and exists in the reference (b)
template <bool MAPPED>
__device__ __forceinline__ auto ld_part(bool a, bool b) {
  if constexpr (MAPPED) return (unsigned char)(b ? (a ? LD_IN_REF | LD_IN_BOTH : LD_IN_REF) : 0);
  else return a & b;
}
// the atom takes part: it is in both structures
template <bool MAPPED>
__device__ __forceinline__ bool ld_takes(unsigned part) {
  if constexpr (MAPPED) return (part & LD_IN_BOTH) != 0;
  else return part != 0;
}
// the atom enters the scored count; gate: LD_IN_BOTH (ignore) or LD_IN_REF (penalise)
template <bool MAPPED>
__device__ __forceinline__ bool ld_counts(unsigned part, unsigned gate) {
  if constexpr (MAPPED) return (part & gate) != 0;
  else return part != 0;
}

// where the verdicts on the maps of a mapped call sit: behind the workspace of the un-mapped entry
__device__ __forceinline__ int* ld_verdicts(const FdiptLddtArgs& a) {
  return (int*)((char*)a.workspace + (size_t)a.P * a.N * (2 * sizeof(double) + sizeof(int)));
}

// the pair's two structures and its rows' masks; false where an index is out of range
__device__ __forceinline__ bool ld_pair(const FdiptLddtArgs& a, int p, LdStructure& sa, LdStructure& sb, const float*& rm, const float*& sm) {
  const int ia = a.pairs[2 * p], ib = a.pairs[2 * p + 1], s_b = a.prot_b ? a.S_b : a.S;
  if (ia < 0 || ia >= a.S || ib < 0 || ib >= s_b) return false;
  const int atoms_b = a.prot_b ? a.atoms_b : a.atoms;
  sa = {a.prot + (long)ia * a.N * a.atoms * 3, a.atom_mask_a ? a.atom_mask_a + (long)ia * a.N * a.atoms : nullptr, a.atoms};
  sb = {(a.prot_b ? a.prot_b : a.prot) + (long)ib * a.N * atoms_b * 3, a.atom_mask_b ? a.atom_mask_b + (long)ib * a.N * atoms_b : nullptr, atoms_b};
  rm = a.res_mask + (long)ia * a.N;
  sm = a.score_mask + (long)ia * a.N;
  return true;
}
// the same of a mapped call: the model has m.N_a rows, the rows' masks are the reference's, rma the model's row mask and mp the pair's
// map; false where an index is out of range or the map was refused
__device__ __forceinline__ bool ld_pair_mapped(const FdiptLddtArgs& a, const FdiptRowMap& m, int p, LdStructure& sa, LdStructure& sb, const float*& rm,
                                               const float*& sm, const float*& rma, const int*& mp) {
  const int ia = a.pairs[2 * p], ib = a.pairs[2 * p + 1];
  if (ia < 0 || ia >= a.S || ib < 0 || ib >= a.S_b || ld_verdicts(a)[p] != 0) return false;
  sa = {a.prot + (long)ia * m.N_a * a.atoms * 3, a.atom_mask_a ? a.atom_mask_a + (long)ia * m.N_a * a.atoms : nullptr, a.atoms};
  sb = {a.prot_b + (long)ib * a.N * a.atoms_b * 3, a.atom_mask_b ? a.atom_mask_b + (long)ib * a.N * a.atoms_b : nullptr, a.atoms_b};
  rm = m.res_mask_b + (long)ib * a.N;
  sm = m.score_mask_b + (long)ib * a.N;
  rma = a.res_mask + (long)ia * m.N_a;
  mp = m.map + (long)p * a.N;
  return true;
}

__device__ __forceinline__ double ld_sum_sq(double x, double y, double z) { return (x * x + y * y) + z * z; }
__device__ __forceinline__ double ld_score(long long c, long long n0, long long n1, long long n2, long long n3) {
  const double norm = 1.0 / (LD_EPS + (double)c);
  return norm * (LD_EPS + 0.25 * (double)(n0 + n1 + n2 + n3));
}

// the backbone frame of a row from its N, CA, C: the axes e0, e1, e2 (the frame's columns are -e0, e1, -e2: the signs cancel in every
// difference of two local points) and the origin
struct LdFrame {
  double e0[3], e1[3], e2[3], t[3];
};
__device__ __forceinline__ void ld_frame(const float (&n)[3], const float (&ca)[3], const float (&c)[3], LdFrame& f) {
  double b[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    f.t[k] = (double)ca[k];
    f.e0[k] = (double)ca[k] - (double)c[k];
    b[k] = (double)n[k] - (double)ca[k];
  }
  double d = sqrt(ld_sum_sq(f.e0[0], f.e0[1], f.e0[2]) + LD_FRAME_EPS);
#pragma unroll
  for (int k = 0; k < 3; ++k) f.e0[k] = f.e0[k] / d;
  const double dot = (f.e0[0] * b[0] + f.e0[1] * b[1]) + f.e0[2] * b[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) f.e1[k] = b[k] - f.e0[k] * dot;
  d = sqrt(ld_sum_sq(f.e1[0], f.e1[1], f.e1[2]) + LD_FRAME_EPS);
#pragma unroll
  for (int k = 0; k < 3; ++k) f.e1[k] = f.e1[k] / d;
  f.e2[0] = f.e0[1] * f.e1[2] - f.e0[2] * f.e1[1];
  f.e2[1] = f.e0[2] * f.e1[0] - f.e0[0] * f.e1[2];
  f.e2[2] = f.e0[0] * f.e1[1] - f.e0[1] * f.e1[0];
}
__device__ __forceinline__ void ld_local(const LdFrame& f, double x, double y, double z, double (&l)[3]) {
  const double dx = x - f.t[0], dy = y - f.t[1], dz = z - f.t[2];
  l[0] = (f.e0[0] * dx + f.e0[1] * dy) + f.e0[2] * dz;
  l[1] = (f.e1[0] * dx + f.e1[1] * dy) + f.e1[2] * dz;
  l[2] = (f.e2[0] * dx + f.e2[1] * dy) + f.e2[2] * dz;
}
__device__ __forceinline__ unsigned ld_wave_sum_u(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int K, int TILE, bool MAPPED>
__device__ __forceinline__ void lddt_pair_body(const FdiptLddtArgs& a, int tiles, const FdiptRowMap& m) {
  static_assert(K <= FD_WAVE && TILE % FD_WAVE == 0 && TILE * K < 65536, "a lane per atom of row i; 16-bit counts per tile");
  constexpr int CA = K == 1 ? 0 : 1;  // the CA atom inside the set
  __shared__ float xs[2][K * 3][TILE];        // [structure][atom, axis][row of the tile]
  __shared__ unsigned char part_sh[K][TILE];  // the atom takes part (MAPPED: LD_IN_* bits)
  __shared__ unsigned char row_sh[TILE];      // 1: the row exists, 2: it is a score row
  __shared__ float xi_sh[FD_WAVES][2][K * 3];
  __shared__ unsigned char parti_sh[FD_WAVES][K];
  const int tid = threadIdx.x, lane = tid & (FD_WAVE - 1), wave = tid / FD_WAVE, N = a.N;
  const int p = blockIdx.x / tiles, i = (blockIdx.x % tiles) * FD_WAVES + wave;
  LdStructure sa, sb;
  const float *rm, *sm, *rma = nullptr;
  const int* mp = nullptr;
  if constexpr (MAPPED) {
    if (!ld_pair_mapped(a, m, p, sa, sb, rm, sm, rma, mp)) return;
  } else {
    if (!ld_pair(a, p, sa, sb, rm, sm)) return;  // (the whole block; the reduce kernel writes the pair's zeros)
  }
  const bool mine = i < N && rm[i < N ? i : 0] != 0.f;  // (the same in every lane of a wave)
  const bool score_row = mine && sm[i < N ? i : 0] != 0.f;
  bool frame_row = false, ca_i = false;
  LdFrame fa, fb;
  if (mine) {
    int ri = i;  // the model's row of row i
    if constexpr (MAPPED) ri = fd_map_row(mp, rma, m.N_a, i);
    if (lane < K) {
      float va[3], vb[3];
      const auto part =
          ld_part<MAPPED>(ld_model_atom<MAPPED>(sa, ri, ld_column<K>(sa.atoms, lane), va), ld_atom(sb, i, ld_column<K>(sb.atoms, lane), vb));
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        xi_sh[wave][0][lane * 3 + c] = va[c];
        xi_sh[wave][1][lane * 3 + c] = vb[c];
      }
      parti_sh[wave][lane] = part;
    }
    float na[3], caa[3], cca[3], nb[3], cab[3], ccb[3];
    const int ca_a = sa.atoms == 1 ? 0 : 1, ca_b = sb.atoms == 1 ? 0 : 1;
    ca_i = ld_model_atom<MAPPED>(sa, ri, ca_a, caa) & ld_atom(sb, i, ca_b, cab);
    if (sa.atoms > 1 && sb.atoms > 1) {
      frame_row = ca_i & ld_model_atom<MAPPED>(sa, ri, 0, na) & ld_atom(sb, i, 0, nb) & ld_model_atom<MAPPED>(sa, ri, 2, cca) & ld_atom(sb, i, 2, ccb);
      if (frame_row) {
        ld_frame(na, caa, cca, fa);
        ld_frame(nb, cab, ccb, fb);
      }
    }
  }
  const bool drmsd_row = score_row && ca_i;
  unsigned gate = LD_IN_BOTH;  // what an atom needs to enter the scored count
  if constexpr (MAPPED) gate = m.coverage == FDIPT_MAP_PENALISE ? LD_IN_REF : LD_IN_BOTH;
  int cnt[5] = {0, 0, 0, 0, 0};  // lane u: c, n_0.5, n_1, n_2, n_4 of atom u of row i
  double fape_sum = 0.0, drmsd_sum = 0.0;
  int points = 0;
  for (int j0 = 0; j0 < N; j0 += TILE) {
    __syncthreads();
    for (int e = tid; e < TILE * K; e += FD_THREADS) {
      const int r = e / K, k = e % K, j = j0 + r;
      const bool ex = j < N && rm[j < N ? j : 0] != 0.f;
      float va[3] = {0.f, 0.f, 0.f}, vb[3] = {0.f, 0.f, 0.f};
      decltype(ld_part<MAPPED>(false, false)) part = 0;
      if (ex) {
        int rj = j;
        if constexpr (MAPPED) rj = fd_map_row(mp, rma, m.N_a, j);
        part = ld_part<MAPPED>(ld_model_atom<MAPPED>(sa, rj, ld_column<K>(sa.atoms, k), va), ld_atom(sb, j, ld_column<K>(sb.atoms, k), vb));
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        xs[0][k * 3 + c][r] = va[c];
        xs[1][k * 3 + c][r] = vb[c];
      }
      part_sh[k][r] = part;
      if (k == 0) row_sh[r] = ex ? (sm[j] != 0.f ? 3 : 1) : 0;
    }
    __syncthreads();
    if (!mine) continue;
    // FAPE points and dRMSD partners: the CA atoms of the tile
    if (frame_row || drmsd_row) {
      const double xia = (double)xi_sh[wave][0][CA * 3], yia = (double)xi_sh[wave][0][CA * 3 + 1], zia = (double)xi_sh[wave][0][CA * 3 + 2];
      const double xib = (double)xi_sh[wave][1][CA * 3], yib = (double)xi_sh[wave][1][CA * 3 + 1], zib = (double)xi_sh[wave][1][CA * 3 + 2];
      for (int jl = lane; jl < TILE; jl += FD_WAVE) {
        const int flags = row_sh[jl];
        if (!(flags & 1) || !ld_takes<MAPPED>(part_sh[CA][jl])) continue;
        const double xja = (double)xs[0][CA * 3][jl], yja = (double)xs[0][CA * 3 + 1][jl], zja = (double)xs[0][CA * 3 + 2][jl];
        const double xjb = (double)xs[1][CA * 3][jl], yjb = (double)xs[1][CA * 3 + 1][jl], zjb = (double)xs[1][CA * 3 + 2][jl];
        if (frame_row) {
          double la[3], lb[3];
          ld_local(fa, xja, yja, zja, la);
          ld_local(fb, xjb, yjb, zjb, lb);
          const double d = sqrt(ld_sum_sq(la[0] - lb[0], la[1] - lb[1], la[2] - lb[2]) + LD_FAPE_EPS);
          fape_sum += fmin(d, LD_FAPE_CLAMP) / LD_FAPE_UNIT;
          points += 1;
        }
        if (drmsd_row && (flags & 2) && j0 + jl != i) {
          const double da = sqrt(ld_sum_sq(xia - xja, yia - yja, zia - zja)), db = sqrt(ld_sum_sq(xib - xjb, yib - yjb, zib - zjb));
          drmsd_sum += (da - db) * (da - db);
        }
      }
    }
    if (!score_row) continue;
    for (int u = 0; u < K; ++u) {
      const unsigned pu = parti_sh[wave][u];
      if (!ld_counts<MAPPED>(pu, gate)) continue;  // (wave-uniform)
      const double xua = (double)xi_sh[wave][0][u * 3], yua = (double)xi_sh[wave][0][u * 3 + 1], zua = (double)xi_sh[wave][0][u * 3 + 2];
      const double xub = (double)xi_sh[wave][1][u * 3], yub = (double)xi_sh[wave][1][u * 3 + 1], zub = (double)xi_sh[wave][1][u * 3 + 2];
      unsigned w0 = 0u, w1 = 0u, w2 = 0u;  // c | n_0.5 << 16, n_1 | n_2 << 16, n_4
      for (int jl = lane; jl < TILE; jl += FD_WAVE) {
        if (!(row_sh[jl] & 1)) continue;
        const bool same = j0 + jl == i;
        if (same && (K == 1 || !a.same_residue)) continue;
        for (int v = 0; v < K; ++v) {
          const unsigned pv = part_sh[v][jl];
          if (!ld_counts<MAPPED>(pv, gate) || (same && v == u)) continue;
          const double db = sqrt(LD_EPS + ld_sum_sq(xub - (double)xs[1][v * 3][jl], yub - (double)xs[1][v * 3 + 1][jl], zub - (double)xs[1][v * 3 + 2][jl]));
          if (!(db < a.cutoff)) continue;
          const double da = sqrt(LD_EPS + ld_sum_sq(xua - (double)xs[0][v * 3][jl], yua - (double)xs[0][v * 3 + 1][jl], zua - (double)xs[0][v * 3 + 2][jl]));
          const double l1 = fabs(db - da);
          if constexpr (MAPPED) {  // a pair passes only where both of its atoms are present in the gathered model
            const bool both = (pu & pv & LD_IN_BOTH) != 0;
            w0 += 1u + ((both && l1 < 0.5 ? 1u : 0u) << 16);
            w1 += (both && l1 < 1.0 ? 1u : 0u) + ((both && l1 < 2.0 ? 1u : 0u) << 16);
            w2 += both && l1 < 4.0 ? 1u : 0u;
          } else {
            w0 += 1u + ((l1 < 0.5 ? 1u : 0u) << 16);
            w1 += (l1 < 1.0 ? 1u : 0u) + ((l1 < 2.0 ? 1u : 0u) << 16);
            w2 += l1 < 4.0 ? 1u : 0u;
          }
        }
      }
      w0 = ld_wave_sum_u(w0);
      w1 = ld_wave_sum_u(w1);
      w2 = ld_wave_sum_u(w2);
      if (lane == u) {
        cnt[0] += (int)(w0 & 0xffffu);
        cnt[1] += (int)(w0 >> 16);
        cnt[2] += (int)(w1 & 0xffffu);
        cnt[3] += (int)(w1 >> 16);
        cnt[4] += (int)w2;
      }
    }
  }
  if (i >= N) return;
  const long row = (long)p * N + i;
  if (a.atom_lddt && lane < K) a.atom_lddt[row * K + lane] = score_row ? ld_score(cnt[0], cnt[1], cnt[2], cnt[3], cnt[4]) : 0.0;
  int tot[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) tot[k] = (int)ld_wave_sum_u((unsigned)cnt[k]);
  fape_sum = wave_sum_d(fape_sum);
  drmsd_sum = wave_sum_d(drmsd_sum);
  points = (int)ld_wave_sum_u((unsigned)points);
  if (lane == 0) {
    double* fape_ws = (double*)a.workspace;
    double* drmsd_ws = fape_ws + (long)a.P * N;
    int* flags_ws = (int*)(drmsd_ws + (long)a.P * N);
    a.res_lddt[row] = score_row ? ld_score(tot[0], tot[1], tot[2], tot[3], tot[4]) : 0.0;
    a.n_scored[row] = tot[0];
#pragma unroll
    for (int k = 0; k < 4; ++k) a.n_passed[row * 4 + k] = tot[1 + k];
    a.res_fape[row] = frame_row ? fape_sum / (LD_FAPE_EPS + (double)points) : 0.0;
    fape_ws[row] = frame_row ? fape_sum : 0.0;
    drmsd_ws[row] = drmsd_sum;
    flags_ws[row] = (score_row ? LD_ROW_SCORE : 0) | (frame_row ? LD_ROW_FRAME : 0) | (mine && ca_i ? LD_ROW_POINT : 0) | (drmsd_row ? LD_ROW_DRMSD : 0) |
                    (score_row && tot[0] == 0 ? LD_ROW_EMPTY : 0);
  }
}

template <bool MAPPED>
__device__ __forceinline__ void lddt_reduce_body(const FdiptLddtArgs& a, int set_atoms, const FdiptRowMap& m) {
  __shared__ double red_d[FD_WAVES * 3];
  __shared__ long long red_i[FD_WAVES * 10];
  const int tid = threadIdx.x, N = a.N, p = blockIdx.x;
  const long row0 = (long)p * N;
  LdStructure sa, sb;
  const float *rm, *sm;
  bool ok;
  if constexpr (MAPPED) {
    const float* rma;
    const int* mp;
    ok = ld_pair_mapped(a, m, p, sa, sb, rm, sm, rma, mp);
  } else {
    ok = ld_pair(a, p, sa, sb, rm, sm);
  }
  if (!ok) {
    for (int i = tid; i < N; i += FD_THREADS) {
      a.res_lddt[row0 + i] = 0.0;
      a.res_fape[row0 + i] = 0.0;
      a.n_scored[row0 + i] = 0;
      for (int k = 0; k < 4; ++k) a.n_passed[(row0 + i) * 4 + k] = 0;
      if (a.atom_lddt)
        for (int k = 0; k < set_atoms; ++k) a.atom_lddt[(row0 + i) * set_atoms + k] = 0.0;
    }
    if (tid == 0) {
      a.lddt[p] = a.drmsd[p] = a.fape[p] = a.region_fape[p] = 0.0;
      if constexpr (MAPPED) a.status[p] = ld_verdicts(a)[p];  // (FDIPT_LDDT_SKIPPED or the map's bits: the pre-pass wrote them)
      else a.status[p] = FDIPT_LDDT_SKIPPED;
    }
    return;
  }
  const double* fape_ws = (const double*)a.workspace;
  const double* drmsd_ws = fape_ws + (long)a.P * N;
  const int* flags_ws = (const int*)(drmsd_ws + (long)a.P * N);
  // 0..4: c and the four n_t of the score rows, 5: frames, 6: points, 7: dRMSD rows, 8: score rows with a frame, 9: score rows without a pair
  long long is[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = tid; i < N; i += FD_THREADS) {
    if (rm[i] == 0.f) continue;
    const int flags = flags_ws[row0 + i];
    if (flags & LD_ROW_SCORE) {
      is[0] += a.n_scored[row0 + i];
#pragma unroll
      for (int k = 0; k < 4; ++k) is[1 + k] += a.n_passed[(row0 + i) * 4 + k];
    }
    is[5] += (flags & LD_ROW_FRAME) != 0;
    is[6] += (flags & LD_ROW_POINT) != 0;
    is[7] += (flags & LD_ROW_DRMSD) != 0;
    is[8] += (flags & LD_ROW_FRAME) && (flags & LD_ROW_SCORE);
    is[9] += (flags & LD_ROW_EMPTY) != 0;
  }
  fd_block_sum(is, red_i);
  const double frames = (double)is[5];
  // 0: compute_fape's inner mean summed over the frames, 1: the squared distance differences, 2: res_fape of the score rows with a frame
  double fs[3] = {0.0, 0.0, 0.0};
  for (int i = tid; i < N; i += FD_THREADS) {
    if (rm[i] == 0.f) continue;
    const int flags = flags_ws[row0 + i];
    if (flags & LD_ROW_FRAME) fs[0] += fape_ws[row0 + i] / (LD_FAPE_EPS + frames);
    if (flags & LD_ROW_DRMSD) fs[1] += drmsd_ws[row0 + i];
    if ((flags & LD_ROW_FRAME) && (flags & LD_ROW_SCORE)) fs[2] += a.res_fape[row0 + i];
  }
  fd_block_sum(fs, red_d);
  if (tid == 0) {
    const double n = (double)is[7];
    a.lddt[p] = ld_score(is[0], is[1], is[2], is[3], is[4]);
    a.drmsd[p] = is[7] > 1 ? sqrt(fs[1] * (1.0 / (n * (n - 1.0)))) : 0.0;
    a.fape[p] = is[5] > 0 ? fs[0] / (LD_FAPE_EPS + (double)is[6]) : 0.0;
    a.region_fape[p] = is[8] > 0 ? fs[2] / (double)is[8] : 0.0;
    a.status[p] = (is[9] > 0 ? FDIPT_LDDT_NO_PARTNER : 0) | (is[5] == 0 ? FDIPT_LDDT_NO_FRAME : 0);
  }
}

// the argument checks the two entries share; score_mask: the one the entry reads
static inline int ld_check_args(const FdiptLddtArgs* a, const float* score_mask) {
  if (!a || a->S < 1 || a->N < 1 || a->P < 1 || a->mode < FDIPT_LDDT_CA || a->mode > FDIPT_LDDT_ALL || !(a->cutoff > 0.0)) return FDIPT_EINVAL;
  const int atoms_b = a->prot_b ? a->atoms_b : a->atoms;
  for (int atoms : {a->atoms, atoms_b}) {
    if (atoms != 37 && atoms != 5 && atoms != 1) return FDIPT_EINVAL;
    if ((a->mode == FDIPT_LDDT_ALL && atoms != 37) || (a->mode == FDIPT_LDDT_BACKBONE && atoms == 1)) return FDIPT_EINVAL;
  }
  if (a->prot_b && a->S_b < 1) return FDIPT_EINVAL;
  if (!a->prot || !a->res_mask || !score_mask || !a->pairs || !a->lddt || !a->res_lddt || !a->n_scored || !a->n_passed || !a->drmsd || !a->fape || !a->res_fape ||
      !a->region_fape || !a->status || !a->workspace)
    return FDIPT_EINVAL;
  const long tiles = cdiv(a->N, FD_WAVES), K = ld_set_atoms(a->mode);
  if (tiles * a->P > 0x7fffffffL || (long)a->N * K * K > 0x7fffffffL) return FDIPT_ESIZE;
  return FDIPT_OK;
}
