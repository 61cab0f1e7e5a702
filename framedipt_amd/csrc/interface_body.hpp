// interface_body.hpp — the prep and rmsd kernels of the interface accuracy entries as device functions with a MAPPED switch, and what
// their contact kernels share (include/fdipt.h, "interface accuracy"; DESIGN.md sections 7.18 and 7.19): interface.hip instantiates the
// bodies for structures in row correspondence (fdipt_sample_interface), interface_mapped.hip for a model read through a row map
// (fdipt_sample_interface_mapped).  The bodies take their arguments by value, as the kernels do.  The CONTACT kernel is not here: it
// stands in full in each of the two units, seven lines apart, because as an instantiation of a shared body its unpruned all-atom pass
// measured 1.2 % slower than the kernel it replaced.
//
// Three launches on one stream, nothing between them on the host (the mapped entry: interface_mapped.hip's map kernel in front):
//   prep kernel     a block per pair: per row the atoms of the set that take part (they exist in both structures), the RMSD atoms, and
//                   the row's reach in both structures (largest CA-to-atom distance) go to the workspace; the per-row outputs of the
//                   pair are zeroed.
//   contact kernel  a block per (pair, interface, tile of FDIPT_IFACE_ROWS rows).  The ligand rows pass through LDS in tiles of TILE rows
//                   (256 at <= 5 atoms per row, 64 at 37: a block's LDS stays below 64 KB); a tile without a ligand row is skipped before
//                   a coordinate is read.  A wave serves the block's receptor rows wave, wave + 4, ...: lane u holds atom u of the row in
//                   both structures (the loop over u reads it with v_readlane), lane l takes the ligand rows l, l + 64, ... of the tile.
//                   One residue pair yields its three bits together: contact of the reference, contact of the model, interface.  A
//                   receptor row's counts belong to its block (plain stores); a ligand row's are summed in LDS per tile and flushed with
//                   integer atomics.
//   rmsd kernel     a block per (pair, interface): the integers of the pair (the receptor rows' counts summed), then two superpositions
//                   as evaluate.hip forms them (centroids, covariance, fd_horn_rotation on one thread, deviations; fd_block_sum's order).
// Integers only leave the contact kernel, so no order of anything changes a bit of them; pruning skips a residue pair of a structure
// only where the triangle inequality proves that no atom pair of it can be within the cutoff.
//
// MAPPED: row j of everything is a row of the REFERENCE (N = N_b).  The prep kernel resolves each reference row ONCE - its model row
// or -1 (fd_map_row, range-checked) - and the contact and rmsd kernels read the model at the resolved rows.  A row without a model row
// takes part under FDIPT_MAP_PENALISE with the reference's own atoms and without IF_COVERED: a residue pair is tested in the model only
// where both rows carry IF_COVERED, and a reference-only row is pruned on the reference side alone.  The RMSD bits are set on covered
// rows only, so both superpositions run over covered rows in ascending reference rows.  The blocks of a pair whose map has a verdict
// (the map kernel left it behind the workspace) return as those of a pair with a bad index do.  Under FDIPT_MAP_IGNORE IF_PRESENT and
// IF_COVERED coincide, and every decision and every sum is the un-mapped instantiation's on the gathered model.
#pragma once
#include "rowmap.hpp"

#pragma clang fp contract(off)  // the distances keep the evaluation order of the contract's expressions

#include "horn.hpp"

#define IF_PRESENT (1ull << 63)  // the row takes part: res_mask of both structures (mapped, PENALISE: of the reference)
#define IF_CA_OK (1ull << 62)    // its CA exists in both structures: the row has a reach
#define IF_COVERED (1ull << 61)  // mapped entry only: the row has a model row (without it the row is evaluated in the reference alone)
#define IF_RMSD_SHIFT 40         // bits 40 .. 43: the RMSD atoms N, CA, C, O that exist in both structures
#define IF_PRUNE_MARGIN 1e-6     // relative, on the cutoff: far above the rounding of the float64 distances
// bits of a row's class in the rmsd kernel
#define IF_CLS_RECEPTOR 1
#define IF_CLS_LIGAND 2
#define IF_CLS_INTERFACE 4

static inline int if_set_atoms(int mode) { return mode == FDIPT_IFACE_CA ? 1 : mode == FDIPT_IFACE_CB ? 2 : mode == FDIPT_IFACE_BACKBONE ? 5 : 37; }
// the column of atom k of a set of K atoms in a layout of `atoms` atoms per row (K = 2: CA, CB)
__host__ __device__ __forceinline__ int if_column(int K, int atoms, int k) { return K == 1 ? (atoms == 1 ? 0 : 1) : K == 2 ? (k == 0 ? 1 : 3) : k; }
// the column of RMSD atom r (N, CA, C, O)
__device__ __forceinline__ int if_rmsd_column(int atoms, int r) { return atoms == 1 ? 0 : r == 3 ? 4 : r; }

struct IfStructure {
  const float* x;
  const unsigned char* m;
  const float* rm;
  int atoms;
};
__device__ __forceinline__ bool if_atom(const IfStructure& s, int row, int col, float (&v)[3]) {
  const long at = (long)row * s.atoms + col;
  const float* p = s.x + at * 3;
  v[0] = p[0];
  v[1] = p[1];
  v[2] = p[2];
  return s.m ? s.m[at] != 0 : (v[0] != 0.f || v[1] != 0.f || v[2] != 0.f);
}
// the workspace: the row bits [P,N] u64, the reaches [P,N,2] f64; behind them in the mapped entry the model rows [P,N_b] i32 and the verdicts [P] i32
__device__ __forceinline__ unsigned long long* if_bits(const FdiptInterfaceArgs& a) { return (unsigned long long*)a.workspace; }
__device__ __forceinline__ double* if_reach(const FdiptInterfaceArgs& a) { return (double*)a.workspace + (long)a.P * a.N; }
__device__ __forceinline__ int* ifm_rows(const FdiptInterfaceArgs& a) { return (int*)((double*)a.workspace + (long)a.P * a.N * 3); }
__device__ __forceinline__ int* ifm_verdicts(const FdiptInterfaceArgs& a) { return ifm_rows(a) + (long)a.P * a.N; }
__device__ __forceinline__ double if_sum_sq(double x, double y, double z) { return (x * x + y * y) + z * z; }
__device__ __forceinline__ float if_readlane_f(float v, int r) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), r)); }

// the pair's two structures; false where an index is out of range
__device__ __forceinline__ bool if_pair(const FdiptInterfaceArgs& a, int p, IfStructure& sa, IfStructure& sb) {
  const int ia = a.pairs[2 * p], ib = a.pairs[2 * p + 1], s_b = a.prot_b ? a.S_b : a.S;
  if (ia < 0 || ia >= a.S || ib < 0 || ib >= s_b) return false;
  const int atoms_b = a.prot_b ? a.atoms_b : a.atoms;
  sa = {a.prot + (long)ia * a.N * a.atoms * 3, a.atom_mask_a ? a.atom_mask_a + (long)ia * a.N * a.atoms : nullptr, a.res_mask + (long)ia * a.N, a.atoms};
  sb = {(a.prot_b ? a.prot_b : a.prot) + (long)ib * a.N * atoms_b * 3, a.atom_mask_b ? a.atom_mask_b + (long)ib * a.N * atoms_b : nullptr,
        (a.prot_b ? a.res_mask_b : a.res_mask) + (long)ib * a.N, atoms_b};
  return true;
}
// ... of the mapped entry (the model has m.N_a rows, the reference a.N)
__device__ __forceinline__ bool ifm_pair(const FdiptInterfaceArgs& a, const FdiptRowMap& m, int p, IfStructure& sa, IfStructure& sb) {
  const int ia = a.pairs[2 * p], ib = a.pairs[2 * p + 1];
  if (ia < 0 || ia >= a.S || ib < 0 || ib >= a.S_b) return false;
  sa = {a.prot + (long)ia * m.N_a * a.atoms * 3, a.atom_mask_a ? a.atom_mask_a + (long)ia * m.N_a * a.atoms : nullptr, a.res_mask + (long)ia * m.N_a, a.atoms};
  sb = {a.prot_b + (long)ib * a.N * a.atoms_b * 3, a.atom_mask_b ? a.atom_mask_b + (long)ib * a.N * a.atoms_b : nullptr, a.res_mask_b + (long)ib * a.N, a.atoms_b};
  return true;
}
// the pair's verdict for the blocks of the three kernels: 0 to go on, FDIPT_IFACE_SKIPPED for an index out of range, MAPPED: the map's
template <bool MAPPED>
__device__ __forceinline__ int if_open_pair(const FdiptInterfaceArgs& a, const FdiptRowMap& m, int p, IfStructure& sa, IfStructure& sb) {
  if constexpr (MAPPED) return ifm_pair(a, m, p, sa, sb) ? ifm_verdicts(a)[p] : FDIPT_IFACE_SKIPPED;
  else return if_pair(a, p, sa, sb) ? 0 : FDIPT_IFACE_SKIPPED;
}

// The least-squares superposition of the RMSD atoms of the rows whose class has a bit of `fit`, then the root mean square deviation of
// the RMSD atoms of the rows whose class has a bit of `eval` under it.  Every thread returns the same numbers; out[0 .. 8] the rotation,
// out[9 .. 11] the translation (zeros with fewer than 3 atoms), rmsd NaN with a status bit.  MAPPED: row i is a reference row and its
// model row is mrow[i] (a row with an RMSD bit is covered: mrow[i] is a row of the model).
template <bool MAPPED>
__device__ __forceinline__ void if_superpose(const IfStructure& sa, const IfStructure& sb, const unsigned long long* wb, const int* mrow, const unsigned char* cls,
                                             int N, int fit, int eval, double* red, double* rot_sh, int* flag_sh, double (&out)[12], double& rmsd, int& status) {
  const int tid = threadIdx.x;
  double cen[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // sums of the model's and the reference's atoms, their number
  for (int i = tid; i < N; i += FD_THREADS) {
    if (!(cls[i] & fit)) continue;
    for (int r = 0; r < 4; ++r) {
      if (!((wb[i] >> (IF_RMSD_SHIFT + r)) & 1ull)) continue;
      float va[3], vb[3];
      if_atom(sa, MAPPED ? mrow[i] : i, if_rmsd_column(sa.atoms, r), va);
      if_atom(sb, i, if_rmsd_column(sb.atoms, r), vb);
      cen[0] += (double)va[0]; cen[1] += (double)va[1]; cen[2] += (double)va[2];
      cen[3] += (double)vb[0]; cen[4] += (double)vb[1]; cen[5] += (double)vb[2];
      cen[6] += 1.0;
    }
  }
  fd_block_sum(cen, red);
  const double M = cen[6], inv_m = M > 0.0 ? 1.0 / M : 0.0;
  const double ca[3] = {cen[0] * inv_m, cen[1] * inv_m, cen[2] * inv_m}, cb[3] = {cen[3] * inv_m, cen[4] * inv_m, cen[5] * inv_m};
  double H[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // H = sum (a - ca)(b - cb)'
  for (int i = tid; i < N; i += FD_THREADS) {
    if (!(cls[i] & fit)) continue;
    for (int r = 0; r < 4; ++r) {
      if (!((wb[i] >> (IF_RMSD_SHIFT + r)) & 1ull)) continue;
      float va[3], vb[3];
      if_atom(sa, MAPPED ? mrow[i] : i, if_rmsd_column(sa.atoms, r), va);
      if_atom(sb, i, if_rmsd_column(sb.atoms, r), vb);
      const double px = (double)va[0] - ca[0], py = (double)va[1] - ca[1], pz = (double)va[2] - ca[2];
      const double qx = (double)vb[0] - cb[0], qy = (double)vb[1] - cb[1], qz = (double)vb[2] - cb[2];
      H[0] += px * qx; H[1] += px * qy; H[2] += px * qz;
      H[3] += py * qx; H[4] += py * qy; H[5] += py * qz;
      H[6] += pz * qx; H[7] += pz * qy; H[8] += pz * qz;
    }
  }
  fd_block_sum(H, red);
  if (tid == 0) {
    int st = 0;
    if (M < 3.0) {
      st = FDIPT_IFACE_TOO_FEW_ATOMS;
      for (int c = 0; c < 12; ++c) rot_sh[c] = 0.0;
    } else {
      double R[9], top, second, scale;
      fd_horn_rotation(H, R, top, second, scale);  // (horn.hpp)
      // the rule of evaluate.hip: the rotation is unique where the two largest eigenvalues differ by more than rounding of the matrix
      if (!(top - second > 1e-9 * scale)) st = FDIPT_IFACE_DEGENERATE;
#pragma unroll
      for (int c = 0; c < 9; ++c) rot_sh[c] = R[c];
      // t = -R ca + cb
      rot_sh[9] = -(R[0] * ca[0] + R[1] * ca[1] + R[2] * ca[2]) + cb[0];
      rot_sh[10] = -(R[3] * ca[0] + R[4] * ca[1] + R[5] * ca[2]) + cb[1];
      rot_sh[11] = -(R[6] * ca[0] + R[7] * ca[1] + R[8] * ca[2]) + cb[2];
    }
    *flag_sh = st;
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 12; ++c) out[c] = rot_sh[c];
  status = *flag_sh;
  double dev[2] = {0.0, 0.0};  // sum of the squared deviations, the number of atoms
  for (int i = tid; i < N; i += FD_THREADS) {
    if (!(cls[i] & eval)) continue;
    for (int r = 0; r < 4; ++r) {
      if (!((wb[i] >> (IF_RMSD_SHIFT + r)) & 1ull)) continue;
      float va[3], vb[3];
      if_atom(sa, MAPPED ? mrow[i] : i, if_rmsd_column(sa.atoms, r), va);
      if_atom(sb, i, if_rmsd_column(sb.atoms, r), vb);
      const double x = (double)va[0], y = (double)va[1], z = (double)va[2];
      const double dx = out[0] * x + out[1] * y + out[2] * z + out[9] - (double)vb[0];
      const double dy = out[3] * x + out[4] * y + out[5] * z + out[10] - (double)vb[1];
      const double dz = out[6] * x + out[7] * y + out[8] * z + out[11] - (double)vb[2];
      dev[0] += dx * dx + dy * dy + dz * dz;
      dev[1] += 1.0;
    }
  }
  fd_block_sum(dev, red);  // (its last barrier also orders rot_sh and flag_sh against the next call)
  rmsd = sqrt(dev[0] / dev[1]);
  if (status & FDIPT_IFACE_TOO_FEW_ATOMS) {
    rmsd = __builtin_nan("");
  } else if (!(dev[1] > 0.0)) {  // no atom to evaluate: a side without an RMSD atom
    rmsd = __builtin_nan("");
    status |= FDIPT_IFACE_TOO_FEW_ATOMS;
  } else if (!isfinite(rmsd)) {
    rmsd = __builtin_nan("");
    status |= FDIPT_IFACE_NOT_FINITE;
  }
}

// What the rmsd kernel writes for a pair that is not evaluated: the integers and fractions 0, the RMSDs and dockq NaN, the transforms 0.
__device__ __forceinline__ void if_write_skipped(const FdiptInterfaceArgs& a, long pk, int status) {
  a.n_native[pk] = a.n_model[pk] = a.n_shared[pk] = a.n_interface_rows[pk] = 0;
  a.fnat[pk] = a.fnonnat[pk] = 0.0;
  a.irmsd[pk] = a.lrmsd[pk] = a.dockq[pk] = __builtin_nan("");
  for (int c = 0; c < 9; ++c) a.interface_rotation[pk * 9 + c] = a.receptor_rotation[pk * 9 + c] = 0.0;
  for (int c = 0; c < 3; ++c) a.interface_translation[pk * 3 + c] = a.receptor_translation[pk * 3 + c] = 0.0;
  a.status[pk] = status;
}

// The outputs of one (pair, interface) from its integers (is[0 .. 2]: contacts of the reference, of the model, of both; is[3]: interface
// rows; is[4], is[5]: receptor and ligand rows that take part) and its two superpositions; one thread.
__device__ __forceinline__ void if_write_scores(const FdiptInterfaceArgs& a, long pk, const long long* is, const double (&ti)[12], const double (&tl)[12],
                                                double irmsd, double lrmsd, int st_i, int st_l) {
  int status = st_i | st_l | (is[0] == 0 ? FDIPT_IFACE_NO_NATIVE_CONTACT : 0) | (is[4] == 0 || is[5] == 0 ? FDIPT_IFACE_EMPTY_SIDE : 0);
  const double fnat = is[0] > 0 ? (double)is[2] / (double)is[0] : 0.0;
  const double fnonnat = is[1] > 0 ? (double)(is[1] - is[2]) / (double)is[1] : 0.0;
  if (is[0] == 0) irmsd = __builtin_nan("");
  const double si = irmsd / 1.5, sl = lrmsd / 8.5;
  a.n_native[pk] = (int)is[0];
  a.n_model[pk] = (int)is[1];
  a.n_shared[pk] = (int)is[2];
  a.n_interface_rows[pk] = (int)is[3];
  a.fnat[pk] = fnat;
  a.fnonnat[pk] = fnonnat;
  a.irmsd[pk] = irmsd;
  a.lrmsd[pk] = lrmsd;
  a.dockq[pk] = (fnat + 1.0 / (1.0 + si * si) + 1.0 / (1.0 + sl * sl)) / 3.0;  // (NaN where an RMSD is)
  for (int c = 0; c < 9; ++c) {
    a.interface_rotation[pk * 9 + c] = ti[c];
    a.receptor_rotation[pk * 9 + c] = tl[c];
  }
  for (int c = 0; c < 3; ++c) {
    a.interface_translation[pk * 3 + c] = ti[9 + c];
    a.receptor_translation[pk * 3 + c] = tl[9 + c];
  }
  a.status[pk] = status;
}

// The prep kernel.  MAPPED: an atom of a covered row takes part where both structures have it, of a reference-only row where the
// reference has it; the un-mapped instantiation knows every row as covered by itself (cov folds to true) and keeps IF_COVERED clear.
template <bool MAPPED>
__device__ __forceinline__ void if_prep_body(FdiptInterfaceArgs a, FdiptRowMap m, int K) {
  const int p = blockIdx.x, N = a.N, tid = threadIdx.x;
  IfStructure sa, sb;
  const bool ok = if_open_pair<MAPPED>(a, m, p, sa, sb) == 0;
  const bool penalise = MAPPED && m.coverage == FDIPT_MAP_PENALISE;
  unsigned long long* bits = if_bits(a) + (long)p * N;
  double* reach = if_reach(a) + (long)p * N * 2;
  for (int i = tid; i < N; i += FD_THREADS) {
    for (int k = 0; k < a.I; ++k) {
      const long at = ((long)p * a.I + k) * N + i;
      a.res_native[at] = a.res_model[at] = a.res_shared[at] = a.interface_rows[at] = 0;
    }
    unsigned long long b = 0ull;
    double ra = 0.0, rb = 0.0;
    int mr = MAPPED ? -1 : i;  // the row of the model
    bool present = ok && sb.rm[i] != 0.f;
    if constexpr (MAPPED) {
      if (present) mr = fd_map_row(m.map + (long)p * N, sa.rm, m.N_a, i);
    } else {
      present = present && sa.rm[i] != 0.f;
    }
    const bool cov = !MAPPED || mr >= 0;
    if (present && (cov || penalise)) {
      b = IF_PRESENT | (MAPPED && cov ? IF_COVERED : 0ull);
      float caa[3] = {0.f, 0.f, 0.f}, cab[3], va[3] = {0.f, 0.f, 0.f}, vb[3];
      bool ca_ok = if_atom(sb, i, if_column(1, sb.atoms, 0), cab);
      if (cov) ca_ok &= if_atom(sa, mr, if_column(1, sa.atoms, 0), caa);
      if (ca_ok) b |= IF_CA_OK;
      for (int k = 0; k < K; ++k) {
        bool both = if_atom(sb, i, if_column(K, sb.atoms, k), vb);
        if (cov) both &= if_atom(sa, mr, if_column(K, sa.atoms, k), va);
        if (both) b |= 1ull << k;
      }
      if (a.mode == FDIPT_IFACE_CB) b &= (b & 2ull) ? ~1ull : ~0ull;  // CB where it takes part, else CA
      for (int k = 0; k < K; ++k) {
        if (!((b >> k) & 1ull) || !ca_ok) continue;
        if_atom(sb, i, if_column(K, sb.atoms, k), vb);
        rb = fmax(rb, if_sum_sq((double)vb[0] - (double)cab[0], (double)vb[1] - (double)cab[1], (double)vb[2] - (double)cab[2]));
        if (!cov) continue;
        if_atom(sa, mr, if_column(K, sa.atoms, k), va);
        ra = fmax(ra, if_sum_sq((double)va[0] - (double)caa[0], (double)va[1] - (double)caa[1], (double)va[2] - (double)caa[2]));
      }
      if (cov) {  // (the RMSDs compare: covered rows only)
        if (a.mode != FDIPT_IFACE_CA && sa.atoms > 1 && sb.atoms > 1) {
          for (int r = 0; r < 4; ++r)
            if (if_atom(sa, mr, if_rmsd_column(sa.atoms, r), va) & if_atom(sb, i, if_rmsd_column(sb.atoms, r), vb)) b |= 1ull << (IF_RMSD_SHIFT + r);
        } else if (ca_ok) {
          b |= 1ull << (IF_RMSD_SHIFT + 1);
        }
      }
    }
    bits[i] = b;
    reach[2 * i] = sqrt(ra);
    reach[2 * i + 1] = sqrt(rb);
    if constexpr (MAPPED) ifm_rows(a)[(long)p * N + i] = (b & IF_COVERED) ? mr : -1;
  }
}

// The rmsd kernel.  MAPPED: a seventh integer, the interface rows that are covered - those that entered irmsd (n_interface_covered).
template <bool MAPPED>
__device__ __forceinline__ void if_rmsd_body(FdiptInterfaceArgs a, FdiptRowMap m) {
  constexpr int SUMS = MAPPED ? 7 : 6;
  __shared__ unsigned char cls[FDIPT_IFACE_MAX_ROWS];
  __shared__ double red[FD_WAVES * 9];
  __shared__ long long red_i[FD_WAVES * SUMS];
  __shared__ double rot_sh[12];
  __shared__ int flag_sh;
  const int tid = threadIdx.x, N = a.N, p = blockIdx.x / a.I, k = blockIdx.x % a.I;
  const long pk = (long)p * a.I + k;
  IfStructure sa, sb;
  const int verdict = if_open_pair<MAPPED>(a, m, p, sa, sb);
  if (verdict) {
    if (tid == 0) {
      if_write_skipped(a, pk, verdict);
      if constexpr (MAPPED) a.n_interface_covered[pk] = 0;
    }
    return;
  }
  const int* side = a.sides + (long)k * N;
  const unsigned long long* wb = if_bits(a) + (long)p * N;
  const int* wm = MAPPED ? ifm_rows(a) + (long)p * N : nullptr;
  // 0 .. 2: contacts of the reference, of the model, of both; 3: interface rows; 4, 5: receptor and ligand rows that take part;
  // MAPPED, 6: interface rows that are covered
  long long is[SUMS] = {};
  for (int i = tid; i < N; i += FD_THREADS) {
    const long at = pk * N + i;
    int c = 0;
    if (wb[i] & IF_PRESENT) c = side[i] == FDIPT_IFACE_RECEPTOR ? IF_CLS_RECEPTOR : side[i] == FDIPT_IFACE_LIGAND ? IF_CLS_LIGAND : 0;
    if (c && a.interface_rows[at]) c |= IF_CLS_INTERFACE;
    cls[i] = (unsigned char)c;
    if (c & IF_CLS_RECEPTOR) {
      is[0] += a.res_native[at];
      is[1] += a.res_model[at];
      is[2] += a.res_shared[at];
    }
    is[3] += (c & IF_CLS_INTERFACE) != 0;
    is[4] += (c & IF_CLS_RECEPTOR) != 0;
    is[5] += (c & IF_CLS_LIGAND) != 0;
    if constexpr (MAPPED) is[6] += (c & IF_CLS_INTERFACE) && (wb[i] & IF_COVERED);
  }
  fd_block_sum(is, red_i);  // (its barriers publish cls)
  double ti[12], tl[12], irmsd, lrmsd;
  int st_i, st_l;
  if_superpose<MAPPED>(sa, sb, wb, wm, cls, N, IF_CLS_INTERFACE, IF_CLS_INTERFACE, red, rot_sh, &flag_sh, ti, irmsd, st_i);
  if_superpose<MAPPED>(sa, sb, wb, wm, cls, N, IF_CLS_RECEPTOR, IF_CLS_LIGAND, red, rot_sh, &flag_sh, tl, lrmsd, st_l);
  if (tid != 0) return;
  if_write_scores(a, pk, is, ti, tl, irmsd, lrmsd, st_i, st_l);
  if constexpr (MAPPED) a.n_interface_covered[pk] = (int)is[6];
}

// The host-side refusals of both entries before any launch (m: the row map of the mapped entry, nullptr for the un-mapped one);
// the entry checks its own workspace size behind this.
static inline int if_check_args(const FdiptInterfaceArgs* a, const FdiptRowMap* m) {
  if (!a || a->S < 1 || a->N < 1 || a->P < 1 || a->I < 1 || a->mode < FDIPT_IFACE_CA || a->mode > FDIPT_IFACE_ALL || !(a->contact_cutoff > 0.0) ||
      !(a->interface_cutoff > 0.0) || (a->flags & ~FDIPT_IFACE_NO_PRUNE))
    return FDIPT_EINVAL;
  if (m && (!a->prot_b || m->N_a < 1 || (m->coverage != FDIPT_MAP_IGNORE && m->coverage != FDIPT_MAP_PENALISE) || !m->map || !m->n_covered ||
            !m->n_reference || !a->n_interface_covered))
    return FDIPT_EINVAL;
  if (a->prot_b && (a->S_b < 1 || !a->res_mask_b)) return FDIPT_EINVAL;
  for (int atoms : {a->atoms, a->prot_b ? a->atoms_b : a->atoms}) {
    if (atoms != 37 && atoms != 5 && atoms != 1) return FDIPT_EINVAL;
    if ((a->mode == FDIPT_IFACE_ALL && atoms != 37) || (a->mode != FDIPT_IFACE_CA && atoms == 1)) return FDIPT_EINVAL;
  }
  if (!a->prot || !a->res_mask || !a->pairs || !a->sides || !a->n_native || !a->n_model || !a->n_shared || !a->n_interface_rows || !a->res_native ||
      !a->res_model || !a->res_shared || !a->interface_rows || !a->fnat || !a->fnonnat || !a->irmsd || !a->lrmsd || !a->dockq || !a->interface_rotation ||
      !a->interface_translation || !a->receptor_rotation || !a->receptor_translation || !a->status || !a->workspace)
    return FDIPT_EINVAL;
  if (a->N > FDIPT_IFACE_MAX_ROWS || (m && m->N_a > FDIPT_IFACE_MAX_ROWS) || a->I > FDIPT_IFACE_MAX_INTERFACES) return FDIPT_ESIZE;
  if ((long)cdiv(a->N, FDIPT_IFACE_ROWS) * a->I * a->P > 0x7fffffffL) return FDIPT_ESIZE;
  return FDIPT_OK;
}
