// interface_common.hpp — what interface.hip and interface_mapped.hip share (include/fdipt.h, "interface accuracy"; DESIGN.md sections 7.18
// and 7.19): the bits of a row in the workspace, the readers of a structure, the layout of the atom sets and the superposition of the
// rmsd kernels.  The contact kernels stand beside each other in the two units: the mapped one reads the model through the row's resolution.
#pragma once
#include "common.hpp"

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
// the index of CA inside the set
__host__ __device__ __forceinline__ int if_ca_index(int K) { return K <= 2 ? 0 : 1; }
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
__device__ __forceinline__ unsigned long long* if_bits(const FdiptInterfaceArgs& a) { return (unsigned long long*)a.workspace; }
__device__ __forceinline__ double* if_reach(const FdiptInterfaceArgs& a) { return (double*)a.workspace + (long)a.P * a.N; }
__device__ __forceinline__ double if_sum_sq(double x, double y, double z) { return (x * x + y * y) + z * z; }
__device__ __forceinline__ float if_readlane_f(float v, int r) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), r)); }

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
