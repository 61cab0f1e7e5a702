// sasa.hip — solvent accessibility of samples on the device (include/fdipt.h, "solvent accessibility"): Shrake &
// Rupley's accessible surface per atom and residue and the relative value, the numbers the reference takes from
// Bio.PDB.SASA.ShrakeRupley().compute(model, level="R") (evaluation/utils/metrics.py:get_sasa), for B samples, all in float64.
//
// Three launches on one stream, no host synchronisation:
//   (a) a block per sample compacts the atoms that exist in (row, column) order into the workspace (ballot + popcount per wave, the
//       four waves' counts through LDS): x, y, z, R, R^2 as float64 in separate arrays, the origin index, the count per sample; the
//       outputs of the atoms that do not exist are zeroed here
//   (b) a wave per compacted atom i (waves past the sample's count exit at once).  Lane l owns points l, l + 64, ... (SLOTS per lane)
//       and keeps their "still accessible" flags in a register mask.  The wave walks the sample's atom list in tiles of 64: lane l
//       tests atom j0 + l with the neighbour filter, the ballot names the tile's neighbours, and for each set bit c_j and R_j^2 are
//       broadcast from the owning lane and every lane tests the points it still holds.  The walk ends when no flag is left.  No lists,
//       no capacities, no atomics, no order that depends on timing; the atom list is read from L2, there is no LDS and no barrier.
//   (c) a thread per row: residue_sasa sequentially in column order, rsa
// Contraction into fused multiply-adds is off in this unit: the distances are compared bit for bit with a NumPy evaluation.
#include "common.hpp"

#pragma clang fp contract(off)

#define SA_FOUR_PI 12.566370614359172  // 4 pi: 4.0 * 3.141592653589793, exact in float64
// The neighbour filter keeps j where |c_i - c_j|^2 <= (R_i + R_j)^2 SA_CULL.  A point of atom i lies R_i (1 +- 1e-7) from c_i (the
// sphere table is unit to float32 rounding) and is buried by j only within R_j of c_j, so a buried point implies |c_i - c_j| <=
// (R_i + R_j) (1 + 1e-7): the factor covers that and every float64 rounding of the filter itself with four orders to spare.
#define SA_CULL 1.00001

// the workspace: the counts of the B samples, then per sample five double arrays and one int array of M = N atoms entries
struct SaWs {
  double *x, *y, *z, *r, *r2;  // [M] each: the compacted atoms
  int* origin;                 // [M]: row * atoms + column
};
__host__ __device__ inline size_t sa_header(size_t B) { return (B * 4 + 7) / 8 * 8; }
__host__ __device__ inline size_t sa_stride(size_t M) { return (M * 44 + 7) / 8 * 8; }
__device__ __forceinline__ int* sa_counts(void* base) { return (int*)base; }
__device__ __forceinline__ SaWs sa_ws(void* base, int B, int b, size_t M) {
  SaWs w;
  w.x = (double*)((char*)base + sa_header((size_t)B) + (size_t)b * sa_stride(M));
  w.y = w.x + M;
  w.z = w.y + M;
  w.r = w.z + M;
  w.r2 = w.r + M;
  w.origin = (int*)(w.r2 + M);
  return w;
}

__global__ __launch_bounds__(FD_THREADS) void sasa_compact_kernel(FdiptSasaArgs a) {
  __shared__ int cnt_sh[FD_WAVES];
  const int tid = threadIdx.x, lane = tid & (FD_WAVE - 1), wave = tid / FD_WAVE, b = blockIdx.x;
  const long M = (long)a.N * a.atoms, e_base = (long)b * M;
  const SaWs w = sa_ws(a.workspace, a.B, b, (size_t)M);
  int base = 0;
  for (long e0 = 0; e0 < M; e0 += FD_THREADS) {
    const long e = e0 + tid;
    bool f = false;
    if (e < M) {
      f = a.res_mask[(long)b * a.N + e / a.atoms] != 0.f && a.atom_mask[e_base + e] != 0;
      if (!f) a.accessible[e_base + e] = 0, a.atom_sasa[e_base + e] = 0.0;
    }
    const unsigned long long mask = __ballot(f);
    if (lane == 0) cnt_sh[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int v = 0; v < FD_WAVES; ++v) {
      const int c = cnt_sh[v];
      before += v < wave ? c : 0;
      total += c;
    }
    if (f) {  // (k < M: no more atoms are kept than were looked at)
      const long k = base + before + __popcll(mask & ((1ull << lane) - 1ull));
      const float* p = a.prot + (e_base + e) * 3;
      const double r = a.atom_radius[e % a.atoms];
      w.x[k] = (double)p[0], w.y[k] = (double)p[1], w.z[k] = (double)p[2];
      w.r[k] = r, w.r2[k] = r * r;
      w.origin[k] = (int)e;
    }
    base += total;
    __syncthreads();
  }
  if (tid == 0) sa_counts(a.workspace)[b] = base, a.n_atoms[b] = base;
}

template <int SLOTS>
__global__ __launch_bounds__(FD_THREADS) void sasa_points_kernel(FdiptSasaArgs a) {
  const int lane = threadIdx.x & (FD_WAVE - 1), b = blockIdx.y;
  const int n = sa_counts(a.workspace)[b];
  const long i = (long)blockIdx.x * FD_WAVES + threadIdx.x / FD_WAVE;
  if (i >= n) return;  // (whole waves leave; the kernel has no barrier)
  const long M = (long)a.N * a.atoms;
  const SaWs w = sa_ws(a.workspace, a.B, b, (size_t)M);
  const double xi = w.x[i], yi = w.y[i], zi = w.z[i], ri = w.r[i];
  double px[SLOTS], py[SLOTS], pz[SLOTS];
  unsigned flags = 0;
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int k = lane + FD_WAVE * s;
    px[s] = py[s] = pz[s] = 0.0;
    if (k < a.n_points) {
      px[s] = a.sphere[3 * k] * ri + xi;
      py[s] = a.sphere[3 * k + 1] * ri + yi;
      pz[s] = a.sphere[3 * k + 2] * ri + zi;
      flags |= 1u << s;
    }
  }
  for (int j0 = 0; j0 < n; j0 += FD_WAVE) {
    const int j = j0 + lane;
    double xj = 0.0, yj = 0.0, zj = 0.0, r2j = 0.0;
    bool near = false;
    if (j < n) {
      xj = w.x[j], yj = w.y[j], zj = w.z[j], r2j = w.r2[j];
      const double dx = xi - xj, dy = yi - yj, dz = zi - zj, reach = ri + w.r[j];
      near = j != i && (dx * dx + dy * dy) + dz * dz <= (reach * reach) * SA_CULL;
    }
    unsigned long long nbrs = __ballot(near);
    while (nbrs) {
      const int l = __ffsll((long long)nbrs) - 1;
      nbrs &= nbrs - 1;
      const double cx = fd_readlane_d(xj, l), cy = fd_readlane_d(yj, l), cz = fd_readlane_d(zj, l), c2 = fd_readlane_d(r2j, l);
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        const double dx = px[s] - cx, dy = py[s] - cy, dz = pz[s] - cz;
        if ((dx * dx + dy * dy) + dz * dz <= c2) flags &= ~(1u << s);
      }
    }
    if (__ballot(flags != 0) == 0) break;
  }
  int count = 0;
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) count += __popcll(__ballot((flags >> s) & 1u));
  if (lane == 0) {
    const long e = (long)b * M + w.origin[i];
    a.accessible[e] = count;
    a.atom_sasa[e] = (double)count * (w.r2[i] * (SA_FOUR_PI / (double)a.n_points));
  }
}

__global__ __launch_bounds__(FD_THREADS) void sasa_rows_kernel(FdiptSasaArgs a) {
  const long row = (long)blockIdx.x * FD_THREADS + threadIdx.x;
  if (row >= (long)a.B * a.N) return;
  const double* v = a.atom_sasa + row * a.atoms;
  double sum = 0.0;
  for (int c = 0; c < a.atoms; ++c) sum += v[c];
  a.residue_sasa[row] = sum;
  a.rsa[row] = sum / a.max_sasa[row];
}

extern "C" size_t fdipt_sample_sasa_workspace(int B, int N, int atoms) {
  if (B < 1 || N < 1 || (atoms != 37 && atoms != 5)) return 0;
  return sa_header((size_t)B) + (size_t)B * sa_stride((size_t)N * (size_t)atoms);
}

extern "C" int fdipt_sample_sasa(const FdiptSasaArgs* a, fdipt_stream_t stream) {
  if (!a || a->B < 1 || a->N < 1 || (a->atoms != 37 && a->atoms != 5) || a->n_points < 1 || a->n_points > 1024) return FDIPT_EINVAL;
  if (!a->prot || !a->res_mask || !a->atom_mask || !a->atom_radius || !a->sphere || !a->max_sasa || !a->accessible || !a->atom_sasa ||
      !a->residue_sasa || !a->rsa || !a->n_atoms || !a->workspace)
    return FDIPT_EINVAL;
  const long M = (long)a->N * a->atoms;
  if (a->B > 65535 || (long)a->B * M > 0x7fffffffL) return FDIPT_ESIZE;  // (grid.y; the origin index and the row grid are ints)
  if (a->workspace_bytes < fdipt_sample_sasa_workspace(a->B, a->N, a->atoms)) return FDIPT_ESIZE;
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sasa_compact_kernel, dim3((unsigned)a->B), dim3(FD_THREADS), 0, s, *a);
  FD_CHECK_LAUNCH();
  const dim3 grid((unsigned)cdiv(M, FD_WAVES), (unsigned)a->B);
  if (a->n_points <= 2 * FD_WAVE)
    hipLaunchKernelGGL(sasa_points_kernel<2>, grid, dim3(FD_THREADS), 0, s, *a);
  else
    hipLaunchKernelGGL(sasa_points_kernel<16>, grid, dim3(FD_THREADS), 0, s, *a);
  FD_CHECK_LAUNCH();
  hipLaunchKernelGGL(sasa_rows_kernel, dim3((unsigned)cdiv((long)a->B * a->N, FD_THREADS)), dim3(FD_THREADS), 0, s, *a);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
