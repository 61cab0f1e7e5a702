// violations.hip — structural violations of samples on the device (include/fdipt.h, "structural violations"): the bond, angle, clash and
// within-residue terms of openfold/utils/loss.py find_structural_violations (:1105) and compute_violation_metrics (:1272) as
// framedipt/analysis/metrics.py:protein_metrics calls them (every residue ALA, tolerance factor 12, overlap tolerance 1.5), and the
// radius of gyration, for B samples, all in float64.
//
// Two launches on one stream, nothing between them on the host:
//   pair kernel    a block serves FD_WAVES rows of one sample, a wave per row i.  The existing rows j of the sample pass through LDS in
//                  tiles of VI_TILE; lane l takes j = l, l + 64, ... ascending, in BOTH directions (index[i] < index[j]: the pair (i, j),
//                  index[j] < index[i]: the pair (j, i)), so every per-atom sum of row i is formed by this wave alone: each lane's terms
//                  in ascending j, then a butterfly.  The wave writes row i's per-atom sums and flags, and to the workspace its sum of the
//                  errors of the pairs (i, j) and their number (an integer).
//   reduce kernel  a block per sample: row i to thread i % 256, a thread's rows ascending, butterfly inside a wave, the waves in index
//                  order.  Forms the O(N) terms (bonds, angles, CA-CA, within-residue, radius of gyration) and the scalars.
// A row that does not exist is skipped; no floating-point atomics: rows appended behind a sample and its batch mates change no bit.
#include "common.hpp"

#define VI_TILE FD_THREADS

// openfold/np/residue_constants.py.  van_der_waals_radius by element, in the atom order N, CA, C, CB, O
#define VI_R_C 1.7
#define VI_R_N 1.55
#define VI_R_O 1.52
#define VI_OVERLAP 1.5  // clash_overlap_tolerance
// between_res_bond_length_c_n[0], between_res_bond_length_stddev_c_n[0]: the reference forms them, and 12 x the stddev, as float32
// tensors (a bool tensor times a Python float) whatever the precision of the coordinates
#define VI_CN_LEN ((double)1.329f)
#define VI_CN_STD ((double)0.014f)
#define VI_CN_TOL ((double)(12.0f * 0.014f))
// between_res_cos_angles_ca_c_n[0] with between_res_bond_length_stddev_c_n[0] as its stddev (a bond-length stddev for an angle, as
// between_residue_bond_loss :807 has it), between_res_cos_angles_c_n_ca; these stay Python floats
#define VI_COS_CA_C_N (-0.4473)
#define VI_STD_CA_C_N 0.014
#define VI_COS_C_N_CA (-0.5203)
#define VI_STD_C_N_CA 0.0353
#define VI_TOL 12.0           // violation_tolerance_factor
#define VI_CA_CA 3.80209737096  // ca_ca
#define VI_CA_FAR 1.5           // extreme_ca_ca_distance_violations: max_angstrom_tolerance
// make_atom14_dists_bounds(1.5, 12) of ALA, a float32 table, rows and columns in the order N, CA, C, CB, O
#define VI_LOWER_TABLE                                                    \
  {{0.0f, 1.21899998f, 1.88165307f, 2.06256866f, 1.57000005f},           \
   {1.21899998f, 0.0f, 1.21300006f, 1.26800001f, 1.9400022f},            \
   {1.88165307f, 1.21300006f, 0.0f, 2.06785154f, 1.00100005f},           \
   {2.06256866f, 1.26800001f, 2.06785154f, 0.0f, 1.72000003f},           \
   {1.57000005f, 1.9400022f, 1.00100005f, 1.72000003f, 0.0f}}
#define VI_UPPER_TABLE                                                    \
  {{0.0f, 1.699f, 3.03730035f, 2.82141972f, 1e+10f},                     \
   {1.699f, 0.0f, 1.83700001f, 1.77199996f, 2.84160995f},                \
   {3.03730035f, 1.83700001f, 0.0f, 2.92383409f, 1.45700002f},           \
   {2.82141972f, 1.77199996f, 2.92383409f, 0.0f, 1e+10f},                \
   {1e+10f, 2.84160995f, 1.45700002f, 1e+10f, 0.0f}}
__device__ __constant__ float vi_lower[5][5] = VI_LOWER_TABLE;
__device__ __constant__ float vi_upper[5][5] = VI_UPPER_TABLE;
static const float vi_lower_host[5][5] = VI_LOWER_TABLE;  // (what fdipt_violation_constants reports)
static const float vi_upper_host[5][5] = VI_UPPER_TABLE;

__device__ __forceinline__ double vi_radius(int a) { return a == 0 ? VI_R_N : a == 4 ? VI_R_O : VI_R_C; }
// the reference's atom14 order of the five atoms (N, CA, C, O, CB) in atom37 columns: the order its within-residue sums run in
__device__ __forceinline__ int vi_atom14(int k) { return k == 3 ? 4 : k == 4 ? 3 : k; }


// the five atoms of row j of sample b (15 doubles), zero where the row does not keep its coordinates
__device__ __forceinline__ void vi_load_row(const FdiptViolationArgs& a, long row, double (&x)[15]) {
  const bool keep = a.keep_mask[row] != 0.f;
  const float* p = a.prot + row * (long)a.atoms * 3;
#pragma unroll
  for (int k = 0; k < 15; ++k) x[k] = keep ? (double)p[k] : 0.0;
}
__device__ __forceinline__ double vi_dist2(const double* p, const double* q) {
  const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
  return dx * dx + dy * dy + dz * dz;
}

__global__ __launch_bounds__(FD_THREADS) void violations_pair_kernel(FdiptViolationArgs a, int tiles) {
  __shared__ float xs[15][VI_TILE];
  __shared__ int idx_sh[VI_TILE];
  __shared__ int exists_sh[VI_TILE];
  const int tid = threadIdx.x, lane = tid & (FD_WAVE - 1), wave = tid / FD_WAVE, N = a.N;
  const int b = blockIdx.x / tiles, i = (blockIdx.x % tiles) * FD_WAVES + wave;
  const long row0 = (long)b * N;
  const bool mine = i < N && a.res_mask[row0 + (i < N ? i : 0)] != 0.f;  // (the same in every lane of a wave)
  double xi[15];
  long idx_i = 0;
#pragma unroll
  for (int k = 0; k < 15; ++k) xi[k] = 0.0;
  if (mine) {
    vi_load_row(a, row0 + i, xi);
    idx_i = a.residue_index[row0 + i];
  }
  double loss[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, err = 0.0;
  unsigned flags = 0u;
  long long pairs = 0;
  for (int j0 = 0; j0 < N; j0 += VI_TILE) {
    __syncthreads();
    {
      const int j = j0 + tid;
      const bool ex = j < N && a.res_mask[row0 + (j < N ? j : 0)] != 0.f;
      exists_sh[tid] = ex;
      if (ex) {
        const bool keep = a.keep_mask[row0 + j] != 0.f;
        const float* p = a.prot + (row0 + j) * (long)a.atoms * 3;
#pragma unroll
        for (int k = 0; k < 15; ++k) xs[k][tid] = keep ? p[k] : 0.f;
        idx_sh[tid] = a.residue_index[row0 + j];
      }
    }
    __syncthreads();
    if (!mine) continue;
    for (int jl = lane; jl < VI_TILE; jl += FD_WAVE) {
      if (!exists_sh[jl]) continue;
      const long idx_j = idx_sh[jl];
      if (idx_j == idx_i) continue;  // (row i itself among them)
      const bool up = idx_i < idx_j;  // the pair (i, j); otherwise the pair (j, i)
      // the peptide bond C - N of neighbouring indices is no clash: C of the lower index, N of the higher
      const bool bonded = up ? idx_i + 1 == idx_j : idx_j + 1 == idx_i;
      double xj[15];
#pragma unroll
      for (int k = 0; k < 15; ++k) xj[k] = (double)xs[k][jl];
      double pair_err = 0.0;
#pragma unroll
      for (int p = 0; p < 5; ++p) {
#pragma unroll
        for (int q = 0; q < 5; ++q) {
          if (bonded && (up ? (p == 2 && q == 0) : (p == 0 && q == 2))) continue;
          const double d2 = vi_dist2(xi + 3 * p, xj + 3 * q);
          // the largest bound is 1.7 + 1.7 - 1.5 = 1.9: beyond a distance of 2 the error is exactly 0 and there is no clash
          if (d2 < 4.0) {
            const double d = sqrt(1e-10 + d2), bound = (vi_radius(p) + vi_radius(q)) - VI_OVERLAP;
            const double e = fmax(bound - d, 0.0);
            loss[p] += e;
            pair_err += e;
            flags |= (d < bound ? 1u : 0u) << p;
          }
        }
      }
      if (up) {
        err += pair_err;
        pairs += bonded ? 24 : 25;
      }
    }
  }
  if (i >= N) return;
#pragma unroll
  for (int p = 0; p < 5; ++p) loss[p] = wave_sum_d(loss[p]);
  err = wave_sum_d(err);
  pairs = wave_sum_ll(pairs);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) flags |= __shfl_xor(flags, o, 64);
  if (lane == 0) {
    double* pair_err_ws = (double*)a.workspace;
    long long* pair_cnt_ws = (long long*)(pair_err_ws + (long)a.B * N);
#pragma unroll
    for (int p = 0; p < 5; ++p) {
      a.clashes_per_atom_loss_sum[(row0 + i) * 5 + p] = loss[p];
      a.clashes_per_atom_clash_mask[(row0 + i) * 5 + p] = (flags >> p) & 1u;
    }
    pair_err_ws[row0 + i] = err;
    pair_cnt_ws[row0 + i] = pairs;
  }
}

// the terms of the peptide bond from row `x` (this) to row `y` (next) of between_residue_bond_loss (:712) and of
// extreme_ca_ca_distance_violations (:1235): the sum of the three flat-bottom errors, each of them, the violation flags
struct ViBond {
  double c_n, ca_c_n, c_n_ca, sum;
  bool violated, ca_far;
};
__device__ __forceinline__ ViBond vi_bond(const double (&x)[15], const double (&y)[15]) {
  const double *ca = x + 3, *c = x + 6, *n = y, *ca2 = y + 3;
  const double c_n_len = sqrt(1e-6 + vi_dist2(c, n)), ca_c_len = sqrt(1e-6 + vi_dist2(ca, c)), n_ca_len = sqrt(1e-6 + vi_dist2(n, ca2));
  const double len_err = sqrt(1e-6 + (c_n_len - VI_CN_LEN) * (c_n_len - VI_CN_LEN));
  double cos1 = 0.0, cos2 = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double c_ca = (ca[k] - c[k]) / ca_c_len, c_n = (n[k] - c[k]) / c_n_len, n_ca = (ca2[k] - n[k]) / n_ca_len;
    cos1 += c_ca * c_n;
    cos2 += (-c_n) * n_ca;
  }
  const double err1 = sqrt(1e-6 + (cos1 - VI_COS_CA_C_N) * (cos1 - VI_COS_CA_C_N));
  const double err2 = sqrt(1e-6 + (cos2 - VI_COS_C_N_CA) * (cos2 - VI_COS_C_N_CA));
  const double tol1 = VI_TOL * VI_STD_CA_C_N, tol2 = VI_TOL * VI_STD_C_N_CA;
  ViBond r;
  r.c_n = fmax(len_err - VI_CN_TOL, 0.0);
  r.ca_c_n = fmax(err1 - tol1, 0.0);
  r.c_n_ca = fmax(err2 - tol2, 0.0);
  r.sum = r.c_n + r.ca_c_n + r.c_n_ca;
  r.violated = len_err > VI_CN_TOL || err1 > tol1 || err2 > tol2;
  r.ca_far = sqrt(1e-6 + vi_dist2(ca, ca2)) - VI_CA_CA > VI_CA_FAR;
  return r;
}

__global__ __launch_bounds__(FD_THREADS) void violations_reduce_kernel(FdiptViolationArgs a) {
  __shared__ double red_d[FD_WAVES * 8];
  __shared__ long long red_i[FD_WAVES * 8];
  const int tid = threadIdx.x, N = a.N, b = blockIdx.x;
  const long row0 = (long)b * N;
  const float* rm = a.res_mask + row0;
  const int* index = a.residue_index + row0;
  const double* pair_err_ws = (const double*)a.workspace;
  const long long* pair_cnt_ws = (const long long*)(pair_err_ws + (long)a.B * N);
  // 0..2: the masked bond and angle errors, 3: the clash errors, 4..6: the coordinates of the kept rows' atoms, 7: their number
  double fs[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  // 0: bonds without a gap, 1: far CA among them, 2: rows, 3..6: rows with a bond / clash / within-residue / any violation, 7: clash pairs
  long long is[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = tid; i < N; i += FD_THREADS) {
    double conn = 0.0;
    unsigned char conn_mask = 0, total = 0;
    if (rm[i] != 0.f) {
      double x[15], y[15];
      vi_load_row(a, row0 + i, x);
      int prev = i - 1, next = i + 1;  // the existing neighbours
      while (prev >= 0 && rm[prev] == 0.f) --prev;
      while (next < N && rm[next] == 0.f) ++next;
      double from_next = 0.0, from_prev = 0.0;
      if (next < N) {
        vi_load_row(a, row0 + next, y);
        const ViBond t = vi_bond(x, y);
        from_next = t.sum;
        if ((long)index[next] - (long)index[i] == 1) {
          fs[0] += t.c_n;
          fs[1] += t.ca_c_n;
          fs[2] += t.c_n_ca;
          is[0] += 1;
          is[1] += t.ca_far;
          conn_mask |= t.violated;
        }
      }
      if (prev >= 0) {
        vi_load_row(a, row0 + prev, y);
        const ViBond t = vi_bond(y, x);
        from_prev = t.sum;
        if ((long)index[i] - (long)index[prev] == 1) conn_mask |= t.violated;
      }
      conn = 0.5 * (from_next + from_prev);
      // within_residue_violations (:1018)
      unsigned char within_any = 0, clash_any = 0;
#pragma unroll
      for (int p = 0; p < 5; ++p) {
        double along = 0.0, across = 0.0;
        bool bad = false;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          const int q = vi_atom14(k);
          if (q == p) continue;
          const double d = sqrt(1e-10 + vi_dist2(x + 3 * p, x + 3 * q)), lo = (double)vi_lower[p][q], hi = (double)vi_upper[p][q];
          const double e = fmax(lo - d, 0.0) + fmax(d - hi, 0.0);
          along += e;
          across += e;
          bad |= d < lo || d > hi;
        }
        a.within_per_atom_loss_sum[(row0 + i) * 5 + p] = along + across;
        a.within_per_atom_violations[(row0 + i) * 5 + p] = bad;
        within_any |= bad;
        clash_any |= a.clashes_per_atom_clash_mask[(row0 + i) * 5 + p];
      }
      total = conn_mask | clash_any | within_any;
      fs[3] += pair_err_ws[row0 + i];
      is[2] += 1;
      is[3] += conn_mask;
      is[4] += clash_any;
      is[5] += within_any;
      is[6] += total;
      is[7] += pair_cnt_ws[row0 + i];
      if (a.keep_mask[row0 + i] != 0.f) {
#pragma unroll
        for (int p = 0; p < 5; ++p) {
          fs[4] += x[3 * p];
          fs[5] += x[3 * p + 1];
          fs[6] += x[3 * p + 2];
        }
        fs[7] += 5.0;
      }
    } else {
#pragma unroll
      for (int p = 0; p < 5; ++p) {
        a.within_per_atom_loss_sum[(row0 + i) * 5 + p] = 0.0;
        a.within_per_atom_violations[(row0 + i) * 5 + p] = 0;
      }
    }
    a.connections_per_residue_loss_sum[row0 + i] = conn;
    a.connections_per_residue_violation_mask[row0 + i] = conn_mask;
    a.total_per_residue_violations_mask[row0 + i] = total;
  }
  fd_block_sum(fs, red_d);
  fd_block_sum(is, red_i);
  // radius of gyration: the deviations from the centroid, in the same order
  const double atoms = fs[7];
  const double cx = fs[4] / atoms, cy = fs[5] / atoms, cz = fs[6] / atoms;
  double dev[1] = {0.0};
  for (int i = tid; i < N; i += FD_THREADS) {
    if (rm[i] != 0.f && a.keep_mask[row0 + i] != 0.f) {
      const float* p = a.prot + (row0 + i) * (long)a.atoms * 3;
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const double dx = (double)p[3 * k] - cx, dy = (double)p[3 * k + 1] - cy, dz = (double)p[3 * k + 2] - cz;
        dev[0] += dx * dx + dy * dy + dz * dz;
      }
    }
  }
  fd_block_sum(dev, red_d);
  if (tid == 0) {
    const double bonds = (double)is[0], rows = (double)is[2];
    a.bonds_c_n_loss_mean[b] = fs[0] / (bonds + 1e-6);
    a.angles_ca_c_n_loss_mean[b] = fs[1] / (bonds + 1e-6);
    a.angles_c_n_ca_loss_mean[b] = fs[2] / (bonds + 1e-6);
    a.clashes_mean_loss[b] = fs[3] / (1e-6 + (double)is[7]);
    a.violations_extreme_ca_ca_distance[b] = (double)is[1] / (1e-4 + bonds);  // (masked_mean's own eps)
    a.violations_between_residue_bond[b] = (double)is[3] / (1e-4 + rows);
    a.violations_between_residue_clash[b] = (double)is[4] / (1e-4 + rows);
    a.violations_within_residue[b] = (double)is[5] / (1e-4 + rows);
    a.violations_per_residue[b] = (double)is[6] / (1e-4 + rows);
    a.radius_of_gyration[b] = sqrt(dev[0] / atoms);  // (no kept row: 0 / 0 = NaN)
    a.num_residue_violations[b] = (int)is[6];
    a.n_clash_pairs[b] = is[7];
  }
}

extern "C" int fdipt_violation_constants(double* out) {
  if (!out) return FDIPT_EINVAL;
  const double head[11] = {VI_R_C, VI_R_N, VI_R_O, VI_CN_LEN, VI_CN_STD, VI_CN_TOL, VI_COS_CA_C_N, VI_STD_CA_C_N, VI_COS_C_N_CA, VI_STD_C_N_CA, VI_CA_CA};
  for (int k = 0; k < 11; ++k) out[k] = head[k];
  for (int k = 0; k < 25; ++k) {
    out[11 + k] = (double)vi_lower_host[k / 5][k % 5];
    out[36 + k] = (double)vi_upper_host[k / 5][k % 5];
  }
  return FDIPT_VIOLATION_CONSTANTS;
}

extern "C" size_t fdipt_sample_violations_workspace(int B, int N) {
  if (B < 1 || N < 1) return 0;
  return (size_t)B * N * (sizeof(double) + sizeof(long long));
}

extern "C" int fdipt_sample_violations(const FdiptViolationArgs* a, fdipt_stream_t stream) {
  if (!a || a->B < 1 || a->N < 1 || (a->atoms != 37 && a->atoms != 5)) return FDIPT_EINVAL;
  if (!a->prot || !a->res_mask || !a->keep_mask || !a->residue_index || !a->bonds_c_n_loss_mean || !a->angles_ca_c_n_loss_mean ||
      !a->angles_c_n_ca_loss_mean || !a->clashes_mean_loss || !a->violations_extreme_ca_ca_distance || !a->violations_between_residue_bond ||
      !a->violations_between_residue_clash || !a->violations_within_residue || !a->violations_per_residue || !a->radius_of_gyration ||
      !a->num_residue_violations || !a->n_clash_pairs || !a->connections_per_residue_loss_sum || !a->connections_per_residue_violation_mask ||
      !a->total_per_residue_violations_mask || !a->clashes_per_atom_loss_sum || !a->clashes_per_atom_clash_mask ||
      !a->within_per_atom_loss_sum || !a->within_per_atom_violations || !a->workspace)
    return FDIPT_EINVAL;
  const long tiles = cdiv(a->N, FD_WAVES);
  if (tiles * a->B > 0x7fffffffL) return FDIPT_ESIZE;
  if (a->workspace_bytes < fdipt_sample_violations_workspace(a->B, a->N)) return FDIPT_ESIZE;
  hipLaunchKernelGGL(violations_pair_kernel, dim3((unsigned)(tiles * a->B)), dim3(FD_THREADS), 0, (hipStream_t)stream, *a, (int)tiles);
  FD_CHECK_LAUNCH();
  hipLaunchKernelGGL(violations_reduce_kernel, dim3(a->B), dim3(FD_THREADS), 0, (hipStream_t)stream, *a);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
