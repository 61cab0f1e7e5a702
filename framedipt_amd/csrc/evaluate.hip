// evaluate.hip — sample evaluation on the device (include/fdipt.h, "sample evaluation"): backbone RMSD of the diffused regions, the
// dihedrals phi / psi / omega with their signed errors, the CA geometry checks and the superposed CA deviation of
// evaluation/utils/metrics.py and framedipt/analysis/metrics.py, for B samples against R ground-truth structures in one launch, all
// in float64.
//
// Blocks 0 .. B - 1 serve a sample each, blocks B .. B + R - 1 write the dihedrals of a ground-truth row (with the chains of the first
// sample that names it).  Phases of a sample's block (a __syncthreads between them, nothing leaves the launch):
//   0  the region table against the masks: every region a maximal run of diffused rows of one chain, all diffused rows covered (all waves)
//   1  per-residue backbone deviation; a wave per region sums its rows; thread 0 adds the regions in table order
//   2  dihedrals of sample and ground truth and their signed errors, a thread per residue
//   3  ordered compaction of the CA atoms of the non-zero rows into the workspace; bonds (strided sums) and the pair loop (integer counts)
//   4  superposition: centroids and the 3 x 3 covariance (strided sums), Horn's 4 x 4 eigenproblem by Jacobi sweeps (thread 0, in
//      registers), then the two deviations under the rotation (strided sums)
// Every floating-point sum is "row i to thread i % 256, the thread's rows in ascending order, then a fixed tree over the block": a row
// that is masked out adds nothing, so neither rows appended behind a sample nor its batch mates change a bit of its outputs.
#include "common.hpp"
#include "horn.hpp"

#define EV_CA_CA 3.80209737096  // residue_constants.ca_ca
#define EV_RAD2DEG 57.29577951308232

struct EvVec { double x, y, z; };
__device__ __forceinline__ EvVec ev_load(const float* p) { return {(double)p[0], (double)p[1], (double)p[2]}; }
__device__ __forceinline__ EvVec ev_sub(EvVec a, EvVec b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double ev_dot(EvVec a, EvVec b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// metrics.py:880-923 in degrees (atan2 of the rejections of b0 and b2 from the normalised b1); NaN where two atoms coincide
__device__ __forceinline__ double ev_dihedral(EvVec a, EvVec b, EvVec c, EvVec d) {
  const EvVec b0 = ev_sub(a, b), b2 = ev_sub(d, c);
  EvVec b1 = ev_sub(c, b);
  const double n1 = sqrt(ev_dot(b1, b1));
  b1 = {b1.x / n1, b1.y / n1, b1.z / n1};
  const double d1 = ev_dot(b0, b1), d2 = ev_dot(b2, b1);
  const EvVec v = {b0.x - d1 * b1.x, b0.y - d1 * b1.y, b0.z - d1 * b1.z}, w = {b2.x - d2 * b1.x, b2.y - d2 * b1.y, b2.z - d2 * b1.z};
  const EvVec cr = {b1.y * v.z - b1.z * v.y, b1.z * v.x - b1.x * v.z, b1.x * v.y - b1.y * v.x};
  return atan2(ev_dot(cr, w), ev_dot(v, w)) * EV_RAD2DEG;
}
// phi, psi, omega of row i of the structure x [N,37,3] (calc_dihedrals :926-956; atom37 columns N = 0, CA = 1, C = 2); prev / next: row
// i - 1 / i + 1 belongs to the same chain
__device__ __forceinline__ void ev_row_dihedrals(const float* x, long i, bool prev, bool next, double (&out)[3]) {
  const float* r = x + i * 111;
  const EvVec n = ev_load(r), ca = ev_load(r + 3), c = ev_load(r + 6);
  out[0] = out[1] = out[2] = 0.0;
  if (prev) out[0] = ev_dihedral(ev_load(r - 111 + 6), n, ca, c);
  if (next) {
    const EvVec n1 = ev_load(r + 111), ca1 = ev_load(r + 111 + 3);
    out[1] = ev_dihedral(n, ca, c, n1);
    out[2] = ev_dihedral(ca, c, n1, ca1);
  }
}
// angle_error_with_sign (:308-331): the candidate of smallest absolute value among d, d + 360, d - 360, the lowest index on equality
__device__ __forceinline__ double ev_signed_error(double a, double b) {
  const double c0 = a - b, c1 = a + 360.0 - b, c2 = a - 360.0 - b;
  double best = c0;
  if (fabs(c1) < fabs(best)) best = c1;
  if (fabs(c2) < fabs(best)) best = c2;
  return best;
}
// sum over the four backbone atoms of |x - y|^2 at one row
__device__ __forceinline__ double ev_row_delta2(const float* x, const float* y) {
  double acc = 0.0;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const EvVec d = ev_sub(ev_load(x + fd_backbone_off(a)), ev_load(y + fd_backbone_off(a)));
    acc += ev_dot(d, d);
  }
  return acc;
}

// ground-truth dihedrals of row r, with the chains and the res_mask of the first sample that names it
__device__ void ev_reference_block(const FdiptEvalArgs& a, int r) {
  __shared__ int owner_sh;
  const int tid = threadIdx.x, N = a.N;
  if (tid == 0) owner_sh = a.B;
  __syncthreads();
  for (int b = tid; b < a.B; b += FD_THREADS)
    if (a.ref_index[b] == r) atomicMin(&owner_sh, b);
  __syncthreads();
  const int b = owner_sh;
  if (b >= a.B) return;
  const float *y = a.ref37 + (long)r * N * 111, *rm = a.res_mask + (long)b * N;
  const int* ch = a.chain_idx + (long)b * N;
  double* out = a.gt_dihedral + (long)r * 3 * N;
  for (int i = tid; i < N; i += FD_THREADS) {
    double d[3] = {0.0, 0.0, 0.0};
    if (rm[i] != 0.f) {
      const bool prev = i > 0 && rm[i - 1] != 0.f && ch[i - 1] == ch[i], next = i + 1 < N && rm[i + 1] != 0.f && ch[i + 1] == ch[i];
      ev_row_dihedrals(y, i, prev, next, d);
    }
    out[i] = d[0];
    out[N + i] = d[1];
    out[2 * (long)N + i] = d[2];
  }
}

__global__ __launch_bounds__(FD_THREADS) void evaluate_kernel(FdiptEvalArgs a) {
  __shared__ double red[FD_WAVES * 9];
  __shared__ double rot_sh[12];  // R (row-major), then t
  __shared__ int cnt[FD_WAVES], bad_sh, len_sh, nan_sh;
  __shared__ unsigned long long pairs_sh[2];  // pairs at distance > 0, clashes among them
  const int tid = threadIdx.x, lane = tid & (FD_WAVE - 1), wave = tid / FD_WAVE, N = a.N;
  if ((int)blockIdx.x >= a.B) {
    ev_reference_block(a, blockIdx.x - a.B);
    return;
  }
  const int b = blockIdx.x;
  const int r_idx = a.ref_index[b], g0 = a.region_start[b], G = a.region_start[b + 1] - g0;
  const float *dm = a.diffuse_mask + (long)b * N, *rm = a.res_mask + (long)b * N, *am = a.align_mask + (long)b * N;
  const int* ch = a.chain_idx + (long)b * N;
  if (tid == 0) {
    bad_sh = 0;
    len_sh = 0;
    nan_sh = 0;
    pairs_sh[0] = pairs_sh[1] = 0ull;
  }
  __syncthreads();

  // ---- phase 0: the device data decide what is addressed: a sample the host's table does not describe is skipped, not trusted
  bool ok = r_idx >= 0 && r_idx < a.R && g0 >= 0 && G >= 0 && g0 + G <= a.n_regions && G <= a.max_regions;
  int n_diffused = 0;
  for (int n0 = 0; n0 < N; n0 += FD_THREADS) {
    const int i = n0 + tid;
    n_diffused += __syncthreads_count(i < N && dm[i] != 0.f && rm[i] != 0.f);
  }
  if (ok) {
    for (int g = tid; g < G; g += FD_THREADS) {
      const int first = a.region_rows[2 * (g0 + g)], last = a.region_rows[2 * (g0 + g) + 1];
      int bad = first < 0 || last < first || last >= N;
      if (!bad) {
        const int c = ch[first];
        for (int i = first; i <= last; ++i) bad |= !(dm[i] != 0.f && rm[i] != 0.f && ch[i] == c);
        // maximal: the neighbours are not diffused rows of the same chain
        if (first > 0) bad |= dm[first - 1] != 0.f && rm[first - 1] != 0.f && ch[first - 1] == c;
        if (last + 1 < N) bad |= dm[last + 1] != 0.f && rm[last + 1] != 0.f && ch[last + 1] == c;
        for (int h = 0; h < g; ++h) bad |= a.region_rows[2 * (g0 + h)] == first;  // (maximal runs overlap only where they are equal)
        atomicAdd(&len_sh, last - first + 1);
      }
      if (bad) atomicOr(&bad_sh, 1);
    }
  }
  __syncthreads();
  ok = ok && !bad_sh && len_sh == n_diffused;
  if (!ok) {
    if (tid == 0) {
      a.status[b] = FDIPT_EVAL_SKIPPED;
      a.n_diffused[b] = n_diffused;
    }
    return;
  }
  const float *x = a.atom37 + (long)b * N * 111, *y = a.ref37 + (long)r_idx * N * 111;

  // ---- phase 1: backbone deviation without superposition
  for (int i = tid; i < N; i += FD_THREADS) {
    double v = 0.0;
    if (dm[i] != 0.f && rm[i] != 0.f) v = sqrt(ev_row_delta2(x + (long)i * 111, y + (long)i * 111) / 4.0);
    a.res_bb_rmsd[(long)b * N + i] = v;
  }
  double* region_out = a.region_bb_rmsd + (long)b * a.max_regions;
  for (int g = wave; g < G; g += FD_WAVES) {  // a wave per region: lane l takes rows first + l, first + l + 64, ...
    const int first = a.region_rows[2 * (g0 + g)], last = a.region_rows[2 * (g0 + g) + 1];
    double acc = 0.0;
    for (int i = first + lane; i <= last; i += FD_WAVE) acc += ev_row_delta2(x + (long)i * 111, y + (long)i * 111);
    acc = wave_sum_d(acc);
    if (lane == 0) region_out[g] = acc;  // (the sum; thread 0 turns it into the deviation below)
  }
  __syncthreads();
  if (tid == 0) {
    double total = 0.0;
    for (int g = 0; g < G; ++g) {
      const double s = region_out[g];
      total += s;
      region_out[g] = sqrt(s / (4.0 * (double)(a.region_rows[2 * (g0 + g) + 1] - a.region_rows[2 * (g0 + g)] + 1)));
    }
    a.bb_rmsd[b] = sqrt(total / (4.0 * (double)n_diffused));  // (no diffused row: 0 / 0 = NaN, np.sqrt(0 / 0) there)
  }

  // ---- phase 2: dihedrals per chain over the rows of res_mask, and the signed errors
  {
    double *ds = a.dihedral + (long)b * 3 * N, *er = a.angle_error + (long)b * 3 * N;
    int any_nan = 0;
    for (int i = tid; i < N; i += FD_THREADS) {
      double s[3] = {0.0, 0.0, 0.0}, t[3] = {0.0, 0.0, 0.0};
      if (rm[i] != 0.f) {
        const bool prev = i > 0 && rm[i - 1] != 0.f && ch[i - 1] == ch[i], next = i + 1 < N && rm[i + 1] != 0.f && ch[i + 1] == ch[i];
        ev_row_dihedrals(x, i, prev, next, s);
        ev_row_dihedrals(y, i, prev, next, t);
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        any_nan |= (s[k] != s[k]) || (t[k] != t[k]);
        ds[(long)k * N + i] = s[k];
        er[(long)k * N + i] = ev_signed_error(t[k], s[k]);  // (residue_signed_angle_error :1132: model_1 is the ground truth)
      }
    }
    if (any_nan) atomicOr(&nan_sh, 1);
  }

  // ---- phase 3: CA geometry over the rows with any non-zero coordinate (bb_mask), bonds regardless of chain breaks
  float* ca = (float*)a.workspace + (long)b * N * 3;
  int K = 0;
  for (int n0 = 0; n0 < N; n0 += FD_THREADS) {
    const int i = n0 + tid;
    bool flag = false;
    if (i < N) {
      const float* row = x + (long)i * 111;
      for (int k = 0; k < 111 && !flag; ++k) flag = row[k] != 0.f;
    }
    const unsigned long long bal = __ballot(flag);
    if (lane == 0) cnt[wave] = __popcll(bal);
    __syncthreads();
    int off = K, tot = 0;
#pragma unroll
    for (int v = 0; v < FD_WAVES; ++v) {
      if (v < wave) off += cnt[v];
      tot += cnt[v];
    }
    if (flag) {  // (pos < N: at most one position per row)
      const int pos = off + __popcll(bal & ((1ull << lane) - 1ull));
      const float* p = x + (long)i * 111 + 3;
      ca[3 * (long)pos] = p[0];
      ca[3 * (long)pos + 1] = p[1];
      ca[3 * (long)pos + 2] = p[2];
    }
    K += tot;
    __syncthreads();
  }
  {
    double bond[2] = {0.0, 0.0};  // sum |d - ca_ca|, number of d < ca_ca + 0.1
    for (int k = 1 + tid; k < K; k += FD_THREADS) {
      const EvVec d = ev_sub(ev_load(ca + 3 * (long)k), ev_load(ca + 3 * (long)(k - 1)));
      const double dist = sqrt(ev_dot(d, d));
      bond[0] += fabs(dist - EV_CA_CA);
      bond[1] += dist < EV_CA_CA + 0.1 ? 1.0 : 0.0;
    }
    fd_block_sum(bond, red);
    unsigned long long n_pos = 0ull, n_clash = 0ull;
    for (int i = wave; i < K; i += FD_WAVES) {
      const EvVec pi = ev_load(ca + 3 * (long)i);
      for (int j = i + 1 + lane; j < K; j += FD_WAVE) {
        const EvVec d = ev_sub(pi, ev_load(ca + 3 * (long)j));
        const double dist = sqrt(ev_dot(d, d));
        n_pos += dist > 0.0;
        n_clash += dist > 0.0 && dist < 1.5;
      }
    }
    atomicAdd(&pairs_sh[0], n_pos);
    atomicAdd(&pairs_sh[1], n_clash);
    __syncthreads();
    if (tid == 0) {  // np.mean of an empty array: 0 / 0 = NaN
      const double nb = (double)(K > 0 ? K - 1 : 0);
      a.ca_ca_bond_dev[b] = bond[0] / nb;
      a.ca_ca_valid_percent[b] = bond[1] / nb;
      a.num_ca_steric_clashes[b] = (int)pairs_sh[1];
      a.ca_steric_clash_percent[b] = (double)pairs_sh[1] / (double)pairs_sh[0];
    }
  }

  // ---- phase 4: superposition of the CA atoms of the align_mask rows onto the ground truth (rigid_transform_3D)
  double cen[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // sums of the sample's and the ground truth's CA, the number of rows
  for (int i = tid; i < N; i += FD_THREADS) {
    if (am[i] != 0.f) {
      const EvVec p = ev_load(x + (long)i * 111 + 3), q = ev_load(y + (long)i * 111 + 3);
      cen[0] += p.x; cen[1] += p.y; cen[2] += p.z;
      cen[3] += q.x; cen[4] += q.y; cen[5] += q.z;
      cen[6] += 1.0;
    }
  }
  fd_block_sum(cen, red);
  const double M = cen[6], inv_m = M > 0.0 ? 1.0 / M : 0.0;
  const EvVec ca_c = {cen[0] * inv_m, cen[1] * inv_m, cen[2] * inv_m}, cb_c = {cen[3] * inv_m, cen[4] * inv_m, cen[5] * inv_m};
  double H[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // H = sum (a - ca)(b - cb)'
  for (int i = tid; i < N; i += FD_THREADS) {
    if (am[i] != 0.f) {
      const EvVec p = ev_sub(ev_load(x + (long)i * 111 + 3), ca_c), q = ev_sub(ev_load(y + (long)i * 111 + 3), cb_c);
      H[0] += p.x * q.x; H[1] += p.x * q.y; H[2] += p.x * q.z;
      H[3] += p.y * q.x; H[4] += p.y * q.y; H[5] += p.y * q.z;
      H[6] += p.z * q.x; H[7] += p.z * q.y; H[8] += p.z * q.z;
    }
  }
  fd_block_sum(H, red);
  if (tid == 0) {
    double R[9], top, second, scale;
    fd_horn_rotation(H, R, top, second, scale);  // (horn.hpp)
    const double det = H[0] * (H[4] * H[8] - H[5] * H[7]) - H[1] * (H[3] * H[8] - H[5] * H[6]) + H[2] * (H[3] * H[7] - H[4] * H[6]);
    // the rotation is unique where the two largest eigenvalues differ: their gap is 2 (s2 + s3) of H's singular values, 2 (s2 - s3)
    // with a reflection; below 1e-9 of the matrix it is rounding
    const bool degenerate = M < 3.0 || !(top - second > 1e-9 * scale);
#pragma unroll
    for (int k = 0; k < 9; ++k) rot_sh[k] = R[k];
    // t = -R ca + cb
    rot_sh[9] = -(R[0] * ca_c.x + R[1] * ca_c.y + R[2] * ca_c.z) + cb_c.x;
    rot_sh[10] = -(R[3] * ca_c.x + R[4] * ca_c.y + R[5] * ca_c.z) + cb_c.y;
    rot_sh[11] = -(R[6] * ca_c.x + R[7] * ca_c.y + R[8] * ca_c.z) + cb_c.z;
#pragma unroll
    for (int k = 0; k < 9; ++k) fd_st(a.rotation + (long)b * 9 + k, rot_sh[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) fd_st(a.translation + (long)b * 3 + k, rot_sh[9 + k]);
    a.reflection[b] = det < 0.0;
    a.status[b] = (nan_sh ? FDIPT_EVAL_NAN_DIHEDRAL : 0) | (degenerate ? FDIPT_EVAL_DEGENERATE_ALIGNMENT : 0);
    a.n_diffused[b] = n_diffused;
  }
  __syncthreads();
  double dev[2] = {0.0, 0.0};  // sum of the distances, sum of their squares
  for (int i = tid; i < N; i += FD_THREADS) {
    if (am[i] != 0.f) {
      const EvVec p = ev_load(x + (long)i * 111 + 3), q = ev_load(y + (long)i * 111 + 3);
      const EvVec d = {rot_sh[0] * p.x + rot_sh[1] * p.y + rot_sh[2] * p.z + rot_sh[9] - q.x,
                       rot_sh[3] * p.x + rot_sh[4] * p.y + rot_sh[5] * p.z + rot_sh[10] - q.y,
                       rot_sh[6] * p.x + rot_sh[7] * p.y + rot_sh[8] * p.z + rot_sh[11] - q.z};
      const double d2 = ev_dot(d, d);
      dev[0] += sqrt(d2);
      dev[1] += d2;
    }
  }
  fd_block_sum(dev, red);
  if (tid == 0) {
    a.aligned_mean_dev[b] = dev[0] * inv_m;
    a.aligned_rmsd[b] = sqrt(dev[1] * inv_m);
  }
}

extern "C" size_t fdipt_eval_workspace_bytes(int B, int N) {
  if (B < 1 || N < 1) return 0;
  return (size_t)B * N * 3 * sizeof(float);
}

extern "C" int fdipt_sample_evaluate(const FdiptEvalArgs* a, fdipt_stream_t stream) {
  if (!a || a->B < 1 || a->N < 1 || a->R < 1 || a->n_regions < 0 || a->max_regions < 1) return FDIPT_EINVAL;
  if (!a->atom37 || !a->ref37 || !a->ref_index || !a->diffuse_mask || !a->res_mask || !a->align_mask || !a->chain_idx || !a->region_start ||
      !a->region_rows || !a->ref_index_host || !a->region_start_host || !a->res_bb_rmsd || !a->region_bb_rmsd || !a->bb_rmsd || !a->dihedral ||
      !a->gt_dihedral || !a->angle_error || !a->ca_ca_bond_dev || !a->ca_ca_valid_percent || !a->num_ca_steric_clashes ||
      !a->ca_steric_clash_percent || !a->aligned_mean_dev || !a->aligned_rmsd || !a->rotation || !a->translation || !a->reflection ||
      !a->status || !a->n_diffused || !a->workspace)
    return FDIPT_EINVAL;
  if (a->region_start_host[0] != 0 || a->region_start_host[a->B] != a->n_regions) return FDIPT_EINVAL;
  for (int b = 0; b < a->B; ++b) {
    const int G = a->region_start_host[b + 1] - a->region_start_host[b];
    if (G < 0 || G > a->max_regions) return FDIPT_EINVAL;
    if (a->ref_index_host[b] < 0 || a->ref_index_host[b] >= a->R) return FDIPT_EINVAL;
  }
  if ((long)a->B + a->R > 0x7fffffffL) return FDIPT_ESIZE;
  if (a->workspace_bytes < fdipt_eval_workspace_bytes(a->B, a->N)) return FDIPT_ESIZE;
  hipLaunchKernelGGL(evaluate_kernel, dim3(a->B + a->R), dim3(FD_THREADS), 0, (hipStream_t)stream, *a);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
