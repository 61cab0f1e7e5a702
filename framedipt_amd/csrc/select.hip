// select.hip — sample selection on the device (include/fdipt.h, "sample selection"): mean, geometric median, mode and the samples
// closest to mean and median of evaluation/utils/sample_selection.py, for G groups of samples in one launch, all in float64.
//
// One block of FD_THREADS serves a group.  Phases (a __syncthreads between them, nothing leaves the launch):
//   0  residue list: ordered compaction of the first member's diffuse_mask                      (all waves)
//   1  mean [L,4,3], summed over the samples in index order                                       (all waves)
//   2  pair statistics: D_sr = sum (x_s - x_r)^2 summed directly, G_sr = sum (x_s - mu)(x_r - mu)   (all waves, a thread per pair s <= r)
//   3  density and mode, then the Weiszfeld iteration in weight space                              (wave 0, lane s owns row s of G)
//   4  median coordinates, the two distance vectors, the two argmins                               (all waves)
// G lives in LDS (64 x 65 doubles: lane s reads G[s][r] at r = 0 .. S - 1, rows 65 apart fall on different banks); D, read once,
// and the residue list live in the caller's workspace.  An iteration is O(S^2) whatever L is: the matrix-vector product takes w_r from
// lane r by v_readlane (r is wave-uniform), and the two sums of an iteration (w'Gw, sum 1/d) add the lanes' values in index order the
// same way, so every lane holds the same bits and short groups (S = 5 is the reference default) pay for 5 terms, not for a 64-lane
// butterfly.
#include "common.hpp"

#define SEL_S FDIPT_SELECT_MAX_SAMPLES
#define SEL_LDG (SEL_S + 1)

// lanes 0 .. S - 1 added in index order
__device__ __forceinline__ double sel_ordered_sum(double v, int S) {
  double acc = 0.0;
  for (int r = 0; r < S; ++r) acc += fd_readlane_d(v, r);
  return acc;
}
// index of the largest (sign = -1) / smallest (sign = +1) of lanes 0 .. S - 1; the lowest index wins on equality (np.argmax / argmin)
__device__ __forceinline__ int sel_arg_best(double v, int S, double sign) {
  double best = sign * fd_readlane_d(v, 0);
  int idx = 0;
  for (int r = 1; r < S; ++r) {
    const double x = sign * fd_readlane_d(v, r);
    if (x < best) { best = x; idx = r; }
  }
  return idx;
}

__global__ __launch_bounds__(FD_THREADS) void select_kernel(FdiptSelectArgs a) {
  __shared__ double Gs[SEL_S * SEL_LDG];
  __shared__ double w_sh[SEL_S], dist_sh[2][SEL_S];
  __shared__ long mbase[SEL_S];  // float offset of every member's atom37 block
  __shared__ int cnt[FD_WAVES], hit_sh;
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & (FD_WAVE - 1), wave = tid / FD_WAVE;
  const int N = a.N, L_max = a.L_max;
  const int b0 = a.group_start[g], S = a.group_start[g + 1] - b0;
  double* Dg = (double*)a.workspace + (size_t)g * (SEL_S * SEL_S);
  int* res = (int*)((double*)a.workspace + (size_t)a.G * (SEL_S * SEL_S)) + (size_t)g * L_max;

  // the device data decide what is addressed: a group the host counts do not describe is skipped, not trusted
  bool ok = S >= 1 && S <= SEL_S && b0 >= 0 && b0 + S <= a.B;
  int bad = 0;
  if (ok && tid < S) {
    const int mb = a.member[b0 + tid];
    bad = mb < 0 || mb >= a.B;
    mbase[tid] = (long)(bad ? 0 : mb) * N * 111;
  }
  const int any_bad = __syncthreads_or(bad);
  ok = ok && !any_bad;
  int L = 0;
  if (ok) {  // phase 0 (block-uniform branch)
    const float* mask = a.diffuse_mask + mbase[0] / 111;
    for (int n0 = 0; n0 < N; n0 += FD_THREADS) {
      const int i = n0 + tid;
      const bool flag = i < N && mask[i] != 0.f;
      const unsigned long long bal = __ballot(flag);
      if (lane == 0) cnt[wave] = __popcll(bal);
      __syncthreads();
      int off = L, tot = 0;
#pragma unroll
      for (int v = 0; v < FD_WAVES; ++v) {
        if (v < wave) off += cnt[v];
        tot += cnt[v];
      }
      const int pos = off + __popcll(bal & ((1ull << lane) - 1ull));
      if (flag && pos < L_max) res[pos] = i;
      L += tot;
      __syncthreads();
    }
    ok = L >= 1 && L <= L_max;
  }
  if (!ok) {
    if (tid == 0) {
      a.status[g] = FDIPT_SELECT_SKIPPED;
      a.n_diffused[g] = L;
      a.index[g * 3] = a.index[g * 3 + 1] = a.index[g * 3 + 2] = -1;
    }
    return;
  }
  const int M = 12 * L;
  double* mean = a.mean + (size_t)g * L_max * 12;
  double* median = a.median + (size_t)g * L_max * 12;
  const float* x = a.atom37;

  // phase 1: mean (np.mean over the sample axis: the samples added in index order, one division)
  for (int m = tid; m < M; m += FD_THREADS) {
    const int l = m / 12, o = m - 12 * l;
    const long k = (long)res[l] * 111 + fd_backbone_off(o / 3) + o % 3;
    double acc = 0.0;
    for (int s = 0; s < S; ++s) acc += (double)x[mbase[s] + k];
    mean[m] = acc / (double)S;
  }
  __syncthreads();

  // phase 2: pair statistics, one thread per pair s <= r (both are symmetric bit for bit)
  for (int p = tid; p < S * S; p += FD_THREADS) {
    const int s = p / S, r = p - s * S;
    if (r < s) continue;
    const float *xs = x + mbase[s], *xr = x + mbase[r];
    double D = 0.0, Gv = 0.0;
    for (int l = 0; l < L; ++l) {
      const long k0 = (long)res[l] * 111;
#pragma unroll
      for (int o = 0; o < 12; ++o) {
        const long k = k0 + fd_backbone_off(o / 3) + o % 3;
        const double vs = (double)xs[k], vr = (double)xr[k], mu = mean[l * 12 + o], d = vs - vr;
        D = fma(d, d, D);
        Gv = fma(vs - mu, vr - mu, Gv);
      }
    }
    Gs[s * SEL_LDG + r] = Gv;
    Gs[r * SEL_LDG + s] = Gv;
    Dg[s * SEL_S + r] = D;
    Dg[r * SEL_S + s] = D;
  }
  __syncthreads();

  // phase 3 (wave 0; every lane executes, lanes >= S carry w = 0 and read row 0)
  if (wave == 0) {
    const bool act = lane < S;
    const int row = act ? lane : 0;
    const double s2 = a.sigma * a.sigma;
    double dens = 0.0;
    for (int r = 0; r < S; ++r) dens += exp(-Dg[row * SEL_S + r] / s2);
    const int mode = sel_arg_best(dens, S, -1.0);
    const double* Grow = Gs + row * SEL_LDG;
    const double gss = Grow[row];
    double w = act ? 1.0 / (double)S : 0.0;
    int hit = -1;
    for (int it = 0; it < a.max_iterations; ++it) {
      double gw = 0.0;
      int r = 0;
      for (; r + 4 <= S; r += 4) {  // four LDS reads in flight (the compiler does not unroll around v_readlane); one chain in index order
        const double g0 = Grow[r], g1 = Grow[r + 1], g2 = Grow[r + 2], g3 = Grow[r + 3];
        gw = fma(g0, fd_readlane_d(w, r), gw);
        gw = fma(g1, fd_readlane_d(w, r + 1), gw);
        gw = fma(g2, fd_readlane_d(w, r + 2), gw);
        gw = fma(g3, fd_readlane_d(w, r + 3), gw);
      }
      for (; r < S; ++r) gw = fma(Grow[r], fd_readlane_d(w, r), gw);
      const double wgw = sel_ordered_sum(w * gw, S);
      const double d = sqrt(fmax(gss - 2.0 * gw + wgw, 0.0));
      const unsigned long long zero = __ballot(act && d == 0.0);
      if (zero) {  // the reference divides by zero here ("div 0 issue!")
        hit = __ffsll((long long)zero) - 1;
        w = lane == hit ? 1.0 : 0.0;
        break;
      }
      const double inv = act ? 1.0 / d : 0.0;
      w = inv / sel_ordered_sum(inv, S);
    }
    if (act) {
      w_sh[lane] = w;
      a.weights[b0 + lane] = w;
      a.density[b0 + lane] = dens;
    }
    if (lane == 0) {
      hit_sh = hit;
      a.status[g] = hit >= 0 ? FDIPT_SELECT_ZERO_DISTANCE : 0;
      a.n_diffused[g] = L;
      a.index[g * 3] = mode;
    }
  }
  __syncthreads();

  // phase 4: median = mu + sum_s w_s (x_s - mu); the sample itself after a zero distance
  const int hit = hit_sh;
  for (int m = tid; m < M; m += FD_THREADS) {
    const int l = m / 12, o = m - 12 * l;
    const long k = (long)res[l] * 111 + fd_backbone_off(o / 3) + o % 3;
    const double mu = mean[m];
    double med;
    if (hit >= 0) {
      med = (double)x[mbase[hit] + k];
    } else {
      double acc = 0.0;
      for (int s = 0; s < S; ++s) acc = fma(w_sh[s], (double)x[mbase[s] + k] - mu, acc);
      med = mu + acc;
    }
    median[m] = med;
  }
  __syncthreads();
  // get_closest_index: per sample the sum over atoms of the Euclidean distance to the reference point; a wave per sample
  for (int s = wave; s < S; s += FD_WAVES) {
    const float* xs = x + mbase[s];
    double pm = 0.0, pd = 0.0;
    for (int j = lane; j < 4 * L; j += FD_WAVE) {
      const int l = j >> 2, at = j & 3;
      const float* p = xs + (long)res[l] * 111 + fd_backbone_off(at);
      const double *mu = mean + j * 3, *md = median + j * 3;
      const double v0 = (double)p[0], v1 = (double)p[1], v2 = (double)p[2];
      const double a0 = v0 - mu[0], a1 = v1 - mu[1], a2 = v2 - mu[2], c0 = v0 - md[0], c1 = v1 - md[1], c2 = v2 - md[2];
      pm += sqrt(a0 * a0 + a1 * a1 + a2 * a2);
      pd += sqrt(c0 * c0 + c1 * c1 + c2 * c2);
    }
    pm = wave_sum_d(pm);
    pd = wave_sum_d(pd);
    if (lane == 0) {
      dist_sh[0][s] = pm;
      dist_sh[1][s] = pd;
      a.dist_to_mean[b0 + s] = pm;
      a.dist_to_median[b0 + s] = pd;
    }
  }
  __syncthreads();
  if (wave == 0) {
    const int row = lane < S ? lane : 0;
    const int c_mean = sel_arg_best(dist_sh[0][row], S, 1.0), c_med = sel_arg_best(dist_sh[1][row], S, 1.0);
    if (lane == 0) {
      a.index[g * 3 + 1] = c_mean;
      a.index[g * 3 + 2] = c_med;
    }
  }
}

static size_t sel_residue_bytes(int G, int L_max) { return ((size_t)G * L_max * sizeof(int32_t) + 7) & ~(size_t)7; }

extern "C" size_t fdipt_select_workspace_bytes(int G, int B, int L_max) {
  if (G < 1 || B < 1 || L_max < 1) return 0;
  return (size_t)G * SEL_S * SEL_S * sizeof(double) + sel_residue_bytes(G, L_max);
}

extern "C" int fdipt_sample_select(const FdiptSelectArgs* a, fdipt_stream_t stream) {
  if (!a || a->B < 1 || a->N < 1 || a->G < 1 || a->L_max < 1 || a->max_iterations < 0 || !(a->sigma > 0.0)) return FDIPT_EINVAL;
  if (!a->atom37 || !a->diffuse_mask || !a->group_start || !a->member || !a->group_start_host || !a->n_diffused_host || !a->mean ||
      !a->median || !a->weights || !a->density || !a->dist_to_mean || !a->dist_to_median || !a->index || !a->status || !a->n_diffused ||
      !a->workspace)
    return FDIPT_EINVAL;
  if (a->group_start_host[0] != 0) return FDIPT_EINVAL;
  for (int g = 0; g < a->G; ++g) {
    const int S = a->group_start_host[g + 1] - a->group_start_host[g], L = a->n_diffused_host[g];
    if (S > SEL_S) return FDIPT_ESIZE;
    if (S < 1 || L < 1 || L > a->L_max || L > a->N) return FDIPT_EINVAL;
  }
  if (a->group_start_host[a->G] > a->B) return FDIPT_EINVAL;
  if (a->workspace_bytes < fdipt_select_workspace_bytes(a->G, a->B, a->L_max)) return FDIPT_ESIZE;
  hipLaunchKernelGGL(select_kernel, dim3(a->G), dim3(FD_THREADS), 0, (hipStream_t)stream, *a);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
