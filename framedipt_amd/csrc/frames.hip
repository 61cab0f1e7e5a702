// frames.hip — rigid-frame algebra, SO(3) exp/log (SciPy conventions), the fused reverse step,
// IGSO(3) / R^3 scores and idealised backbone atoms.  All O(N) kernels: a few KB of state, latency-bound.
// Reference lines are cited per function (paths relative to the reference repository root).
#include "common.hpp"
#include "kernels.hpp"
#include "philox.hpp"

#pragma clang fp contract(off)  // keep the float32 evaluation order of the reference expressions

// ------------------------------------------------------------------ float32 quaternion algebra
__device__ __forceinline__ void d_quat_to_rot(const float* q, float* R) {  // openfold/utils/rigid_utils.py:173-205
  const float a = q[0], b = q[1], c = q[2], d = q[3];
  R[0] = a * a + b * b - c * c - d * d; R[1] = 2 * b * c - 2 * a * d; R[2] = 2 * b * d + 2 * a * c;
  R[3] = 2 * b * c + 2 * a * d; R[4] = a * a - b * b + c * c - d * d; R[5] = 2 * c * d - 2 * a * b;
  R[6] = 2 * b * d - 2 * a * c; R[7] = 2 * c * d + 2 * a * b; R[8] = a * a - b * b - c * c + d * d;
}
__device__ __forceinline__ void d_quat_mul(const float* p, const float* q, float* o) {  // rigid_utils.py:230-263
  o[0] = p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3];
  o[1] = p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2];
  o[2] = p[0] * q[2] - p[1] * q[3] + p[2] * q[0] + p[3] * q[1];
  o[3] = p[0] * q[3] + p[1] * q[2] - p[2] * q[1] + p[3] * q[0];
}
__device__ __forceinline__ void d_quat_mul_vec(const float* q, const float* v, float* o) {  // rigid_utils.py:266-279
  o[0] = -q[1] * v[0] - q[2] * v[1] - q[3] * v[2];
  o[1] = q[0] * v[0] + q[2] * v[2] - q[3] * v[1];
  o[2] = q[0] * v[1] - q[1] * v[2] + q[3] * v[0];
  o[3] = q[0] * v[2] + q[1] * v[1] - q[2] * v[0];
}
__device__ __forceinline__ void d_invert_quat(const float* q, float* o) {  // rigid_utils.py:282-286
  const float n = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  o[0] = q[0] / n; o[1] = -q[1] / n; o[2] = -q[2] / n; o[3] = -q[3] / n;
}
__device__ __forceinline__ void d_rot_vec(const float* R, const float* v, float* o) {  // rigid_utils.py:82-106
  o[0] = R[0] * v[0] + R[1] * v[1] + R[2] * v[2];
  o[1] = R[3] * v[0] + R[4] * v[1] + R[5] * v[2];
  o[2] = R[6] * v[0] + R[7] * v[1] + R[8] * v[2];
}
__device__ __forceinline__ void d_quat_to_rotvec(const float* qin, float* rv) {  // framedipt/data/transforms.py:53-69
  float q[4] = {qin[0], qin[1], qin[2], qin[3]};
  if (q[0] < 0.f) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
  const float nv = sqrtf(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const float angle = 2.f * atan2f(nv, q[0]);
  const float a2 = angle * angle;
  const float sc = (angle <= 1e-3f) ? (2.f + a2 / 12.f + 7.f * a2 * a2 / 2880.f) : (angle / sinf(angle / 2.f + 1e-6f));
  rv[0] = sc * q[1]; rv[1] = sc * q[2]; rv[2] = sc * q[3];
}

// ------------------------------------------------------------------ SciPy Rotation conventions, float64
// Rotation.from_rotvec(rv).as_matrix()  (framedipt/data/transforms.py:42 ; se3_diffuser.py:31)
// Rotation(quat).as_matrix() for a unit quaternion (x, y, z, w)
__device__ __forceinline__ void d_quat_matrix(const double* q, double* R) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w;
  const double xy = x * y, zw = z * w, xz = x * z, yw = y * w, yz = y * z, xw = x * w;
  R[0] = x2 - y2 - z2 + w2; R[3] = 2 * (xy + zw); R[6] = 2 * (xz - yw);
  R[1] = 2 * (xy - zw); R[4] = -x2 + y2 - z2 + w2; R[7] = 2 * (yz + xw);
  R[2] = 2 * (xz + yw); R[5] = 2 * (yz - xw); R[8] = -x2 - y2 + z2 + w2;
}
__device__ __forceinline__ void d_so3_exp(const double* rv, double* R) {
  const double th2 = rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2];
  const double th = sqrt(th2);
  const double sc = (th <= 1e-3) ? (0.5 - th2 / 48.0 + th2 * th2 / 3840.0) : (sin(th / 2) / th);
  const double q[4] = {sc * rv[0], sc * rv[1], sc * rv[2], cos(th / 2)};
  d_quat_matrix(q, R);
}
// Markley quaternion of a 3x3 matrix (Rotation.from_matrix, SciPy 1.7.3 = the reference pin: no SVD projection).
// q is scalar-LAST (x,y,z,w), normalised.
__device__ __forceinline__ void d_markley(const double* m, double* q) {
  const double d0 = m[0], d1 = m[4], d2 = m[8], tr = d0 + d1 + d2;
  int ch = 0;
  double best = d0;
  if (d1 > best) { best = d1; ch = 1; }
  if (d2 > best) { best = d2; ch = 2; }
  if (tr > best) { ch = 3; }
  if (ch == 3) {
    q[0] = m[7] - m[5]; q[1] = m[2] - m[6]; q[2] = m[3] - m[1]; q[3] = 1 + tr;
  } else {
    const int i = ch, j = (i + 1) % 3, k = (j + 1) % 3;
    q[i] = 1 - tr + 2 * m[i * 3 + i];
    q[j] = m[j * 3 + i] + m[i * 3 + j];
    q[k] = m[k * 3 + i] + m[i * 3 + k];
    q[3] = m[k * 3 + j] - m[j * 3 + k];
  }
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n;
}
// Rotation.from_matrix(m).as_rotvec()  (framedipt/data/transforms.py:46 ; se3_diffuser.py:21)
__device__ __forceinline__ void d_so3_log(const double* m, double* rv) {
  double q[4];
  d_markley(m, q);
  if (q[3] < 0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
  const double ang = 2 * atan2(sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]), q[3]);
  const double a2 = ang * ang;
  const double sc = (ang <= 1e-3) ? (2 + a2 / 12 + 7 * a2 * a2 / 2880) : (ang / sin(ang / 2));
  rv[0] = sc * q[0]; rv[1] = sc * q[1]; rv[2] = sc * q[2];
}

struct BackboneTables {  // packed by framedipt_amd/residue_tables.py
  float default_frames[21 * 8 * 16];
  float ideal_pos[21 * 14 * 3];
  float atom_mask[21 * 14];
  int32_t group_idx[21 * 14];
};

__device__ __forceinline__ void d_compose(const float* R1, const float* t1, const float* R2, const float* t2, float* Ro,
                                          float* to) {  // Rigid.compose, rigid_utils.py:1065-1079
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Ro[i * 3 + j] = R1[i * 3] * R2[j] + R1[i * 3 + 1] * R2[3 + j] + R1[i * 3 + 2] * R2[6 + j];
  float tmp[3];
  d_rot_vec(R1, t2, tmp);
  to[0] = tmp[0] + t1[0]; to[1] = tmp[1] + t1[1]; to[2] = tmp[2] + t1[2];
}

// all_atom.compute_backbone for residue r with frame (Rb, tbv)
__device__ __forceinline__ void d_backbone_residue(long r, const float* Rb, const float* tbv, const float* __restrict__ psi,
                                                   const int32_t* __restrict__ aatype, const BackboneTables* __restrict__ tb,
                                                   float* __restrict__ atom37, float* __restrict__ atom14) {
  int aa = aatype ? aatype[r] : 0;
  if (aa == 20) aa = 0;
  const float s = psi[r * 2], co = psi[r * 2 + 1];
  float FR[8][9], FT[8][3];
  for (int g = 0; g < 8; ++g) {
    const float* d44 = tb->default_frames + (aa * 8 + g) * 16;
    float Rd[9], td[3], Ra[9];
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) Rd[i * 3 + j] = d44[i * 4 + j];
      td[i] = d44[i * 4 + 3];
    }
    const float a0 = g == 0 ? 0.f : s, a1 = g == 0 ? 1.f : co;  // backbone frame: (sin,cos) = (0,1)
    Ra[0] = 1; Ra[1] = 0; Ra[2] = 0; Ra[3] = 0; Ra[4] = a1; Ra[5] = -a0; Ra[6] = 0; Ra[7] = a0; Ra[8] = a1;
    const float z3[3] = {0.f, 0.f, 0.f};
    d_compose(Rd, td, Ra, z3, FR[g], FT[g]);
  }
  for (int g = 5; g < 8; ++g) {  // chi2..chi4 chained onto chi1 (feats.py:204-212)
    float Rn[9], tn[3];
    d_compose(FR[g - 1], FT[g - 1], FR[g], FT[g], Rn, tn);
    for (int c = 0; c < 9; ++c) FR[g][c] = Rn[c];
    for (int c = 0; c < 3; ++c) FT[g][c] = tn[c];
  }
  float pos[14][3];
  for (int at = 0; at < 14; ++at) {
    const int g = tb->group_idx[aa * 14 + at];
    float Rg[9], tg[3], p[3];
    d_compose(Rb, tbv, FR[g], FT[g], Rg, tg);
    d_rot_vec(Rg, tb->ideal_pos + (aa * 14 + at) * 3, p);
    const float mk = tb->atom_mask[aa * 14 + at];
    for (int c = 0; c < 3; ++c) pos[at][c] = (p[c] + tg[c]) * mk;
  }
  if (atom14)
    for (int at = 0; at < 14; ++at)
      for (int c = 0; c < 3; ++c) fd_st(atom14 + (r * 14 + at) * 3 + c, pos[at][c]);
  if (atom37) {
    for (int c = 0; c < 37 * 3; ++c) atom37[r * 111 + c] = 0.f;  // (merged wide stores of a constant register: nothing overwrites it)
    // atom14 order N,CA,C,O,CB -> atom37 order N,CA,C,CB,O (all_atom.py:168-174)
    const int map[5] = {0, 1, 2, 4, 3};
    for (int at = 0; at < 5; ++at)
      for (int c = 0; c < 3; ++c) fd_st(atom37 + r * 111 + at * 3 + c, pos[map[at]][c]);
  }
}

// One atom of all_atom.compute_backbone: atom `at` (atom14 index) of residue type aa with frame (Rb, tbv) and psi = (s, co).  The same
// expressions in the same order as d_backbone_residue evaluates for that atom (only the frames of its own group chain are built).
__device__ __forceinline__ void d_backbone_atom(int at, int aa, float s, float co, const float* Rb, const float* tbv,
                                                const BackboneTables* __restrict__ tb, float* p3) {
  const int g = tb->group_idx[aa * 14 + at];
  auto frame = [&](int gg, float* R, float* T) {
    const float* d44 = tb->default_frames + (aa * 8 + gg) * 16;
    float Rd[9], td[3], Ra[9];
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) Rd[i * 3 + j] = d44[i * 4 + j];
      td[i] = d44[i * 4 + 3];
    }
    const float a0 = gg == 0 ? 0.f : s, a1 = gg == 0 ? 1.f : co;
    Ra[0] = 1; Ra[1] = 0; Ra[2] = 0; Ra[3] = 0; Ra[4] = a1; Ra[5] = -a0; Ra[6] = 0; Ra[7] = a0; Ra[8] = a1;
    const float z3[3] = {0.f, 0.f, 0.f};
    d_compose(Rd, td, Ra, z3, R, T);
  };
  float FRg[9], FTg[3];
  frame(g < 5 ? g : 4, FRg, FTg);
  for (int gg = 5; gg <= g; ++gg) {  // chi2..chi4 chained onto chi1 (feats.py:204-212)
    float Rc[9], Tc[3], Rn[9], Tn[3];
    frame(gg, Rc, Tc);
    d_compose(FRg, FTg, Rc, Tc, Rn, Tn);
    for (int c = 0; c < 9; ++c) FRg[c] = Rn[c];
    for (int c = 0; c < 3; ++c) FTg[c] = Tn[c];
  }
  float Rg[9], tg[3], p[3];
  d_compose(Rb, tbv, FRg, FTg, Rg, tg);
  d_rot_vec(Rg, tb->ideal_pos + (aa * 14 + at) * 3, p);
  const float mk = tb->atom_mask[aa * 14 + at];
  for (int c = 0; c < 3; ++c) p3[c] = (p[c] + tg[c]) * mk;
}

// ------------------------------------------------------------------ fused reverse step
// grid (row blocks, samples): every block recomputes its sample's centre-of-mass sums (cheap: a few fused multiply-adds per
// residue, the same summation order in every block), then takes rpb residues through the float64 SO(3) exp / log chain (a
// long dependent sequence: one residue per lane, as many waves on as many CUs as the batch allows).  In-place updates
// (rigids_out == rigids_t) need the whole sample in one block: rpb = N.
struct ReverseArgs {  // filled by name (the exported entries below); what an entry does not have stays NULL / 0
  int B = 0, N = 0;
  const float* rigids_t = nullptr;
  const double* rot_score = nullptr;
  const float* trans_score = nullptr;
  const float* diffuse_mask = nullptr;
  const double *z_rot = nullptr, *z_trans = nullptr;
  double t = 0, dt = 0, noise_scale = 0;
  int center = 0, diffuse_rot = 0, diffuse_trans = 0;
  double so3_min_sigma = 0, so3_max_sigma = 0, r3_min_b = 0, r3_max_b = 0, cs = 0;
  float* rigids_out = nullptr;
  float* out_rot = nullptr;
  int rpb = 0;  // residues per block in the second pass (reverse_launch sets it)
  const float* psi = nullptr;  // optional compute_backbone of x_{t-1} (atom37 != nullptr)
  const int32_t* aatype = nullptr;
  const BackboneTables* tables = nullptr;
  float* atom37 = nullptr;
  // optional trans_traj row of the trajectory (experiments/utils.py:390-400): diffuse_mask * trans(x_0 prediction) + fixed * trans(x_{t-1})
  const float* pred_rigids = nullptr;   // [B,N,7] x_0 prediction of this step's forward
  const float* traj_fixed = nullptr;    // [B,N] fixed_mask * res_mask
  float* trans_traj = nullptr;          // [B,N,3]
  // optional step cursor (fdipt_se3_reverse_step_indexed; kernels.hpp: FdStep): rigids_t / rigids_out / z_* / atom37 / trans_traj /
  // kept_rigids are then bases of per-step arrays whose rows fd_step_rows picks, the step's time is t_table[k], and the last block to
  // finish advances the cursor.  A step that keeps no frame (row -1) builds no backbone and writes no trans_traj / kept_rigids row.
  FdStep step;
  const double* t_table = nullptr;
  float* kept_rigids = nullptr;  // [rows,B,N,7] copy of x_{t-1} in the frame's row
  // GEN (the *_gen entries, noise="device"): z_rot / z_trans are NULL and every value is drawn in the kernel from the sample's key
  // (philox.hpp: a function of key, purpose, step, residue index within the sample and component only); the step is the cursor's, or
  // noise_step without a cursor
  const uint64_t* noise_keys = nullptr;  // [B]
  int noise_step = 0;
};

// GEN: both passes need z_trans and both draw it: N / rpb times the Philox work of one pass, a few dozen integer operations per residue,
// against a buffer or a launch of its own.  KEPT is nothing but the argument of fd_step_rows (kernels.hpp).  Measured on one MI355X against
// the commit before the resolver (c4 bench, medians of three interleaved runs, us per call): <false, false> 24.25 against 26.31 on a lease
// that spread the parent over 5 us; with the addressing decided at run time 26.46 against 26.00 (allowed 26.31).  DESIGN.md section 7.2.
template <bool GEN, bool KEPT>
__global__ __launch_bounds__(FD_THREADS) void reverse_step_kernel(ReverseArgs a) {
  __shared__ double red[4][FD_THREADS / 64];
  __shared__ double com[4];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N;
  const FdStepRows at = fd_step_rows<KEPT>(a.step);
  const long R = (long)a.B * N;
  const uint64_t key = GEN ? a.noise_keys[b] : 0;
  const int step = a.step.cursor ? (int)at.step : a.noise_step;
  a.rigids_t += at.state_in * R * 7;
  a.rigids_out += at.state_out * R * 7;
  if (!GEN) {
    a.z_rot += at.step * R * 3;
    a.z_trans += at.step * R * 3;
  }
  if (a.step.cursor) a.t = a.t_table[at.step];
  if (at.frame < 0) {
    a.atom37 = a.trans_traj = a.kept_rigids = nullptr;
  } else {
    if (a.atom37) a.atom37 += at.frame * R * 111;
    if (a.trans_traj) a.trans_traj += at.frame * R * 3;
    if (a.kept_rigids) a.kept_rigids += at.frame * R * 7;
  }
  // schedules: so3_diffuser.py:299-319, r3_diffuser.py:48-85
  const double emax = exp(a.so3_max_sigma), emin = exp(a.so3_min_sigma);
  const double sig = log(a.t * emax + (1 - a.t) * emin);
  const double g_rot = sqrt(2 * (emax - emin) * sig / exp(sig));
  const double bt = a.r3_min_b + a.t * (a.r3_max_b - a.r3_min_b);
  const double g_tr = sqrt(bt);
  const double sdt = sqrt(a.dt);
  double sx = 0, sy = 0, sz = 0, sm = 0;
  // pass 1: translations x_{t-1} before centring (r3_diffuser.py:368-378), accumulate COM sums
  for (int i = tid; i < N; i += FD_THREADS) {
    const long r = (long)b * N + i;
    const double m = a.diffuse_mask ? (double)a.diffuse_mask[r] : 1.0;
    double x1[3], zt[3] = {0.0, 0.0, 0.0};
    if (GEN && a.diffuse_trans) fd_noise3(key, (uint32_t)i, (uint32_t)step, FD_NOISE_REV_TRANS, zt);
    for (int c = 0; c < 3; ++c) {
      const double x = (double)a.rigids_t[r * 7 + 4 + c] * a.cs;
      const double f = -0.5 * bt * x;
      const double z = a.noise_scale * (GEN ? zt[c] : a.z_trans[r * 3 + c]);
      double pert = (f - g_tr * g_tr * (double)a.trans_score[r * 3 + c]) * a.dt + g_tr * sdt * z;
      pert *= m;
      x1[c] = x - pert;
    }
    sx += x1[0]; sy += x1[1]; sz += x1[2]; sm += m;
  }
  sx = wave_sum_d(sx); sy = wave_sum_d(sy); sz = wave_sum_d(sz); sm = wave_sum_d(sm);
  if (lane == 0) { red[0][wave] = sx; red[1][wave] = sy; red[2][wave] = sz; red[3][wave] = sm; }
  __syncthreads();
  if (tid < 4) {
    double s = 0;
    for (int w = 0; w < FD_THREADS / 64; ++w) s += red[tid][w];
    com[tid] = s;
  }
  __syncthreads();
  // COM quirk of the reference: sum over ALL residues divided by the number of DIFFUSED residues (r3:379-383)
  const double cx = a.center ? com[0] / com[3] : 0.0, cy = a.center ? com[1] / com[3] : 0.0,
               cz = a.center ? com[2] / com[3] : 0.0;
  const int i_end = (int)(blockIdx.x + 1) * a.rpb < N ? (int)(blockIdx.x + 1) * a.rpb : N;
  for (int i = blockIdx.x * a.rpb + tid; i < i_end; i += FD_THREADS) {
    const long r = (long)b * N + i;
    const bool has_mask = a.diffuse_mask != nullptr;
    const double m = has_mask ? (double)a.diffuse_mask[r] : 1.0;
    // ---- translation
    double tr_out[3], zt[3] = {0.0, 0.0, 0.0}, zr[3] = {0.0, 0.0, 0.0};
    if (GEN && a.diffuse_trans) fd_noise3(key, (uint32_t)i, (uint32_t)step, FD_NOISE_REV_TRANS, zt);
    for (int c = 0; c < 3; ++c) {
      const double xt = (double)a.rigids_t[r * 7 + 4 + c];
      double x1 = xt;
      if (a.diffuse_trans) {
        const double x = xt * a.cs;
        const double f = -0.5 * bt * x;
        const double z = a.noise_scale * (GEN ? zt[c] : a.z_trans[r * 3 + c]);
        double pert = (f - g_tr * g_tr * (double)a.trans_score[r * 3 + c]) * a.dt + g_tr * sdt * z;
        pert *= m;
        x1 = x - pert;
        x1 -= (c == 0 ? cx : (c == 1 ? cy : cz));
        x1 = x1 / a.cs;
      }
      tr_out[c] = has_mask ? (m * x1 + (1 - m) * xt) : x1;  // se3_diffuser.py:397-399
    }
    // ---- rotation: f32 quat -> f32 matrix -> f64 rotvec (se3_diffuser.py:16-23)
    float R32[9];
    d_quat_to_rot(a.rigids_t + r * 7, R32);
    double Rt[9], Ro[9];
    for (int c = 0; c < 9; ++c) Rt[c] = (double)R32[c];
    double pert[3];
    if (GEN && a.diffuse_rot) fd_noise3(key, (uint32_t)i, (uint32_t)step, FD_NOISE_REV_ROT, zr);
    for (int c = 0; c < 3; ++c)
      pert[c] = g_rot * g_rot * a.rot_score[r * 3 + c] * a.dt + g_rot * sdt * (a.noise_scale * (GEN ? zr[c] : a.z_rot[r * 3 + c]));
    if (!has_mask || m == 1.0 || m == 0.0) {
      // Binary masks (the only ones the samplers produce): the rotation vectors of the reference are only ever passed through
      // exp(log(.)), which is the matrix of the Markley unit quaternion — from_rotvec(as_rotvec(q)).as_matrix() and
      // q.as_matrix() agree to float64 rounding, far below the float32 cast that follows — so the chain
      // log -> exp, exp -> compose -> log -> exp collapses to two quaternion extractions and ONE sin/cos pair (the float64
      // atan2 / sin / cos calls are the whole latency of this kernel).
      double q0[4];
      d_markley(Rt, q0);
      if (a.diffuse_rot && m != 0.0) {
        double Re[9], Rp[9], Rc[9], q1[4];
        d_quat_matrix(q0, Re);
        d_so3_exp(pert, Rp);
        for (int ii = 0; ii < 3; ++ii)
          for (int jj = 0; jj < 3; ++jj)
            Rc[ii * 3 + jj] = Re[ii * 3] * Rp[jj] + Re[ii * 3 + 1] * Rp[3 + jj] + Re[ii * 3 + 2] * Rp[6 + jj];
        d_markley(Rc, q1);
        d_quat_matrix(q1, Ro);
      } else {
        d_quat_matrix(q0, Ro);
      }
    } else {  // fractional mask: the reference's chain literally
    double rv[3];
    d_so3_log(Rt, rv);
    double rv1[3] = {rv[0], rv[1], rv[2]};
    if (a.diffuse_rot) {
      double Rp[9], Rc[9];
      double Re[9];
      d_so3_exp(rv, Re);
      d_so3_exp(pert, Rp);
      for (int ii = 0; ii < 3; ++ii)
        for (int jj = 0; jj < 3; ++jj)
          Rc[ii * 3 + jj] = Re[ii * 3] * Rp[jj] + Re[ii * 3 + 1] * Rp[3 + jj] + Re[ii * 3 + 2] * Rp[6 + jj];
      d_so3_log(Rc, rv1);  // compose_rotvec, framedipt/data/transforms.py:33-46
    }
    if (has_mask)
      for (int c = 0; c < 3; ++c) rv1[c] = m * rv1[c] + (1 - m) * rv[c];
    d_so3_exp(rv1, Ro);
    }
    // ---- assemble (se3_diffuser.py:26-36): float32 rotation matrix + translation, then tensor_7
    float Rf[9];
    for (int c = 0; c < 9; ++c) Rf[c] = (float)Ro[c];
    if (a.out_rot)
      for (int c = 0; c < 9; ++c) fd_st(a.out_rot + r * 9 + c, Rf[c]);
    double Rd[9], q[4];
    for (int c = 0; c < 9; ++c) Rd[c] = (double)Rf[c];
    d_markley(Rd, q);  // rot_to_quat (rigid_utils.py:208-227) up to sign; consumers are sign-invariant
    if (q[3] < 0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
    float* o = a.rigids_out + r * 7;
    fd_st(o, (float)q[3]); fd_st(o + 1, (float)q[0]); fd_st(o + 2, (float)q[1]); fd_st(o + 3, (float)q[2]);
    fd_st(o + 4, (float)tr_out[0]); fd_st(o + 5, (float)tr_out[1]); fd_st(o + 6, (float)tr_out[2]);
    if (a.kept_rigids)
      for (int c = 0; c < 7; ++c) fd_st(a.kept_rigids + r * 7 + c, o[c]);
    if (a.atom37) {
      const float tf[3] = {o[4], o[5], o[6]};
      d_backbone_residue(r, Rf, tf, a.psi, a.aatype, a.tables, a.atom37, nullptr);
    }
    if (a.trans_traj) {
      const float dm = a.diffuse_mask ? a.diffuse_mask[r] : 1.f, fm = a.traj_fixed[r];
      for (int c = 0; c < 3; ++c) fd_st(a.trans_traj + r * 3 + c, dm * a.pred_rigids[r * 7 + 4 + c] + fm * o[4 + c]);
    }
  }
  if (a.step.cursor) {
    // every block read the cursor before any block can get here; the last one to arrive moves it to the next step (the launches of
    // that step are ordered behind this kernel by the stream / graph).  This is the one launch that writes the cursor.
    __syncthreads();
    if (tid == 0) {
      int32_t* cursor = const_cast<int32_t*>(a.step.cursor);
      const int n_blocks = (int)(gridDim.x * gridDim.y);
      if (atomicAdd(cursor + 1, 1) == n_blocks - 1) {
        cursor[1] = 0;
        atomicAdd(cursor, 1);
      }
    }
  }
}

// out [n_steps,B,N,3]: the draws of steps k_begin .. k_begin + n_steps - 1 for one purpose, through the step kernels' own device function
__global__ void noise_fill_kernel(int B, int N, const uint64_t* __restrict__ keys, uint32_t purpose, int k_begin, long n,
                                  double* __restrict__ out) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const int i = (int)(r % N), b = (int)((r / N) % B);
  const long s = r / ((long)N * B);
  double z[3];
  fd_noise3(keys[b], (uint32_t)i, (uint32_t)(k_begin + s), purpose, z);
  for (int c = 0; c < 3; ++c) out[r * 3 + c] = z[c];
}

// ------------------------------------------------------------------ IGSO(3) rotation score
// 16 lanes per residue split the 1000-term series; float32 sin/cos of omega*(l+1/2), float64 weights and sums
// (the dtype flow torch produces for so3_diffuser.py:68-77,180-191 on the path).  The series weights
// (2l+1) exp(-l(l+1) sigma^2 / 2) depend on the sample only: the block builds them once in LDS for the (at most two)
// samples its residues belong to instead of evaluating a float64 exp per residue and term.
#define RS_L 1000
#define RS_LANES 16
// Terms whose weight exp(-l(l+1) sigma^2 / 2) is exactly 0.0 in float64 (exponent below -760; exp underflows to 0 below
// -745.2) add +-0.0 to both sums: the series is cut there, bit-identical to the 1000-term sum (sigma = 1.5: 28 terms,
// sigma = 0.1: 392 terms).
__device__ __forceinline__ int rs_cut(double sg) {
  const double c = sqrt(1520.0) / sg + 2.0;
  return c < (double)RS_L ? (int)c : RS_L;
}
// Optional epilogue of IpaScore/ScoreNetwork.forward done by otherwise idle lanes of the residue's 16-lane group: the R^3
// score (r3_diffuser.py:387-440 with use_torch=True, scale=True), the tensor_7 / unscaled translations (ipa:557, sn:268), the
// psi normalisation (ipa:355-362) with the fixed-residue merge (sn:259-260), and a contiguous copy of the predicted CA
// positions (the next step's self-conditioning input, experiments/utils.py:361-366).
struct ScoreTail {
  const float* trans;  // [R,3] predicted translations, scaled (nullptr: rotation score only)
  float cs;
  const float* psi_un; int ld_psi;
  const float *gt_psi, *fixed_mask, *t;
  float min_b, max_b;
  float *rigids, *psi, *trans_score, *ca_out;
  // optional last torsion layer (ipa:349-353, Linear(c_s, 2), fp32): psi_un is then computed here from hid [R, ld_hid]
  const float *hid, *torf_w, *torf_b; int ld_hid, c_hid;
  // so3.use_cached_score (so3_diffuser.py:389-396): the score norm is looked up instead of evaluated — table [B][n_omega] = the row
  // of _score_norms at each sample's t, edges [n_omega - 1] = discrete_omega[:-1]; index = torch.bucketize(omega, edges)
  const double *score_table = nullptr, *omega_edges = nullptr; int n_omega = 0;
  // optional backbone atoms of the finished frames (all_atom.compute_backbone; replaces a backbone_kernel launch): the residue's 16
  // lanes take one atom14 atom each
  const int32_t* aatype = nullptr; const BackboneTables* tables = nullptr; float *atom37 = nullptr, *atom14 = nullptr;
  // optional step cursor (FdiptForwardArgs.step_cursor / frame_rows / state_ring; kernels.hpp: FdStep): x_t (tensor_7), sigma, t, the
  // score-table rows and atom37 are then bases of per-step arrays: sigma / t / the table at row k, x_t at the state row, atom37 at the
  // frame's row — or no backbone atoms at all on a step that keeps no frame
  FdStep step = {};
};
template <bool KEPT>  // (the argument of fd_step_rows, nothing else)
__global__ __launch_bounds__(FD_THREADS) void rot_score_kernel(int B, int N, const float* __restrict__ quats_t_, int ld_t,
                                                               const float* __restrict__ quats_0, int ld_0,
                                                               const double* __restrict__ sigma_,
                                                               const float* __restrict__ res_mask,
                                                               double* __restrict__ score, ScoreTail x) {
  __shared__ double wtab[2][RS_L];
  const FdStepRows at = fd_step_rows<KEPT>(x.step);
  const float* __restrict__ quats_t = quats_t_ + at.state_in * B * N * ld_t;
  const double* __restrict__ sigma = sigma_ + at.step * B;
  x.t += at.step * B;
  if (x.score_table) x.score_table += at.step * B * x.n_omega;
  if (at.frame < 0) x.atom37 = x.atom14 = nullptr;
  else if (x.atom37) x.atom37 += at.frame * B * N * 111;
  constexpr int RPB = FD_THREADS / RS_LANES;  // residues per block
  const long total = (long)B * N;
  const long r_first = (long)blockIdx.x * RPB;
  const int b_first = (int)((r_first < total ? r_first : total - 1) / N);
  // a block then spans at most two samples; tiny N evaluates the weights per lane; the cached-score path (x.score_table) has no series
  const bool use_tab = N >= RPB && !x.score_table;
  if (use_tab) {
    const int b1 = b_first + 1 < B ? b_first + 1 : B - 1;
    const double s0 = sigma[b_first], s1 = sigma[b1];
    const int c0 = rs_cut(s0), c1 = (r_first + RPB - 1) / N > b_first ? rs_cut(s1) : 0;
    for (int v = threadIdx.x; v < c0 + c1; v += FD_THREADS) {
      const int which = v >= c0, l = which ? v - c0 : v;
      const double sg = which ? s1 : s0;
      wtab[which][l] = (double)(2 * l + 1) * exp(-(double)l * (double)(l + 1) * sg * sg / 2);
    }
  }
  __syncthreads();
  const long gid = r_first + (threadIdx.x / RS_LANES);
  const int sub = threadIdx.x % RS_LANES;
  const long r = gid < total ? gid : total - 1;
  const int b = (int)(r / N);
  const double* wt = wtab[b - b_first < 2 ? b - b_first : 1];
  const double sg = sigma[b];
  const int lcut = x.score_table ? 0 : rs_cut(sg);  // (cached score: no series)
  float qi[4], q0t[4], rv[3];
  d_invert_quat(quats_0 + r * ld_0, qi);
  d_quat_mul(qi, quats_t + r * ld_t, q0t);
  d_quat_to_rotvec(q0t, rv);
  const float omega = sqrtf(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]) + 1e-6f;
  const float lo = sinf(omega / 2.f), dlo = 0.5f * cosf(omega / 2.f);
  const float den = lo * lo;
  double f = 0, ds = 0;
  for (int l = sub; l < lcut; l += RS_LANES) {
    const double w = use_tab ? wt[l] : (double)(2 * l + 1) * exp(-(double)l * (double)(l + 1) * sg * sg / 2);
    const float lh = (float)l + 0.5f;
    const float arg = omega * lh;
    const float hi = sinf(arg), dhi = lh * cosf(arg);
    f += w * (double)hi / (double)lo;
    const float num = lo * dhi - hi * dlo;
    ds += w * (double)num / (double)den;
  }
#pragma unroll
  for (int o = 1; o < RS_LANES; o <<= 1) {
    f += __shfl_xor(f, o, 64);
    ds += __shfl_xor(ds, o, 64);
  }
  float pa = 0.f, pb = 0.f;
  if (x.hid) {  // the residue's 16 lanes split the two c_hid-long dot products
    const float* h = x.hid + r * x.ld_hid;
    for (int k = sub * 4; k < x.c_hid; k += RS_LANES * 4) {
      const float4 hv = *(const float4*)(h + k), w0 = *(const float4*)(x.torf_w + k), w1 = *(const float4*)(x.torf_w + x.c_hid + k);
      pa = fmaf(hv.w, w0.w, fmaf(hv.z, w0.z, fmaf(hv.y, w0.y, fmaf(hv.x, w0.x, pa))));
      pb = fmaf(hv.w, w1.w, fmaf(hv.z, w1.z, fmaf(hv.y, w1.y, fmaf(hv.x, w1.x, pb))));
    }
#pragma unroll
    for (int o = 1; o < RS_LANES; o <<= 1) {
      pa += __shfl_xor(pa, o, 64);
      pb += __shfl_xor(pb, o, 64);
    }
    pa += x.torf_b[0]; pb += x.torf_b[1];
  }
  if (gid >= total) return;
  if (sub < 3) {
    double sc = ds / (f + 1e-4);
    if (x.score_table) {
      // bucketize (right = False): the number of edges strictly below omega (float32 promoted to float64, as torch does)
      const double om = (double)omega;
      int lo_i = 0, hi_i = x.n_omega - 1;
      while (lo_i < hi_i) {
        const int mid = (lo_i + hi_i) >> 1;
        if (x.omega_edges[mid] < om) lo_i = mid + 1; else hi_i = mid;
      }
      sc = x.score_table[(long)b * x.n_omega + lo_i];
    }
    const double m = res_mask ? (double)res_mask[r] : 1.0;
    score[r * 3 + sub] = sc * (double)rv[sub] / (double)omega * m;
  }
  if (!x.trans) return;
  if (sub >= 3 && sub < 6) {
    const int c = sub - 3;
    const float x0u = x.trans[r * 3 + c] / x.cs;
    x.rigids[r * 7 + 4 + c] = x0u;
    if (x.ca_out) fd_st(x.ca_out + r * 3 + c, x0u);
    const float tt = x.t[b];
    const float mb = tt * x.min_b + 0.5f * (tt * tt) * (x.max_b - x.min_b);
    const float e = expf(-0.5f * mb);
    const float cv = 1.f - expf(-mb);
    const float m = res_mask ? res_mask[r] : 1.f;
    const float xt = quats_t[r * ld_t + 4 + c] * x.cs, x0 = x0u * x.cs;  // rigids_t is tensor_7: translations behind the quaternion
    fd_st(x.trans_score + r * 3 + c, -(xt - e * x0) / cv * m);
  } else if (sub >= 6 && sub < 10) {
    x.rigids[r * 7 + sub - 6] = quats_0[r * ld_0 + sub - 6];
  } else if (sub == 10) {
    const float a = x.hid ? pa : x.psi_un[r * x.ld_psi], bq = x.hid ? pb : x.psi_un[r * x.ld_psi + 1];
    const float dn = sqrtf(fmaxf(a * a + bq * bq, 1e-8f));
    const float dm = 1.f - x.fixed_mask[r];
    x.psi[r * 2] = dm * (a / dn) + (1.f - dm) * x.gt_psi[r * 2];
    x.psi[r * 2 + 1] = dm * (bq / dn) + (1.f - dm) * x.gt_psi[r * 2 + 1];
  }
  if (x.tables && (x.atom37 || x.atom14)) {
    // backbone atoms of the frame just assembled (quaternion = quats_0, translation = trans / cs, psi as lane 10 stores it): lane `sub`
    // builds atom14 atom `sub`; atom37 = zeros except N, CA, C, CB, O (atom14 order N, CA, C, O, CB: all_atom.py:168-174)
    if (x.atom37) {
#pragma unroll
      for (int c = 0; c < 6; ++c) x.atom37[r * 111 + 15 + 6 * sub + c] = 0.f;
    }
    if (sub < 14) {
      const float a = x.hid ? pa : x.psi_un[r * x.ld_psi], bq = x.hid ? pb : x.psi_un[r * x.ld_psi + 1];
      const float dn = sqrtf(fmaxf(a * a + bq * bq, 1e-8f));
      const float dm = 1.f - x.fixed_mask[r];
      const float ps = dm * (a / dn) + (1.f - dm) * x.gt_psi[r * 2], pc = dm * (bq / dn) + (1.f - dm) * x.gt_psi[r * 2 + 1];
      float Rb[9], tbv[3], p3[3];
      d_quat_to_rot(quats_0 + r * ld_0, Rb);
      for (int c = 0; c < 3; ++c) tbv[c] = x.trans[r * 3 + c] / x.cs;
      int aa = x.aatype ? x.aatype[r] : 0;
      if (aa == 20) aa = 0;
      d_backbone_atom(sub, aa, ps, pc, Rb, tbv, x.tables, p3);
      if (x.atom14)
        for (int c = 0; c < 3; ++c) fd_st(x.atom14 + (r * 14 + sub) * 3 + c, p3[c]);
      if (x.atom37 && sub < 5) {
        const int slot = sub == 3 ? 4 : (sub == 4 ? 3 : sub);
        for (int c = 0; c < 3; ++c) fd_st(x.atom37 + r * 111 + slot * 3 + c, p3[c]);
      }
    }
  }
}

// R^3 score, float32 (r3_diffuser.py:387-440 with use_torch=True, scale=True)
__global__ void trans_score_kernel(int B, int N, const float* __restrict__ trans_t, int ld_t,
                                   const float* __restrict__ trans_0, int ld_0, const float* __restrict__ t,
                                   float min_b, float max_b, float cs, const float* __restrict__ res_mask,
                                   float* __restrict__ score) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= (long)B * N) return;
  const float tt = t[r / N];
  const float mb = tt * min_b + 0.5f * (tt * tt) * (max_b - min_b);
  const float e = expf(-0.5f * mb);
  const float cv = 1.f - expf(-mb);
  const float m = res_mask ? res_mask[r] : 1.f;
  for (int c = 0; c < 3; ++c) {
    const float xt = trans_t[r * ld_t + c] * cs, x0 = trans_0[r * ld_0 + c] * cs;
    fd_st(score + r * 3 + c, -(xt - e * x0) / cv * m);
  }
}

// ------------------------------------------------------------------ backbone atoms
// all_atom.py:147-176 -> openfold/utils/feats.py:165-228 -> all_atom.py:108-144.  One thread per residue.
// With a step cursor atom37_ is the base of a per-step array and the frames go to the step's frame row (kernels.hpp: FdStep) — nowhere on
// a step that keeps no frame.
__global__ void backbone_kernel(int n, const float* __restrict__ t7, const float* __restrict__ rot,
                                const float* __restrict__ trans, int ld_trans, const float* __restrict__ psi,
                                const int32_t* __restrict__ aatype, const BackboneTables* __restrict__ tb,
                                float* __restrict__ atom37_, float* __restrict__ atom14, FdStep step) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const long row = fd_step_rows(step).frame;
  if (row < 0) return;
  float* __restrict__ atom37 = atom37_ ? atom37_ + row * n * 111 : atom37_;
  float Rb[9], tbv[3];
  if (rot) {
    for (int c = 0; c < 9; ++c) Rb[c] = rot[r * 9 + c];
    for (int c = 0; c < 3; ++c) tbv[c] = trans[r * ld_trans + c];
  } else {
    d_quat_to_rot(t7 + r * 7, Rb);
    for (int c = 0; c < 3; ++c) tbv[c] = t7[r * 7 + 4 + c];
  }
  d_backbone_residue(r, Rb, tbv, psi, aatype, tb, atom37, atom14);
}

// ------------------------------------------------------------------ small per-residue kernels of the trunk
// Rigid.compose_q_update_vec with update_mask (rigid_utils.py:587-616,1039-1063); quat [n,4] / trans [n,3] in place.
__global__ void compose_q_update_kernel(long n, float* __restrict__ quat, float* __restrict__ trans,
                                        const float* __restrict__ upd, int ld_upd, const float* __restrict__ mask) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const float m = mask ? mask[r] : 1.f;
  float q[4] = {quat[r * 4], quat[r * 4 + 1], quat[r * 4 + 2], quat[r * 4 + 3]};
  float dq[4], R[9], dt[3];
  d_quat_mul_vec(q, upd + r * ld_upd, dq);
  d_quat_to_rot(q, R);
  d_rot_vec(R, upd + r * ld_upd + 3, dt);
  float nq[4];
  for (int c = 0; c < 4; ++c) nq[c] = q[c] + dq[c] * m;
  const float nrm = sqrtf(nq[0] * nq[0] + nq[1] * nq[1] + nq[2] * nq[2] + nq[3] * nq[3]);
  for (int c = 0; c < 4; ++c) quat[r * 4 + c] = nq[c] / nrm;
  for (int c = 0; c < 3; ++c) fd_st(trans + r * 3 + c, trans[r * 3 + c] + dt[c] * m);
}

int fd_compose_q_update(long n, float* quat, float* trans, const float* upd, int ld_upd, const float* mask,
                        hipStream_t st) {
  hipLaunchKernelGGL(compose_q_update_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, n, quat, trans, upd, ld_upd, mask);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}

// IpaScore.forward prologue (ipa_pytorch.py:516-524): split tensor_7, scale translations; diffuse_mask = (1-fixed)*res.
__global__ void split_rigids_kernel(long n, const float* __restrict__ t7_, float cs, const float* __restrict__ res_mask,
                                    const float* __restrict__ fixed_mask, float* __restrict__ quat,
                                    float* __restrict__ trans, float* __restrict__ diffuse_mask, FdStep step) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const float* __restrict__ t7 = t7_ + fd_step_rows(step).state_in * n * 7;  // (step cursor: the state row of x_t)
  for (int c = 0; c < 4; ++c) quat[r * 4 + c] = t7[r * 7 + c];
  for (int c = 0; c < 3; ++c) fd_st(trans + r * 3 + c, t7[r * 7 + 4 + c] * cs);
  diffuse_mask[r] = (1.f - fixed_mask[r]) * res_mask[r];
}
int fd_split_rigids(long n, const float* t7, float cs, const float* res_mask, const float* fixed_mask, float* quat,
                    float* trans, float* dmask, FdStep step, hipStream_t st) {
  hipLaunchKernelGGL(split_rigids_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, n, t7, cs, res_mask, fixed_mask, quat, trans, dmask, step);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}

// Epilogue of IpaScore/ScoreNetwork.forward: unscale translations (ipa:557), tensor_7 (sn:268), psi normalisation
// (ipa:355-362) and the fixed-residue psi merge (sn:259-260).
__global__ void finish_kernel(long n, const float* __restrict__ quat, const float* __restrict__ trans, float cs,
                              const float* __restrict__ psi_un, int ld_psi, const float* __restrict__ gt_psi,
                              const float* __restrict__ fixed_mask, float* __restrict__ rigids,
                              float* __restrict__ psi) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  for (int c = 0; c < 4; ++c) rigids[r * 7 + c] = quat[r * 4 + c];
  for (int c = 0; c < 3; ++c) fd_st(rigids + r * 7 + 4 + c, trans[r * 3 + c] / cs);
  const float a = psi_un[r * ld_psi], bq = psi_un[r * ld_psi + 1];
  const float den = sqrtf(fmaxf(a * a + bq * bq, 1e-8f));
  const float dm = 1.f - fixed_mask[r];
  psi[r * 2] = dm * (a / den) + (1.f - dm) * gt_psi[r * 2];
  psi[r * 2 + 1] = dm * (bq / den) + (1.f - dm) * gt_psi[r * 2 + 1];
}
int fd_finish(long n, const float* quat, const float* trans, float cs, const float* psi_un, int ld_psi,
              const float* gt_psi, const float* fixed_mask, float* rigids, float* psi, hipStream_t st) {
  hipLaunchKernelGGL(finish_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, n, quat, trans, cs, psi_un, ld_psi, gt_psi,
                     fixed_mask, rigids, psi);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}

// Node / pair first-layer input features (score_network.py:152-182): pte = [aatype one-hot?, t-embed, fixed_mask];
// node_feat = [pte, index-embed] zero-padded to ld_node; pte zero-padded to ld_pte.
struct FeatsExtra {  // optional work folded into the feature kernel's launch (nullptr to skip each part)
  const float *t7, *res_mask; float cs; float *quat, *trans, *dmask;  // split of x_t into quaternion / scaled translation
  const float *w1i, *w1j, *b1; int cz; float *pi, *pj;              // per-residue halves of the first edge-embedder layer
  FdStep step;  // optional step cursor: t_emb and t7 are bases of per-step arrays, read at row k / the state row of x_t
};
template <bool KEPT>  // (the argument of fd_step_rows, nothing else)
__global__ void build_feats_kernel(int B, int N, int use_aatype, int E, const int32_t* __restrict__ aatype,
                                   const float* __restrict__ t_emb_, const float* __restrict__ t_emb_eps,
                                   const float* __restrict__ fixed_mask, const float* __restrict__ idx_emb,
                                   float* __restrict__ node_feat, int ld_node, float* __restrict__ pte, int ld_pte,
                                   FeatsExtra x) {
  __shared__ float pte_s[128];
  const FdStepRows at = fd_step_rows<KEPT>(x.step);
  const float* __restrict__ t_emb = t_emb_ + at.step * B * E;
  if (x.t7) x.t7 += at.state_in * B * N * 7;
  const long r = blockIdx.x;
  const int b = (int)(r / N);
  const float fm = fixed_mask[r];
  const int d1 = E + 1 + (use_aatype ? 21 : 0);
  if (x.t7 && threadIdx.x < 8) {  // IpaScore.forward prologue (ipa_pytorch.py:516-524), as split_rigids_kernel
    const int c = threadIdx.x;
    if (c < 4) x.quat[r * 4 + c] = x.t7[r * 7 + c];
    else if (c < 7) x.trans[r * 3 + c - 4] = x.t7[r * 7 + c] * x.cs;
    else x.dmask[r] = (1.f - fm) * x.res_mask[r];
  }
  for (int c = threadIdx.x; c < ld_node; c += blockDim.x) {
    float v = 0.f;
    int cc = c;
    if (use_aatype) {
      if (c < 21) { v = (aatype[r] == c) ? 1.f : 0.f; cc = -1; } else cc = c - 21;
    }
    if (cc >= 0) {
      if (cc < E) v = (use_aatype && fm != 0.f) ? t_emb_eps[cc] : t_emb[b * E + cc];
      else if (cc == E) v = fm;
      else if (cc < 2 * E + 1) v = idx_emb[r * E + (cc - E - 1)];
    }
    node_feat[r * ld_node + c] = v;
    if (c < ld_pte) {
      pte[r * ld_pte + c] = c < d1 ? v : 0.f;
      if (x.pi && c < 128) pte_s[c] = c < d1 ? v : 0.f;
    }
  }
  if (!x.pi) return;
  // first edge-embedder layer, per-residue halves (score_network.py:173-180: the cross-concatenated pair feature's i and j
  // parts are each a [c_z, d1] product with this residue's feature row): column c of both, fp32
  __syncthreads();
  for (int c = threadIdx.x; c < x.cz; c += blockDim.x) {
    const float4* wi = (const float4*)(x.w1i + (long)c * ld_pte);
    const float4* wj = (const float4*)(x.w1j + (long)c * ld_pte);
    float si = 0.f, sj = 0.f;
    for (int k = 0; k < ld_pte / 4; ++k) {
      const float4 a = wi[k], bq = wj[k];
      const float p0 = pte_s[4 * k], p1 = pte_s[4 * k + 1], p2 = pte_s[4 * k + 2], p3 = pte_s[4 * k + 3];
      si = fmaf(p3, a.w, fmaf(p2, a.z, fmaf(p1, a.y, fmaf(p0, a.x, si))));
      sj = fmaf(p3, bq.w, fmaf(p2, bq.z, fmaf(p1, bq.y, fmaf(p0, bq.x, sj))));
    }
    x.pi[r * x.cz + c] = si + x.b1[c];
    x.pj[r * x.cz + c] = sj;
  }
}
int fd_build_feats(int B, int N, int use_aatype, int E, const int32_t* aatype, const float* t_emb, const float* t_emb_eps,
                   const float* fixed_mask, const float* idx_emb, float* node_feat, int ld_node, float* pte, int ld_pte,
                   const float* t7, const float* res_mask, float cs, float* quat, float* trans, float* dmask, const float* w1i,
                   const float* w1j, const float* b1, int cz, float* pi, float* pj, FdStep step, hipStream_t st) {
  if (use_aatype && (!aatype || !t_emb_eps)) return FDIPT_EINVAL;
  if (pi && (ld_pte > 128 || (ld_pte & 3))) return FDIPT_EINVAL;
  FeatsExtra x = {t7, res_mask, cs, quat, trans, dmask, w1i, w1j, b1, cz, pi, pj, step};
  const auto kernel = step.kept() ? build_feats_kernel<true> : build_feats_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(B * N), dim3(128), 0, st, B, N, use_aatype, E, aatype, t_emb, t_emb_eps,
                     fixed_mask, idx_emb, node_feat, ld_node, pte, ld_pte, x);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}

int fd_rot_score(int B, int N, const float* qt, int ld_t, const float* q0, int ld_0, const double* sigma,
                 const float* res_mask, double* score, hipStream_t st) {
  ScoreTail x = {};
  hipLaunchKernelGGL(rot_score_kernel<false>, dim3(cdiv((long)B * N, FD_THREADS / RS_LANES)), dim3(FD_THREADS), 0, st, B, N, qt, ld_t, q0,
                     ld_0, sigma, res_mask, score, x);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
// rotation score + translation score + finish (tensor_7, psi, self-conditioning CA copy) in one launch; rigids_t is tensor_7
int fd_score_tail(int B, int N, const float* rigids_t, const float* quat, const float* trans, float cs, const float* psi_un,
                  int ld_psi, const float* gt_psi, const float* fixed_mask, const float* res_mask, const double* sigma,
                  const float* t, float min_b, float max_b, float* rigids, float* psi, double* rot_score, float* trans_score,
                  float* ca_out, const float* hid, int ld_hid, int c_hid, const float* torf_w, const float* torf_b,
                  const double* score_table, const double* omega_edges, int n_omega, const int32_t* aatype, const void* bb_tables,
                  float* atom37, float* atom14, FdStep step, hipStream_t st) {
  if (hid && ((c_hid & 3) || (ld_hid & 3))) return FDIPT_EINVAL;
  if (score_table && (!omega_edges || n_omega < 2)) return FDIPT_EINVAL;
  if ((atom37 || atom14) && !bb_tables) return FDIPT_EINVAL;
  ScoreTail x = {trans, cs, psi_un, ld_psi, gt_psi, fixed_mask, t, min_b, max_b, rigids, psi, trans_score, ca_out,
                 hid, torf_w, torf_b, ld_hid, c_hid, score_table, omega_edges, n_omega, aatype, (const BackboneTables*)bb_tables, atom37, atom14,
                 step};
  const auto kernel = step.kept() ? rot_score_kernel<true> : rot_score_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(cdiv((long)B * N, FD_THREADS / RS_LANES)), dim3(FD_THREADS), 0, st, B, N, rigids_t, 7,
                     quat, 4, sigma, res_mask, rot_score, x);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
int fd_trans_score(int B, int N, const float* tt, int ld_t, const float* t0, int ld_0, const float* t, float min_b,
                   float max_b, float cs, const float* res_mask, float* score, hipStream_t st) {
  hipLaunchKernelGGL(trans_score_kernel, dim3(cdiv((long)B * N, 256)), dim3(256), 0, st, B, N, tt, ld_t, t0, ld_0, t, min_b,
                     max_b, cs, res_mask, score);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
int fd_backbone(int n, const float* t7, const float* rot, const float* trans, int ld_trans, const float* psi,
                const int32_t* aatype, const void* tables, float* atom37, float* atom14, hipStream_t st, FdStep step) {
  // kept-frame loop: tensor_7 frames into the map's row of atom37 and nothing else (a step that keeps no frame builds nothing).  rot is
  // refused on purpose: the former kept kernel had no such input, the merged one would read it (no caller passes it).
  if (step.frame_rows && (!t7 || rot || !atom37 || atom14)) return FDIPT_EINVAL;
  hipLaunchKernelGGL(backbone_kernel, dim3(cdiv(n, 64)), dim3(64), 0, st, n, t7, rot, trans, ld_trans, psi, aatype,
                     (const BackboneTables*)tables, atom37, atom14, step);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}

// ------------------------------------------------------------------ elementwise exports (a8)
#define FD_EW_KERNEL(name, ...)                                                                  \
  __global__ void name##_k(int n, const float* __restrict__ x, const float* __restrict__ y,     \
                           float* __restrict__ o, float* __restrict__ o2) {                     \
    const int r = blockIdx.x * blockDim.x + threadIdx.x;                                        \
    if (r >= n) return;                                                                         \
    __VA_ARGS__                                                                                 \
  }
FD_EW_KERNEL(quat_to_rot, d_quat_to_rot(x + r * 4, o + r * 9);)
FD_EW_KERNEL(quat_multiply, d_quat_mul(x + r * 4, y + r * 4, o + r * 4);)
FD_EW_KERNEL(quat_multiply_by_vec, d_quat_mul_vec(x + r * 4, y + r * 3, o + r * 4);)
FD_EW_KERNEL(invert_quat, d_invert_quat(x + r * 4, o + r * 4);)
FD_EW_KERNEL(quat_to_rotvec, d_quat_to_rotvec(x + r * 4, o + r * 3);)
FD_EW_KERNEL(rigid_apply, float R[9], p[3]; d_quat_to_rot(x + r * 7, R); d_rot_vec(R, y + r * 3, p);
             for (int c = 0; c < 3; ++c) o[r * 3 + c] = p[c] + x[r * 7 + 4 + c];)
FD_EW_KERNEL(rigid_invert_apply, float R[9], Rt[9], d[3]; d_quat_to_rot(x + r * 7, R);
             for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Rt[i * 3 + j] = R[j * 3 + i];
             for (int c = 0; c < 3; ++c) d[c] = y[r * 3 + c] - x[r * 7 + 4 + c];
             d_rot_vec(Rt, d, o + r * 3);)
FD_EW_KERNEL(rigid_compose, float R1[9], R2[9]; d_quat_to_rot(x + r * 7, R1); d_quat_to_rot(y + r * 7, R2);
             d_compose(R1, x + r * 7 + 4, R2, y + r * 7 + 4, o + r * 9, o2 + r * 3);)
FD_EW_KERNEL(rigid_invert, float R[9], Rt[9], p[3]; d_quat_to_rot(x + r * 7, R);
             for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Rt[i * 3 + j] = R[j * 3 + i];
             d_rot_vec(Rt, x + r * 7 + 4, p);
             for (int c = 0; c < 9; ++c) o[r * 9 + c] = Rt[c];
             for (int c = 0; c < 3; ++c) o2[r * 3 + c] = -p[c];)
FD_EW_KERNEL(rot_to_quat, double m[9], q[4]; for (int c = 0; c < 9; ++c) m[c] = (double)x[r * 9 + c]; d_markley(m, q);
             if (q[3] < 0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
             o[r * 4] = (float)q[3]; o[r * 4 + 1] = (float)q[0]; o[r * 4 + 2] = (float)q[1]; o[r * 4 + 3] = (float)q[2];)

__global__ void so3_exp_k(int n, const double* __restrict__ rv, double* __restrict__ R) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) d_so3_exp(rv + r * 3, R + r * 9);
}
__global__ void so3_log_k(int n, const double* __restrict__ R, double* __restrict__ rv) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) d_so3_log(R + r * 9, rv + r * 3);
}
// Rigid.from_3_points (openfold/utils/rigid_utils.py:1233-1275): Gram-Schmidt frame, columns e0 | e1 | e2, float32 in the
// reference's evaluation order
__global__ void from_3_points_k(int n, const float* __restrict__ pa, const float* __restrict__ po, const float* __restrict__ pc,
                                float eps, float* __restrict__ rot) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  float e0[3], e1[3];
  for (int c = 0; c < 3; ++c) { e0[c] = po[r * 3 + c] - pa[r * 3 + c]; e1[c] = pc[r * 3 + c] - po[r * 3 + c]; }
  float dn = sqrtf(((e0[0] * e0[0] + e0[1] * e0[1]) + e0[2] * e0[2]) + eps);
  for (int c = 0; c < 3; ++c) e0[c] = e0[c] / dn;
  const float dot = (e0[0] * e1[0] + e0[1] * e1[1]) + e0[2] * e1[2];
  for (int c = 0; c < 3; ++c) e1[c] = e1[c] - e0[c] * dot;
  dn = sqrtf(((e1[0] * e1[0] + e1[1] * e1[1]) + e1[2] * e1[2]) + eps);
  for (int c = 0; c < 3; ++c) e1[c] = e1[c] / dn;
  const float e2[3] = {e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]};
  for (int c = 0; c < 3; ++c) { rot[r * 9 + 3 * c] = e0[c]; rot[r * 9 + 3 * c + 1] = e1[c]; rot[r * 9 + 3 * c + 2] = e2[c]; }
}

// ---- SO(3) exp / log of the geomstats fork (framedipt/diffusion/so3_utils.py), float64 here (the reference evaluates them in
// the dtype of its inputs)
// omega (:103-117): rotation angle from the trace shrunk by (1 - eps)
__device__ __forceinline__ double d_gs_omega(const double* R, double eps) {
  const double tr = (R[0] + R[4] + R[8]) * (1.0 - eps);
  return acos((tr - 1.0) / 2.0);
}
// rot_mat_from_axis_angle_by_exp_map (:90-100): matrix exponential of the skew matrix of v (:4-22) = Rodrigues' formula
__device__ __forceinline__ void d_gs_exp(const double* v, double* R) {
  const double th2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], th = sqrt(th2);
  // sin(th)/th and (1 - cos th)/th^2 with their series near 0
  const double a = th < 1e-4 ? 1.0 - th2 / 6.0 : sin(th) / th;
  const double b = th < 1e-4 ? 0.5 - th2 / 24.0 : (1.0 - cos(th)) / th2;
  const double K[9] = {0, -v[2], v[1], v[2], 0, -v[0], -v[1], v[0], 0};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double k2 = 0;
      for (int k = 0; k < 3; ++k) k2 += K[i * 3 + k] * K[k * 3 + j];
      R[i * 3 + j] = (i == j ? 1.0 : 0.0) + a * K[i * 3 + j] + b * k2;
    }
}
__device__ __forceinline__ bool d_isclose(double x, double y, double atol) { return fabs(x - y) <= atol + 1e-5 * fabs(y); }
// regularize (:193-231): angle folded into [0, pi]
__device__ __forceinline__ void d_gs_regularize(double* p) {
  const double PI = 3.14159265358979323846;
  const double th = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
  const double k = floor(th / 2.0 / PI), ang = th - 2.0 * k * PI;
  const bool zero = d_isclose(th, 0.0, 1e-8);
  const double th_eps = zero ? 1.0 : th;
  const double na = ang <= PI ? ang : 2.0 * PI - ang;
  double ratio = zero ? 1.0 : na / th_eps;
  if (ang > PI) ratio = -ratio;
  for (int c = 0; c < 3; ++c) p[c] *= ratio;
}
// rotation_vector_from_matrix (:120-190)
__device__ __forceinline__ void d_gs_log(const double* R, double* rv) {
  const double PI = 3.14159265358979323846;
  const double ang = d_gs_omega(R, 1e-4);
  // vee(R - R^T) (:25-40)
  double np_[3] = {-(R[5] - R[7]), R[2] - R[6], -(R[1] - R[3])};
  const double m0 = d_isclose(ang, 0.0, 1e-8) ? 1.0 : 0.0, mpi = d_isclose(ang, PI, 1e-2) ? 1.0 : 0.0, me = (1.0 - m0) * (1.0 - mpi);
  const double num = 0.5 * m0 + ang * me, den = (1.0 - ang * ang / 6.0) * m0 + 2.0 * sin(ang) * me + mpi;
  for (int c = 0; c < 3; ++c) np_[c] = np_[c] * num / den;
  double vo[9];
  for (int i = 0; i < 9; ++i) vo[i] = 0.5 * ((i % 4 == 0 ? 1.0 : 0.0) + R[i]);
  for (int i = 0; i < 3; ++i) vo[4 * i] = fmax(0.0, vo[4 * i]);
  int best = 0;
  double bn = -1.0;
  for (int i = 0; i < 3; ++i) {
    const double nl = sqrt(vo[3 * i] * vo[3 * i] + vo[3 * i + 1] * vo[3 * i + 1] + vo[3 * i + 2] * vo[3 * i + 2]);
    if (nl > bn) { bn = nl; best = i; }  // (first maximum, as torch.argmax)
  }
  for (int c = 0; c < 3; ++c) {
    const double sl = vo[3 * best + c], sg = sl > 0 ? 1.0 : (sl < 0 ? -1.0 : 0.0);
    rv[c] = np_[c] + mpi * (ang * sg * sqrt(vo[4 * c]));
  }
  d_gs_regularize(rv);
}
__global__ void gs_exp_k(int n, const double* __restrict__ rv, double* __restrict__ R) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) d_gs_exp(rv + r * 3, R + r * 9);
}
__global__ void gs_log_k(int n, const double* __restrict__ R, double* __restrict__ rv) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) d_gs_log(R + r * 9, rv + r * 3);
}
__global__ void gs_omega_k(int n, const double* __restrict__ R, double eps, double* __restrict__ out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) out[r] = d_gs_omega(R + r * 9, eps);
}

__global__ void cqu_t7_k(int n, const float* __restrict__ t7, const float* __restrict__ upd,
                         const float* __restrict__ mask, float* __restrict__ out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const float m = mask ? mask[r] : 1.f;
  const float* q = t7 + r * 7;
  float dq[4], R[9], dt[3], nq[4];
  d_quat_mul_vec(q, upd + r * 6, dq);
  d_quat_to_rot(q, R);
  d_rot_vec(R, upd + r * 6 + 3, dt);
  for (int c = 0; c < 4; ++c) nq[c] = q[c] + dq[c] * m;
  const float nrm = sqrtf(nq[0] * nq[0] + nq[1] * nq[1] + nq[2] * nq[2] + nq[3] * nq[3]);
  for (int c = 0; c < 4; ++c) out[r * 7 + c] = nq[c] / nrm;
  for (int c = 0; c < 3; ++c) out[r * 7 + 4 + c] = q[4 + c] + dt[c] * m;
}

// ------------------------------------------------------------------ the reverse step's one launcher
// Validation, block size and launch for every exported reverse-step entry; the entries below only marshal their arguments onto it.
// gen: the noise comes from keys (tape pointers must be NULL), otherwise from the tape.  indexed: the cursor entries (rigids_t ==
// rigids_out == the state's base; the time comes from t_table).
static int reverse_launch(ReverseArgs a, bool gen, bool indexed, hipStream_t st) {
  if (a.B <= 0 || a.N <= 0) return FDIPT_OK;
  if (!a.rigids_t || !a.rot_score || !a.trans_score || !a.rigids_out) return FDIPT_EINVAL;
  if (gen ? (!a.noise_keys || a.noise_step < 0 || a.z_rot || a.z_trans) : (!a.z_rot || !a.z_trans)) return FDIPT_EINVAL;
  if (indexed ? (!a.step.cursor || !a.t_table) : !(a.t >= 0 && a.t <= 1)) return FDIPT_EINVAL;
  if (a.atom37 && (!a.psi || !a.tables || (!indexed && a.rigids_out == a.rigids_t))) return FDIPT_EINVAL;
  if (a.trans_traj && (!a.pred_rigids || !a.traj_fixed)) return FDIPT_EINVAL;
  if (!a.step.valid() || (a.kept_rigids && !a.step.frame_rows)) return FDIPT_EINVAL;
  a.rpb = !indexed && a.rigids_out == a.rigids_t ? a.N : 64;  // in place: the whole sample in one block
  const dim3 grid(cdiv(a.N, a.rpb), a.B);
  const bool kept = a.step.kept();
  const auto kernel = gen ? (kept ? reverse_step_kernel<true, true> : reverse_step_kernel<true, false>)
                          : (kept ? reverse_step_kernel<false, true> : reverse_step_kernel<false, false>);
  hipLaunchKernelGGL(kernel, grid, dim3(FD_THREADS), 0, st, a);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
// the entries that take their arguments one by one (fdipt_se3_reverse_step, _atoms, _traj, _traj_gen)
static int reverse_flat(int B, int N, const float* rigids_t, const double* rot_score, const float* trans_score, const float* diffuse_mask,
                        const double* z_rot, const double* z_trans, const uint64_t* noise_keys, int noise_step, double t, double dt,
                        double noise_scale, int center, int diffuse_rot, int diffuse_trans, double so3_min_sigma, double so3_max_sigma,
                        double r3_min_b, double r3_max_b, double coordinate_scaling, float* rigids_out, float* out_rot, const float* psi,
                        const int32_t* aatype, const void* tables, float* atom37, const float* pred_rigids, const float* traj_fixed_mask,
                        float* trans_traj, bool gen, fdipt_stream_t stream) {
  ReverseArgs a;
  a.B = B; a.N = N;
  a.rigids_t = rigids_t; a.rot_score = rot_score; a.trans_score = trans_score; a.diffuse_mask = diffuse_mask;
  a.z_rot = z_rot; a.z_trans = z_trans; a.noise_keys = noise_keys; a.noise_step = noise_step;
  a.t = t; a.dt = dt; a.noise_scale = noise_scale;
  a.center = center; a.diffuse_rot = diffuse_rot; a.diffuse_trans = diffuse_trans;
  a.so3_min_sigma = so3_min_sigma; a.so3_max_sigma = so3_max_sigma; a.r3_min_b = r3_min_b; a.r3_max_b = r3_max_b; a.cs = coordinate_scaling;
  a.rigids_out = rigids_out; a.out_rot = out_rot;
  a.psi = psi; a.aatype = aatype; a.tables = (const BackboneTables*)tables; a.atom37 = atom37;
  a.pred_rigids = pred_rigids; a.traj_fixed = traj_fixed_mask; a.trans_traj = trans_traj;
  return reverse_launch(a, gen, false, (hipStream_t)stream);
}
// the cursor entries (fdipt_se3_reverse_step_indexed, _indexed_gen): noise_keys is the _gen entry's, whose x carries no tape
static int reverse_indexed(const FdiptReverseIndexed* x, const uint64_t* noise_keys, bool gen, fdipt_stream_t stream) {
  if (!x) return FDIPT_EINVAL;
  ReverseArgs a;
  a.B = x->B; a.N = x->N;
  a.rigids_t = a.rigids_out = x->rigid_traj; a.rot_score = x->rot_score; a.trans_score = x->trans_score; a.diffuse_mask = x->diffuse_mask;
  a.z_rot = x->z_rot; a.z_trans = x->z_trans; a.noise_keys = noise_keys;
  a.dt = x->dt; a.noise_scale = x->noise_scale;
  a.center = x->center; a.diffuse_rot = x->diffuse_rot; a.diffuse_trans = x->diffuse_trans;
  a.so3_min_sigma = x->so3_min_sigma; a.so3_max_sigma = x->so3_max_sigma; a.r3_min_b = x->r3_min_b; a.r3_max_b = x->r3_max_b;
  a.cs = x->coordinate_scaling;
  a.psi = x->psi; a.aatype = x->aatype; a.tables = (const BackboneTables*)x->bb_tables; a.atom37 = x->prot_traj;
  a.pred_rigids = x->pred_rigids; a.traj_fixed = x->traj_fixed_mask; a.trans_traj = x->trans_traj;
  a.step = FdStep{x->step_cursor, x->frame_rows, x->state_ring};
  a.t_table = x->t_table; a.kept_rigids = x->kept_rigids;
  return reverse_launch(a, gen, true, (hipStream_t)stream);
}

#define FD_EW_EXPORT(name, X, Y, O, O2)                                                        \
  if (n <= 0) return FDIPT_OK;                                                                 \
  if (!(X) || !(O)) return FDIPT_EINVAL;                                                       \
  hipLaunchKernelGGL(name##_k, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)s, n, X, Y, O, O2); \
  FD_CHECK_LAUNCH();                                                                           \
  return FDIPT_OK;

extern "C" {
int fdipt_quat_to_rot(int n, const float* quat, float* rot, fdipt_stream_t s) { FD_EW_EXPORT(quat_to_rot, quat, nullptr, rot, nullptr) }
int fdipt_rot_to_quat(int n, const float* rot, float* quat, fdipt_stream_t s) { FD_EW_EXPORT(rot_to_quat, rot, nullptr, quat, nullptr) }
int fdipt_quat_multiply(int n, const float* q1, const float* q2, float* out, fdipt_stream_t s) { FD_EW_EXPORT(quat_multiply, q1, q2, out, nullptr) }
int fdipt_quat_multiply_by_vec(int n, const float* q, const float* v, float* out, fdipt_stream_t s) { FD_EW_EXPORT(quat_multiply_by_vec, q, v, out, nullptr) }
int fdipt_invert_quat(int n, const float* q, float* out, fdipt_stream_t s) { FD_EW_EXPORT(invert_quat, q, nullptr, out, nullptr) }
int fdipt_rigid_apply(int n, const float* t7, const float* pts, float* out, fdipt_stream_t s) { FD_EW_EXPORT(rigid_apply, t7, pts, out, nullptr) }
int fdipt_rigid_invert_apply(int n, const float* t7, const float* pts, float* out, fdipt_stream_t s) { FD_EW_EXPORT(rigid_invert_apply, t7, pts, out, nullptr) }
int fdipt_rigid_compose(int n, const float* a, const float* b, float* out_rot, float* out_trans, fdipt_stream_t s) { FD_EW_EXPORT(rigid_compose, a, b, out_rot, out_trans) }
int fdipt_rigid_invert(int n, const float* t7, float* out_rot, float* out_trans, fdipt_stream_t s) { FD_EW_EXPORT(rigid_invert, t7, nullptr, out_rot, out_trans) }
int fdipt_quat_to_rotvec(int n, const float* q, float* rotvec, fdipt_stream_t s) { FD_EW_EXPORT(quat_to_rotvec, q, nullptr, rotvec, nullptr) }

int fdipt_rigid_compose_q_update(int n, const float* t7, const float* upd6, const float* mask, float* out_t7,
                                 fdipt_stream_t s) {
  if (n <= 0) return FDIPT_OK;
  if (!t7 || !upd6 || !out_t7) return FDIPT_EINVAL;
  hipLaunchKernelGGL(cqu_t7_k, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)s, n, t7, upd6, mask, out_t7);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
int fdipt_rigid_from_3_points(int n, const float* p_neg_x_axis, const float* origin, const float* p_xy_plane, float eps, float* rot,
                              fdipt_stream_t s) {
  if (n <= 0) return FDIPT_OK;
  if (!p_neg_x_axis || !origin || !p_xy_plane || !rot) return FDIPT_EINVAL;
  hipLaunchKernelGGL(from_3_points_k, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)s, n, p_neg_x_axis, origin, p_xy_plane, eps, rot);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
int fdipt_so3_exp_geomstats(int n, const double* rotvec, double* rot, fdipt_stream_t s) {
  if (n <= 0) return FDIPT_OK;
  if (!rotvec || !rot) return FDIPT_EINVAL;
  hipLaunchKernelGGL(gs_exp_k, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)s, n, rotvec, rot);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
int fdipt_so3_log_geomstats(int n, const double* rot, double* rotvec, fdipt_stream_t s) {
  if (n <= 0) return FDIPT_OK;
  if (!rotvec || !rot) return FDIPT_EINVAL;
  hipLaunchKernelGGL(gs_log_k, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)s, n, rot, rotvec);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
int fdipt_so3_omega(int n, const double* rot, double eps, double* angle, fdipt_stream_t s) {
  if (n <= 0) return FDIPT_OK;
  if (!angle || !rot) return FDIPT_EINVAL;
  hipLaunchKernelGGL(gs_omega_k, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)s, n, rot, eps, angle);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
int fdipt_so3_exp(int n, const double* rotvec, double* rot, fdipt_stream_t s) {
  if (n <= 0) return FDIPT_OK;
  if (!rotvec || !rot) return FDIPT_EINVAL;
  hipLaunchKernelGGL(so3_exp_k, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)s, n, rotvec, rot);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
int fdipt_so3_log(int n, const double* rot, double* rotvec, fdipt_stream_t s) {
  if (n <= 0) return FDIPT_OK;
  if (!rot || !rotvec) return FDIPT_EINVAL;
  hipLaunchKernelGGL(so3_log_k, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)s, n, rot, rotvec);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}

int fdipt_se3_reverse_step_traj(int B, int N, const float* rigids_t, const double* rot_score, const float* trans_score,
                                const float* diffuse_mask, const double* z_rot, const double* z_trans, double t, double dt,
                                double noise_scale, int center, int diffuse_rot, int diffuse_trans, double so3_min_sigma,
                                double so3_max_sigma, double r3_min_b, double r3_max_b, double coordinate_scaling,
                                float* rigids_out, float* out_rot, const float* psi, const int32_t* aatype,
                                const void* tables, float* atom37, const float* pred_rigids, const float* traj_fixed_mask,
                                float* trans_traj, fdipt_stream_t stream) {
  return reverse_flat(B, N, rigids_t, rot_score, trans_score, diffuse_mask, z_rot, z_trans, nullptr, 0, t, dt, noise_scale, center,
                      diffuse_rot, diffuse_trans, so3_min_sigma, so3_max_sigma, r3_min_b, r3_max_b, coordinate_scaling, rigids_out, out_rot,
                      psi, aatype, tables, atom37, pred_rigids, traj_fixed_mask, trans_traj, false, stream);
}
int fdipt_se3_reverse_step_atoms(int B, int N, const float* rigids_t, const double* rot_score, const float* trans_score,
                                 const float* diffuse_mask, const double* z_rot, const double* z_trans, double t, double dt,
                                 double noise_scale, int center, int diffuse_rot, int diffuse_trans, double so3_min_sigma,
                                 double so3_max_sigma, double r3_min_b, double r3_max_b, double coordinate_scaling,
                                 float* rigids_out, float* out_rot, const float* psi, const int32_t* aatype,
                                 const void* tables, float* atom37, fdipt_stream_t stream) {
  return reverse_flat(B, N, rigids_t, rot_score, trans_score, diffuse_mask, z_rot, z_trans, nullptr, 0, t, dt, noise_scale, center,
                      diffuse_rot, diffuse_trans, so3_min_sigma, so3_max_sigma, r3_min_b, r3_max_b, coordinate_scaling, rigids_out, out_rot,
                      psi, aatype, tables, atom37, nullptr, nullptr, nullptr, false, stream);
}
int fdipt_se3_reverse_step(int B, int N, const float* rigids_t, const double* rot_score, const float* trans_score,
                           const float* diffuse_mask, const double* z_rot, const double* z_trans, double t, double dt,
                           double noise_scale, int center, int diffuse_rot, int diffuse_trans, double so3_min_sigma,
                           double so3_max_sigma, double r3_min_b, double r3_max_b, double coordinate_scaling,
                           float* rigids_out, float* out_rot, fdipt_stream_t stream) {
  return reverse_flat(B, N, rigids_t, rot_score, trans_score, diffuse_mask, z_rot, z_trans, nullptr, 0, t, dt, noise_scale, center,
                      diffuse_rot, diffuse_trans, so3_min_sigma, so3_max_sigma, r3_min_b, r3_max_b, coordinate_scaling, rigids_out, out_rot,
                      nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, false, stream);
}
// noise="device": the same launches with the samples' noise keys in place of the tape rows (reverse_step_kernel<true, .>)
int fdipt_se3_reverse_step_traj_gen(int B, int N, const float* rigids_t, const double* rot_score, const float* trans_score,
                                    const float* diffuse_mask, const uint64_t* noise_keys, int step, double t, double dt,
                                    double noise_scale, int center, int diffuse_rot, int diffuse_trans, double so3_min_sigma,
                                    double so3_max_sigma, double r3_min_b, double r3_max_b, double coordinate_scaling,
                                    float* rigids_out, float* out_rot, const float* psi, const int32_t* aatype,
                                    const void* tables, float* atom37, const float* pred_rigids, const float* traj_fixed_mask,
                                    float* trans_traj, fdipt_stream_t stream) {
  return reverse_flat(B, N, rigids_t, rot_score, trans_score, diffuse_mask, nullptr, nullptr, noise_keys, step, t, dt, noise_scale, center,
                      diffuse_rot, diffuse_trans, so3_min_sigma, so3_max_sigma, r3_min_b, r3_max_b, coordinate_scaling, rigids_out, out_rot,
                      psi, aatype, tables, atom37, pred_rigids, traj_fixed_mask, trans_traj, true, stream);
}
int fdipt_se3_reverse_step_indexed(const FdiptReverseIndexed* x, fdipt_stream_t stream) {
  return reverse_indexed(x, nullptr, false, stream);
}
int fdipt_se3_reverse_step_indexed_gen(const FdiptReverseIndexed* x, const uint64_t* noise_keys, fdipt_stream_t stream) {
  return reverse_indexed(x, noise_keys, true, stream);
}
int fdipt_noise_fill(int B, int N, const uint64_t* noise_keys, int purpose, int k_begin, int n_steps, double* out, fdipt_stream_t stream) {
  if (B <= 0 || N <= 0 || n_steps <= 0) return FDIPT_OK;
  if (!noise_keys || !out || purpose < 0 || purpose >= (int)FD_NOISE_PURPOSES || k_begin < 0) return FDIPT_EINVAL;
  const long n = (long)n_steps * B * N;
  hipLaunchKernelGGL(noise_fill_kernel, dim3(cdiv(n, FD_THREADS)), dim3(FD_THREADS), 0, (hipStream_t)stream, B, N, noise_keys,
                     (uint32_t)purpose, k_begin, n, out);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
int fdipt_igso3_rot_score(int B, int N, const float* quats_t, const float* quats_0, const double* sigma,
                          const float* res_mask, double* score, fdipt_stream_t s) {
  if (B <= 0 || N <= 0) return FDIPT_OK;
  if (!quats_t || !quats_0 || !sigma || !score) return FDIPT_EINVAL;
  return fd_rot_score(B, N, quats_t, 4, quats_0, 4, sigma, res_mask, score, (hipStream_t)s);
}
int fdipt_igso3_rot_score_cached(int B, int N, const float* quats_t, const float* quats_0, const double* score_table,
                                 const double* omega_edges, int n_omega, const float* res_mask, double* score, fdipt_stream_t s) {
  if (B <= 0 || N <= 0) return FDIPT_OK;
  if (!quats_t || !quats_0 || !score_table || !omega_edges || n_omega < 2 || !score) return FDIPT_EINVAL;
  ScoreTail x = {};
  x.score_table = score_table; x.omega_edges = omega_edges; x.n_omega = n_omega;
  // (sigma is not read with a table; the table itself stands in for the pointer so that the kernel's per-sample read stays in bounds)
  hipLaunchKernelGGL(rot_score_kernel<false>, dim3(cdiv((long)B * N, FD_THREADS / RS_LANES)), dim3(FD_THREADS), 0, (hipStream_t)s, B, N, quats_t, 4,
                     quats_0, 4, score_table, res_mask, score, x);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
int fdipt_r3_trans_score(int B, int N, const float* trans_t, const float* trans_0, const float* t, float min_b,
                         float max_b, float coordinate_scaling, const float* res_mask, float* score, fdipt_stream_t s) {
  if (B <= 0 || N <= 0) return FDIPT_OK;
  if (!trans_t || !trans_0 || !t || !score) return FDIPT_EINVAL;
  return fd_trans_score(B, N, trans_t, 3, trans_0, 3, t, min_b, max_b, coordinate_scaling, res_mask, score, (hipStream_t)s);
}
int fdipt_backbone_atoms(int n, const float* t7, const float* rot, const float* trans, const float* psi,
                         const int32_t* aatype, const void* tables, float* atom37, float* atom14, fdipt_stream_t s) {
  if (n <= 0) return FDIPT_OK;
  if ((!t7 && !(rot && trans)) || !psi || !tables) return FDIPT_EINVAL;
  return fd_backbone(n, t7, rot, trans, 3, psi, aatype, tables, atom37, atom14, (hipStream_t)s);
}
int fdipt_backbone_atoms_indexed(int n, const float* t7, const float* psi, const int32_t* aatype, const void* tables,
                                 float* atom37_rows, const int32_t* step_cursor, fdipt_stream_t s) {
  if (n <= 0) return FDIPT_OK;
  if (!t7 || !psi || !tables || !atom37_rows || !step_cursor) return FDIPT_EINVAL;
  return fd_backbone(n, t7, nullptr, nullptr, 3, psi, aatype, tables, atom37_rows, nullptr, (hipStream_t)s, FdStep{step_cursor});
}
int fdipt_backbone_atoms_kept(int n, const float* t7, const float* psi, const int32_t* aatype, const void* tables,
                              float* atom37_rows, const int32_t* step_cursor, const int32_t* frame_rows, fdipt_stream_t s) {
  if (n <= 0) return FDIPT_OK;
  if (!t7 || !psi || !tables || !atom37_rows || !step_cursor || !frame_rows) return FDIPT_EINVAL;
  return fd_backbone(n, t7, nullptr, nullptr, 3, psi, aatype, tables, atom37_rows, nullptr, (hipStream_t)s, FdStep{step_cursor, frame_rows});
}
}  // extern "C"

// ------------------------------------------------------------------ EigenFold confidence score
// experiments/utils.py:752-869 walks x_0 -> x_T with one-step forward noising and sums log p(x_{t-1} | x_t) - log q(x_t | x_{t-1}).
// The state between steps is what the reference carries: float32 rotation matrices + float32 translations (se3_diffuser.py:26-36),
// all arithmetic in between is float64 (NumPy on the host there).
struct SdeConsts { double so3_min_sigma, so3_max_sigma, r3_min_b, r3_max_b, cs; };
__device__ __forceinline__ double d_g_rot(const SdeConsts& k, double t) {  // so3_diffuser.py:299-319
  const double emax = exp(k.so3_max_sigma), emin = exp(k.so3_min_sigma);
  const double sig = log(t * emax + (1 - t) * emin);
  return sqrt(2 * (emax - emin) * sig / exp(sig));
}
__device__ __forceinline__ double d_b_t(const SdeConsts& k, double t) { return k.r3_min_b + t * (k.r3_max_b - k.r3_min_b); }  // r3:48-62
__device__ __forceinline__ void d_matmul3(const double* A, const double* B, double* C) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}
// transforms.compose_rotvec (framedipt/data/transforms.py:33-46)
__device__ __forceinline__ void d_compose_rotvec(const double* r1, const double* r2, double* out) {
  double R1[9], R2[9], Rc[9];
  d_so3_exp(r1, R1);
  d_so3_exp(r2, R2);
  d_matmul3(R1, R2, Rc);
  d_so3_log(Rc, out);
}
// so3_diffuser.py:99-119 align_rotation_vectors
__device__ __forceinline__ void d_align_rotvec(const double* in, const double* target, double* out) {
  const double ang = sqrt(in[0] * in[0] + in[1] * in[1] + in[2] * in[2]);
  const double tn = sqrt(target[0] * target[0] + target[1] * target[1] + target[2] * target[2]);
  const double ax[3] = {in[0] / ang, in[1] / ang, in[2] / ang};
  const double dot = (target[0] / tn) * ax[0] + (target[1] / tn) * ax[1] + (target[2] / tn) * ax[2];
  const double sign = dot > 0 ? 1.0 : (dot < 0 ? -1.0 : dot);  // np.sign (0 and NaN pass through)
  const double new_ang = sign > 0 ? ang : 2 * M_PI - ang;
  for (int c = 0; c < 3; ++c) out[c] = ax[c] * sign * new_ang;
}
// torch.distributions.Normal(mu, std).log_prob(x)
__device__ __forceinline__ double d_normal_logp(double x, double mu, double std) {
  const double d = x - mu;
  return -(d * d) / (2 * std * std) - log(std) - 0.91893853320467274178;  // log(sqrt(2 pi))
}
__device__ __forceinline__ void d_rot32_log(const float* R32, double* rv) {  // se3_diffuser.py:16-23 on a float32 matrix
  double R[9];
  for (int c = 0; c < 9; ++c) R[c] = (double)R32[c];
  d_so3_log(R, rv);
}

// SE3Diffuser.forward (se3_diffuser.py:50-95; r3_diffuser.py:122-161 with center=False; so3_diffuser.py:408-443)
// GEN (fdipt_se3_forward_step_gen): z_rot / z_trans are NULL and the values are drawn here (philox.hpp, the forward purposes)
template <bool GEN>
__device__ __forceinline__ void se3_forward_step_body(long n, const float* __restrict__ rot_1, const float* __restrict__ trans_1,
                                                      const float* __restrict__ mask, const double* __restrict__ z_rot,
                                                      const double* __restrict__ z_trans, double t_1, double dt, double noise_scale,
                                                      const SdeConsts& k, float* __restrict__ rot_out, float* __restrict__ trans_out,
                                                      float* __restrict__ t7_out, const uint64_t* __restrict__ keys, int N, int step) {
  const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  double zt[3] = {0.0, 0.0, 0.0}, zr[3] = {0.0, 0.0, 0.0};
  if (GEN) {
    const uint64_t key = keys[r / N];
    fd_noise3(key, (uint32_t)(r % N), (uint32_t)step, FD_NOISE_FWD_TRANS, zt);
    fd_noise3(key, (uint32_t)(r % N), (uint32_t)step, FD_NOISE_FWD_ROT, zr);
  }
  const bool has_mask = mask != nullptr;
  const double m = has_mask ? (double)mask[r] : 1.0;
  const double sdt = sqrt(dt), bt = d_b_t(k, t_1), g_tr = sqrt(bt), g_rot = d_g_rot(k, t_1);
  float tr[3];
  for (int c = 0; c < 3; ++c) {
    const double x0 = (double)trans_1[r * 3 + c];
    const double x = x0 * k.cs;
    double pert = (-0.5 * bt * x) * dt + g_tr * sdt * (noise_scale * (GEN ? zt[c] : z_trans[r * 3 + c]));
    if (has_mask) pert *= m;
    const double xt = (x + pert) / k.cs;
    tr[c] = (float)(has_mask ? m * xt + (1 - m) * x0 : xt);
  }
  double rv1[3], pert[3], rvt[3], Ro[9];
  d_rot32_log(rot_1 + r * 9, rv1);
  for (int c = 0; c < 3; ++c) {
    pert[c] = g_rot * sdt * (noise_scale * (GEN ? zr[c] : z_rot[r * 3 + c]));
    if (has_mask) pert[c] *= m;
  }
  d_compose_rotvec(rv1, pert, rvt);
  if (has_mask)
    for (int c = 0; c < 3; ++c) rvt[c] = m * rvt[c] + (1 - m) * rv1[c];
  d_so3_exp(rvt, Ro);
  float Rf[9];
  for (int c = 0; c < 9; ++c) Rf[c] = (float)Ro[c];
  for (int c = 0; c < 9; ++c) fd_st(rot_out + r * 9 + c, Rf[c]);
  for (int c = 0; c < 3; ++c) fd_st(trans_out + r * 3 + c, tr[c]);
  if (t7_out) {  // Rigid.to_tensor_7 (rot_to_quat up to sign, as in the reverse step)
    double Rd[9], q[4];
    for (int c = 0; c < 9; ++c) Rd[c] = (double)Rf[c];
    d_markley(Rd, q);
    if (q[3] < 0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
    float* o = t7_out + r * 7;
    fd_st(o, (float)q[3]); fd_st(o + 1, (float)q[0]); fd_st(o + 2, (float)q[1]); fd_st(o + 3, (float)q[2]);
    fd_st(o + 4, tr[0]); fd_st(o + 5, tr[1]); fd_st(o + 6, tr[2]);
  }
}
__global__ void se3_forward_step_kernel(long n, const float* __restrict__ rot_1, const float* __restrict__ trans_1,
                                        const float* __restrict__ mask, const double* __restrict__ z_rot,
                                        const double* __restrict__ z_trans, double t_1, double dt, double noise_scale, SdeConsts k,
                                        float* __restrict__ rot_out, float* __restrict__ trans_out, float* __restrict__ t7_out) {
  se3_forward_step_body<false>(n, rot_1, trans_1, mask, z_rot, z_trans, t_1, dt, noise_scale, k, rot_out, trans_out, t7_out, nullptr, 1, 0);
}
__global__ void se3_forward_step_gen_kernel(long n, int N, const float* __restrict__ rot_1, const float* __restrict__ trans_1,
                                            const float* __restrict__ mask, const uint64_t* __restrict__ keys, int step, double t_1,
                                            double dt, double noise_scale, SdeConsts k, float* __restrict__ rot_out,
                                            float* __restrict__ trans_out, float* __restrict__ t7_out) {
  se3_forward_step_body<true>(n, rot_1, trans_1, mask, nullptr, nullptr, t_1, dt, noise_scale, k, rot_out, trans_out, t7_out, keys, N, step);
}

// One block per sample: out[b] = {log p backward (trans, rot), log q forward (trans, rot)} summed over the diffused residues
// (se3_diffuser.py:97-196, r3_diffuser.py:163-260, so3_diffuser.py:466-567, r3_utils.py:10-42).  scores == nullptr: forward terms only.
__global__ __launch_bounds__(FD_THREADS) void se3_step_log_prob_kernel(int N, const float* __restrict__ rot_t, const float* __restrict__ trans_t,
                                                                        const float* __restrict__ rot_1, const float* __restrict__ trans_1,
                                                                        const double* __restrict__ rot_score, const float* __restrict__ trans_score,
                                                                        const float* __restrict__ mask, double t, double t_1, double dt,
                                                                        SdeConsts k, double* __restrict__ out) {
  __shared__ double red[4][FD_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double sdt = sqrt(dt);
  const double bt = d_b_t(k, t), bt1 = d_b_t(k, t_1), g_rot = d_g_rot(k, t), g_rot1 = d_g_rot(k, t_1);
  double acc[4] = {0, 0, 0, 0};
  for (int i = tid; i < N; i += FD_THREADS) {
    const long r = (long)b * N + i;
    const double m = mask ? (double)mask[r] : 1.0;
    if (mask && mask[r] == 0.f) continue;  // torch.masked_select(log_p, mask.bool())
    // ---- translations (scaled coordinates)
    for (int c = 0; c < 3; ++c) {
      const double xt = (double)trans_t[r * 3 + c] * k.cs, x1 = (double)trans_1[r * 3 + c] * k.cs;
      if (trans_score) {  // p(x_{t-1} | x_t): r3_diffuser.py:163-191, 227-260 (mask as bool)
        const double f = -0.5 * bt * xt, g2 = bt;
        const double mu = xt - (f - g2 * (double)trans_score[r * 3 + c]) * dt;
        acc[0] += d_normal_logp(x1, mu, sqrt(bt) * sdt);
      }
      const double muf = (x1 + (-0.5 * bt1 * x1) * dt) * m;  // q(x_t | x_{t-1}): r3_diffuser.py:193-225
      acc[2] += d_normal_logp(xt, muf, sqrt(bt1) * sdt);
    }
    // ---- rotations (rotation vectors of the float32 matrices)
    double rvt[3], rv1[3], al[3];
    d_rot32_log(rot_t + r * 9, rvt);
    d_rot32_log(rot_1 + r * 9, rv1);
    if (rot_score) {  // so3_diffuser.py:497-567
      double drift[3], mu[3];
      for (int c = 0; c < 3; ++c) drift[c] = g_rot * g_rot * rot_score[r * 3 + c] * dt * m;
      d_compose_rotvec(rvt, drift, mu);
      d_align_rotvec(rv1, mu, al);
      for (int c = 0; c < 3; ++c) acc[1] += d_normal_logp(al[c], mu[c], g_rot * sdt);
    }
    d_align_rotvec(rvt, rv1, al);  // so3_diffuser.py:466-495
    for (int c = 0; c < 3; ++c) acc[3] += d_normal_logp(al[c], rv1[c], g_rot1 * sdt);
  }
  for (int q = 0; q < 4; ++q) {
    const double s = wave_sum_d(acc[q]);
    if (lane == 0) red[q][wave] = s;
  }
  __syncthreads();
  if (tid < 4) {
    double s = 0;
    for (int w = 0; w < FD_THREADS / 64; ++w) s += red[tid][w];
    out[b * 4 + tid] = s;
  }
}

// Terminal term of logp_confidence_score (experiments/utils.py:846-866): standard-normal log density of the scaled x_T translations
// (float32 there) over the diffused residues + log(1 / pi^2) per diffused residue.  out[b] = {trans, rot}
__global__ __launch_bounds__(FD_THREADS) void se3_prior_log_prob_kernel(int N, const float* __restrict__ trans_T, const float* __restrict__ mask,
                                                                         float cs, double* __restrict__ out) {
  __shared__ double red[2][FD_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double a0 = 0, a1 = 0;
  for (int i = tid; i < N; i += FD_THREADS) {
    const long r = (long)b * N + i;
    if (mask && mask[r] == 0.f) continue;
    for (int c = 0; c < 3; ++c) {
      const float x = trans_T[r * 3 + c] * cs;
      a0 += (double)(-(x * x) / 2.f - 0.91893853320467274178f);
    }
    a1 += mask ? (double)mask[r] : 1.0;
  }
  a0 = wave_sum_d(a0); a1 = wave_sum_d(a1);
  if (lane == 0) { red[0][wave] = a0; red[1][wave] = a1; }
  __syncthreads();
  if (tid == 0) {
    double s0 = 0, s1 = 0;
    for (int w = 0; w < FD_THREADS / 64; ++w) { s0 += red[0][w]; s1 += red[1][w]; }
    out[b * 2] = s0;
    out[b * 2 + 1] = log(1.0 / (M_PI * M_PI)) * s1;
  }
}

extern "C" {
int fdipt_se3_forward_step(int B, int N, const float* rot_t_1, const float* trans_t_1, const float* diffuse_mask, const double* z_rot,
                           const double* z_trans, double t_1, double dt, double noise_scale, double so3_min_sigma, double so3_max_sigma,
                           double r3_min_b, double r3_max_b, double coordinate_scaling, float* rot_t, float* trans_t, float* rigids_t,
                           fdipt_stream_t stream) {
  if (B <= 0 || N <= 0) return FDIPT_OK;
  if (!rot_t_1 || !trans_t_1 || !z_rot || !z_trans || !rot_t || !trans_t || !(t_1 >= 0 && t_1 <= 1)) return FDIPT_EINVAL;
  const long n = (long)B * N;
  const SdeConsts k = {so3_min_sigma, so3_max_sigma, r3_min_b, r3_max_b, coordinate_scaling};
  hipLaunchKernelGGL(se3_forward_step_kernel, dim3(cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, n, rot_t_1, trans_t_1, diffuse_mask,
                     z_rot, z_trans, t_1, dt, noise_scale, k, rot_t, trans_t, rigids_t);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
int fdipt_se3_forward_step_gen(int B, int N, const float* rot_t_1, const float* trans_t_1, const float* diffuse_mask,
                               const uint64_t* noise_keys, int step, double t_1, double dt, double noise_scale, double so3_min_sigma,
                               double so3_max_sigma, double r3_min_b, double r3_max_b, double coordinate_scaling, float* rot_t,
                               float* trans_t, float* rigids_t, fdipt_stream_t stream) {
  if (B <= 0 || N <= 0) return FDIPT_OK;
  if (!rot_t_1 || !trans_t_1 || !noise_keys || step < 0 || !rot_t || !trans_t || !(t_1 >= 0 && t_1 <= 1)) return FDIPT_EINVAL;
  const long n = (long)B * N;
  const SdeConsts k = {so3_min_sigma, so3_max_sigma, r3_min_b, r3_max_b, coordinate_scaling};
  hipLaunchKernelGGL(se3_forward_step_gen_kernel, dim3(cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, n, N, rot_t_1, trans_t_1,
                     diffuse_mask, noise_keys, step, t_1, dt, noise_scale, k, rot_t, trans_t, rigids_t);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
int fdipt_se3_step_log_prob(int B, int N, const float* rot_t, const float* trans_t, const float* rot_t_1, const float* trans_t_1,
                            const double* rot_score, const float* trans_score, const float* diffuse_mask, double t, double t_1, double dt,
                            double so3_min_sigma, double so3_max_sigma, double r3_min_b, double r3_max_b, double coordinate_scaling,
                            double* out, fdipt_stream_t stream) {
  if (B <= 0 || N <= 0) return FDIPT_OK;
  if (!rot_t || !trans_t || !rot_t_1 || !trans_t_1 || !out || (rot_score == nullptr) != (trans_score == nullptr)) return FDIPT_EINVAL;
  const SdeConsts k = {so3_min_sigma, so3_max_sigma, r3_min_b, r3_max_b, coordinate_scaling};
  hipLaunchKernelGGL(se3_step_log_prob_kernel, dim3(B), dim3(FD_THREADS), 0, (hipStream_t)stream, N, rot_t, trans_t, rot_t_1, trans_t_1,
                     rot_score, trans_score, diffuse_mask, t, t_1, dt, k, out);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
int fdipt_se3_prior_log_prob(int B, int N, const float* trans_T, const float* diffuse_mask, double coordinate_scaling, double* out,
                             fdipt_stream_t stream) {
  if (B <= 0 || N <= 0) return FDIPT_OK;
  if (!trans_T || !out) return FDIPT_EINVAL;
  hipLaunchKernelGGL(se3_prior_log_prob_kernel, dim3(B), dim3(FD_THREADS), 0, (hipStream_t)stream, N, trans_T, diffuse_mask,
                     (float)coordinate_scaling, out);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
}  // extern "C"
