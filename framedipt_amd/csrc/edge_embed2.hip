// edge_embed2.hip — half-precision pair embedder (framedipt/model/score_network.py:98-105,184-197: the edge MLP of
// Embedder.forward) for the reference widths, activations in REGISTERS.
//
//   * the first layer has no GEMM: cross-concat / relative-index / distogram features are per-residue or one-hot, so its
//     pre-activation is four table rows summed (Pi[i] + Pj[j] + R[idx_i - idx_j] + D[bin(|ca_i - ca_j|)]), gathered as whole
//     512 B rows through a wave-private LDS tile, the next tile's rows requested a tile ahead;
//   * layers 2 / 3 are computed TRANSPOSED, D[out feature, pair] = W[out, k] * X^T[k, pair]: weights are the MFMA A operand
//     from two LDS-resident 32 KB images (persistent block), activations the B operand in registers; the C/D fragment of a
//     layer is the B fragment of the next one up to a fixed 16-wise permutation of k folded into the images;
//   * LayerNorm + mask epilogue in registers; the same epilogue emits the first block's pair bias linear_b(z)/sqrt(3) from
//     its output fragments (saves a pass over z).
//   * a model without the self-conditioning distogram (embed_self_conditioning = False, FdiptDims.num_bins = 0) runs the
//     DIST = false instantiation: three table rows per pair, no distances, no bins, nothing of the distogram in LDS.
#include "common.hpp"
#include "kernels.hpp"
#include "ee2_table_map.hpp"

#define ET2_CZ 128
#define EE2_WBC 2048     // compact linear_b image of the first block (8 head rows); then a 64 B zero unit, the hi / lo down_z images (8 KB each)
#define EE2_EPI_IMG (EE2_WBC + 64 + 2 * 8192 + 128)  // ... and the down_z bias [32] f32

// logical (row, 16-byte chunk) -> byte offset inside a weight image (bank-conflict-free ds_read_b128)
__host__ __device__ __forceinline__ int et2_off_wide(int row, int c, int row_bytes) {
  return row * row_bytes + ((c ^ (row & 15)) << 4);
}
// acc += W_slab[32 x 16*KS] * B[16*KS x 32]: A fragments stream from LDS through a DEPTH-deep register ring so that
// every ds_read_b128 is issued DEPTH MFMAs (= DEPTH*32 cycles) ahead of its consumer.
template <int KS, int ROWB, int DEPTH = 8, int ABL = 0>
__device__ __forceinline__ void mma_slab(f32x16& acc, const char* slab, int li, int hi, const hx8* Bf) {
  hx8 ring[DEPTH];
#pragma unroll
  for (int s = 0; s < DEPTH; ++s) ring[s] = fd_frag(slab + et2_off_wide(li, 2 * s + hi, ROWB));
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    acc = fd_mfma32(ring[s % DEPTH], Bf[s], acc);
    if (s + DEPTH < KS) ring[s % DEPTH] = fd_frag(slab + et2_off_wide(li, 2 * (s + DEPTH) + hi, ROWB));
    __builtin_amdgcn_sched_barrier(0);  // pin the MFMA / ds_read interleave (hipcc otherwise sinks the reads)
  }
}

// ---- VALU-lean pieces for the embedder (its waves are issue-bound: ~1500 VALU instructions per 32-pair tile before) ----
// LayerNorm epilogue of the embedder in packed fp32 math (one pass: sum and sum of squares; the layer bias is already in Y).  z' is
// staged in the wave's LDS tile and stored as whole 64 B row segments; the first block's pair bias comes from the same fragments.
// pz_tile (round 6): when set, the epilogue also emits pair_z = down_z(z') + b of the first block's IPA for this row's 32 keys (8 key
// groups of 256 B, layout fd_pz_bytes; groups >= ng_valid are beyond N): z' is the A operand of these MFMAs, so a lane (d, half) ends
// up with four consecutive keys per register quad = 8 B of the image; hi + lo weight fragments follow the compact linear_b image in LDS
// TABLE (the row-table launch, below): the 32 "pairs" of the tile are table rows; the same arithmetic, but the pair bias goes to
// bias_out as [row][8 heads] and pair_z to pz_tile as [row][32 d] (nvalid rows), the records ee2_spread_kernel copies from
template <bool TRACE, bool TABLE = false>
__device__ __forceinline__ void ee_ln_epilogue(f32x16 (&Y)[4], const float* gamma_l, const float* beta_l, float em, int li, int hi,
                                               int lane, char* stage, half_t* __restrict__ z_tile, int nvalid,
                                               float* __restrict__ tr_row, bool valid, const char* wb_lds, const f32x4 bbv,
                                               float* __restrict__ bias_out, int H, long bidx, int ii, int jj, int nt,
                                               half_t* __restrict__ pz_tile, int ng_valid) {
  f32x2 u1 = {0.f, 0.f}, u2 = {0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      const f32x2 y = {Y[t][r], Y[t][r + 1]};
      u1 += y;
      u2 = __builtin_elementwise_fma(y, y, u2);
    }
  float s1 = u1[0] + u1[1], s2 = u2[0] + u2[1];
  s1 += __shfl_xor(s1, 32, 64);
  s2 += __shfl_xor(s2, 32, 64);
  const float mu = s1 * (1.0f / ET2_CZ);
  const float rstd = 1.0f / sqrtf(fmaxf(s2 * (1.0f / ET2_CZ) - mu * mu, 0.f) + 1e-5f);
  const f32x2 sa = {rstd, rstd}, sc = {-mu * rstd, -mu * rstd}, em2 = {em, em};
  u32x4 zB[8];  // half-precision z' as B fragments
  // (gamma, beta) of a feature group come from LDS one group AHEAD of their use; the interleave is pinned: left alone hipcc
  // emits read -> s_waitcnt lgkmcnt(0) -> use for each of the 16 groups (16 exposed LDS round trips per tile)
  f32x4 gq[2], bq[2];
  gq[0] = *(const f32x4*)(gamma_l + 4 * hi);
  bq[0] = *(const f32x4*)(beta_l + 4 * hi);
#pragma unroll
  for (int idx = 0; idx < 16; ++idx) {
    const int t = idx >> 2, g = idx & 3, f0 = 32 * t + 8 * g + 4 * hi;
    if (idx + 1 < 16) {
      const int f1 = 32 * ((idx + 1) >> 2) + 8 * ((idx + 1) & 3) + 4 * hi;
      gq[(idx + 1) & 1] = *(const f32x4*)(gamma_l + f1);
      bq[(idx + 1) & 1] = *(const f32x4*)(beta_l + f1);
    }
    const f32x4 gm = gq[idx & 1], bt = bq[idx & 1];
    f32x2 o0 = {Y[t][4 * g], Y[t][4 * g + 1]}, o1 = {Y[t][4 * g + 2], Y[t][4 * g + 3]};
    o0 = __builtin_elementwise_fma(o0, sa, sc);
    o1 = __builtin_elementwise_fma(o1, sa, sc);
    o0 = __builtin_elementwise_fma(o0, f32x2{gm[0], gm[1]}, f32x2{bt[0], bt[1]}) * em2;
    o1 = __builtin_elementwise_fma(o1, f32x2{gm[2], gm[3]}, f32x2{bt[2], bt[3]}) * em2;
    const u32x2 ow = {fd_cvt_pk(o0[0], o0[1]), fd_cvt_pk(o1[0], o1[1])};
    // features f0..f0+3 = bytes 2 f0 .. 2 f0 + 7 of the pair's row: 16 B unit 4t + g, half hi; unit u of row r at u ^ (r & 15)
    *(u32x2*)(stage + li * 256 + (((4 * t + g) ^ (li & 15)) << 4) + 8 * hi) = ow;
    zB[2 * t + (g >> 1)][2 * (g & 1)] = ow[0];
    zB[2 * t + (g >> 1)][2 * (g & 1) + 1] = ow[1];
    if (TRACE && valid) *(f32x4*)(tr_row + f0) = f32x4{o0[0], o0[1], o1[0], o1[1]};
    __builtin_amdgcn_sched_barrier(0);
  }
  // every LDS operand of the tail is requested before the first use: the 8 row segments of the z tile (other lanes' writes above:
  // DS operations of a wave execute in order) and the 8 linear_b fragments
  const int sr = lane >> 4, sc16 = lane & 15;
  u16x8 zrow[8];
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int r = 4 * it + sr;
    zrow[it] = *(const u16x8*)(stage + r * 256 + ((sc16 ^ (r & 15)) << 4));
  }
  const bool full = nvalid == 32;  // wave-uniform: 9 of 10 tiles at N = 300 take the branch-free stores
  if (wb_lds) {
    hx8 wf[8];
    {  // compact image (8 head rows): lanes >= 8 read the zero unit behind it
      const int wl = li < 8 ? hi * 128 + li * 16 : EE2_WBC, ws = li < 8 ? 256 : 0;
#pragma unroll
      for (int s = 0; s < 8; ++s) wf[s] = fd_frag(wb_lds + wl + s * ws);
    }
    __builtin_amdgcn_sched_barrier(0);
    f32x16 accb;
#pragma unroll
    for (int r = 0; r < 16; ++r) accb[r] = 0.f;
#pragma unroll
    for (int s = 0; s < 8; ++s) accb = fd_mfma32(wf[s], __builtin_bit_cast(hx8, zB[s]), accb);
    float* bo = bias_out + fd_bias_frag_off(bidx * H + 4 * hi, nt, ii, valid ? jj : 0);  // 32 lanes = 32 consecutive keys: 128 B rows
    const long hstride = (long)nt * nt * 1024;  // floats per (sample, head)
    if constexpr (TABLE) {
      if (valid) *(f32x4*)(bias_out + li * 8 + 4 * hi) = f32x4{accb[0] + bbv[0], accb[1] + bbv[1], accb[2] + bbv[2], accb[3] + bbv[3]};
    } else if (full && H == 8) {
#pragma unroll
      for (int r = 0; r < 4; ++r) bo[r * hstride] = accb[r] + bbv[r];
    } else if (valid) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (4 * hi + r < H) bo[r * hstride] = accb[r] + bbv[r];
    }
    if (pz_tile) {
      const char* dzh = wb_lds + EE2_WBC + 64;
      const float bd = *(const float*)(dzh + 2 * 8192 + 4 * li);
      f32x16 accd;
#pragma unroll
      for (int r = 0; r < 16; ++r) accd[r] = bd;
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {  // hi image, then lo image: 8 fragments each, requested a batch ahead of their MFMAs
#pragma unroll
        for (int s = 0; s < 8; ++s) wf[s] = fd_frag(dzh + h2 * 8192 + s * 1024 + lane * 16);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 8; ++s) accd = fd_mfma32(__builtin_bit_cast(hx8, zB[s]), wf[s], accd);
      }
      // registers 4 g .. 4 g + 3 = keys 8 g + 4 hi + q of the tile = key group 2 g + hi, channel d = li
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const u32x2 ow = {fd_cvt_pk(accd[4 * g], accd[4 * g + 1]), fd_cvt_pk(accd[4 * g + 2], accd[4 * g + 3])};
        if constexpr (TABLE) {  // (the same conversions; one row's 32 channels are 64 contiguous bytes)
          unsigned short* pt = (unsigned short*)pz_tile + (8 * g + 4 * hi) * 32 + li;
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (8 * g + 4 * hi + q < nvalid) pt[q * 32] = (unsigned short)(ow[q >> 1] >> (16 * (q & 1)));
        } else if (2 * g + hi < ng_valid) *(u32x2*)(pz_tile + ((2 * g + hi) * 32 + li) * 4) = ow;
      }
    }
  }
  if (full) {
#pragma unroll
    for (int it = 0; it < 8; ++it) *(u16x8*)(z_tile + (4 * it + sr) * ET2_CZ + 8 * sc16) = zrow[it];
  } else {
#pragma unroll
    for (int it = 0; it < 8; ++it)
      if (4 * it + sr < nvalid) *(u16x8*)(z_tile + (4 * it + sr) * ET2_CZ + 8 * sc16) = zrow[it];
  }
}

// edge_embed2_kernel — bf16 pair branch of Embedder.forward (framedipt/model/score_network.py:98-105,173-196) in the
// same register-resident style.  Layer 1 has no GEMM: the cross-concat / relative-index / distogram features are
// one-hot or per-residue, so h1 = relu(Pi[i] + Pj[j] + R[idx_i - idx_j] + D[bin(|ca_i - ca_j|)]) is four table rows
// summed directly in B-fragment layout.  Layers 2 and 3 (128x128 each, 64 KB bf16 together) stay RESIDENT in LDS for
// the whole persistent block, so there is no per-tile barrier: waves loop over 32-pair tiles independently.
#define EE2_IMG (128 * 128 * 2)  // 32 KB per layer

__global__ void ee2_build_images_kernel(const float* __restrict__ w2, const float* __restrict__ w3,
                                        half_t* __restrict__ img) {
  const int n_chunks = 2 * EE2_IMG / 16;
  for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < n_chunks; g += gridDim.x * blockDim.x) {
    const int layer = g / (EE2_IMG / 16), q = g % (EE2_IMG / 16);
    const int row = q / 16, cp = q % 16, c = cp ^ (row & 15);  // row = out feature (slab = row/32), 256-byte rows
    const float* src = layer == 0 ? w2 : w3;
    for (int e = 0; e < 8; ++e) {
      const int k = c * 8 + e;
      const int col = layer == 0 ? k : (k & ~15) + fd_perm16(k & 15);
      img[(long)g * 8 + e] = f2h(src[(long)row * 128 + col]);
    }
  }
}
// fp16x: W - half(W) in the same layout, read by the LO kernels from L2 (the LDS holds the hi images and is full)
__global__ void ee2_build_lo_images_kernel(const float* __restrict__ w2, const float* __restrict__ w3,
                                           half_t* __restrict__ img) {
  const int n_chunks = 2 * EE2_IMG / 16;
  for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < n_chunks; g += gridDim.x * blockDim.x) {
    const int layer = g / (EE2_IMG / 16), q = g % (EE2_IMG / 16);
    const int row = q / 16, cp = q % 16, c = cp ^ (row & 15);
    const float* src = layer == 0 ? w2 : w3;
    for (int e = 0; e < 8; ++e) {
      const int k = c * 8 + e;
      const int col = layer == 0 ? k : (k & ~15) + fd_perm16(k & 15);
      const float v = src[(long)row * 128 + col];
      img[(long)g * 8 + e] = f2h(v - h2f(f2h(v)));
    }
  }
}
int fd_ee2_build_images(const float* w2, const float* w3, void* img, hipStream_t st, int lo) {
  hipLaunchKernelGGL(ee2_build_images_kernel, dim3(16), dim3(256), 0, st, w2, w3, (half_t*)img);
  if (lo) hipLaunchKernelGGL(ee2_build_lo_images_kernel, dim3(16), dim3(256), 0, st, w2, w3, (half_t*)img + 2 * EE2_IMG / 2);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
size_t fd_ee2_image_bytes(int lo) { return (lo ? 4 : 2) * EE2_IMG; }
// acc += W_lo slab * B with the A fragments straight from global memory (L2-resident 64 KB lo images, layout of the LDS slabs)
__device__ __forceinline__ void mma_slab_lo(f32x16& acc, const char* __restrict__ slab, int li, int hi, const hx8* Bf) {
  hx8 r[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) r[s] = __builtin_bit_cast(hx8, *(const u16x8*)(slab + et2_off_wide(li, 2 * s + hi, 256)));
#pragma unroll
  for (int s = 0; s < 8; ++s) acc = fd_mfma32(r[s], Bf[s], acc);
}

// 512-thread persistent blocks: 8 independent waves (two per SIMD) share the 64 KB weight images; every wave owns an
// 8 KB LDS tile that transposes between "whole 512 B table rows per 32 lanes" (the global side) and MFMA fragments.
//
// Work decomposition (round 2): a tile is one query row i against 32 consecutive keys j0..j0+31 of one sample, and a wave walks
// CONSECUTIVE rows i of one (sample, key tile) group.  Of the four table rows a pair sums, only R[idx_i - idx_j] is then a per-tile
// gather from L2 (16 KB): Pj[j] of the 32 keys stays in 64 registers for the whole walk, Pi[i] is one 512 B row per tile and the
// distogram table D (num_bins + 1 rows) sits in LDS.  The previous generation walked flat 32-pair tiles and fetched all four rows of
// every pair (64 KB per tile through the 64 B/clk L2 -> CU path: 1.5 GB per launch).  The next row's R rows and Pi row are
// requested before the LayerNorm epilogue of the current one.
#define EE2_THREADS 512
// phase profile (-DEE2_PROF, tools/micro/ee2_bench.hip): cycles of wave 0 of every block, accumulated over its tiles
#ifdef EE2_PROF
__device__ unsigned ee2_prof[256 * 8];
#define EE2_STAMP(k)                                             \
  do {                                                           \
    __builtin_amdgcn_sched_barrier(0);                           \
    const unsigned t_ = (unsigned)__builtin_amdgcn_s_memtime(); \
    ph[k] += t_ - tlast;                                         \
    tlast = t_;                                                  \
    __builtin_amdgcn_sched_barrier(0);                           \
  } while (0)
#else
#define EE2_STAMP(k) \
  do {               \
  } while (0)
#endif
#define EE2_MAXB 63      // distogram bins (edges in LDS)
#define EE2_MAXB_LDS 39  // ... with the table rows in LDS as well (20 KB)
#define EE2_LDS_NODIST (2 * EE2_IMG + 8 * 8192 + 4 * ET2_CZ * 4 + EE2_EPI_IMG)  // ... + the epilogue's images
#define EE2_LDS_BASE (EE2_LDS_NODIST + 256)                                       // ... + distogram edges
#define EE2_LDS_MAX 163840
// the reference model's 22 bins keep their table rows in LDS with 64 B to spare: the epilogue's images cannot grow without moving
// them to the L2 path
static_assert(EE2_LDS_BASE + (22 + 1) * ET2_CZ * 4 <= EE2_LDS_MAX, "edge_embed2: the 22-bin distogram rows no longer fit in LDS");
// DIST = false: the model has no distogram channels (num_bins = 0); DLDS is then false as well.  LO (fp16x): layers 2 and 3 add W_lo h,
// the lo images following the hi ones in `img` (fd_ee2_build_images lo = 1)
// distogram bin of one distance: calc_distogram's strict inequalities against the stored edges (last upper edge 1e8); the
// candidate comes from the edge spacing, its neighbours are re-tested, so the result is the one a full scan finds.  One copy for
// the pair kernel and the spread launch: a pair's bin must not depend on which of them computes it
struct Ee2Bins {
  const float* edg;  // [nb + 1] in LDS
  int nb;
  float e0, inv_step;
  __device__ __forceinline__ Ee2Bins(const float* e, int n) : edg(e), nb(n), e0(e[0]), inv_step(n > 1 ? 1.0f / (e[1] - e[0]) : 0.f) {}
  __device__ __forceinline__ int of(float d) const {
    int k0 = (int)((d - e0) * inv_step);
    k0 = k0 < 1 ? 1 : (k0 > nb - 2 ? nb - 2 : k0);
    int bin = nb;
#pragma unroll
    for (int k = -1; k <= 1; ++k) {
      const int kk = k0 + k;
      if (kk >= 0 && kk < nb && d > edg[kk] && d < edg[kk + 1]) bin = kk;
    }
    return bin;
  }
  __device__ __forceinline__ int of_pair(float i0, float i1, float i2, float j0, float j1, float j2) const {
    const float dx = i0 - j0, dy = i1 - j1, dz = i2 - j2;
    return of(sqrtf(dx * dx + dy * dy + dz * dz));
  }
};

// ---- the row table (model.hip: ForwardPlan.ee_table).  Without aatype features Pi and Pj depend on a residue only through its
// fixed-mask bit, so the launch's whole output for a pair is a function of (sample, class_i, class_j, rel, bin): the TABLE
// instantiation evaluates each such row once (same arithmetic as the pair kernel) and ee2_spread_kernel copies the records to the pairs.
// Row r of sample b: b * rows_per_sample + ((2 class_i + class_j) * n_rel + rel) * (num_bins + 1) + bin; the sample's last row is the
// all-zero row of masked pairs.  Records: z [128] half, pair bias [8] f32, pair_z [32] half, one array each.
// Only LEADERS have their rows evaluated (ee2_leaders_kernel below; a.leaders): a follower's pairs point into its leader's rows, the
// zero row included, and the follower's own region of the table stays unwritten and unread.
__host__ __device__ __forceinline__ int ee2_rows_per_sample(int n_rel, int nb) { return 4 * n_rel * (nb + 1) + 1; }
size_t fd_ee2_table_bytes(int B, int n_rel, int num_bins) {
  return (size_t)B * ee2_rows_per_sample(n_rel, num_bins) * (ET2_CZ * 2 + 8 * 4 + 32 * 2);
}
struct Ee2Table {
  half_t* z;
  float* bias;
  half_t* pz;
  int rps;
};
__host__ __device__ __forceinline__ Ee2Table ee2_table_of(void* table, int B, int n_rel, int nb) {
  Ee2Table t;
  t.rps = ee2_rows_per_sample(n_rel, nb);
  const size_t rows = (size_t)B * t.rps;
  t.z = (half_t*)table;
  t.bias = (float*)((char*)table + rows * ET2_CZ * 2);
  t.pz = (half_t*)((char*)table + rows * (ET2_CZ * 2 + 8 * 4));
  return t;
}

// TABLE: a tile is 32 bins of one (leader, class pair, rel) and the walk goes over rel: Pi / Pj are the rows of the first residue of
// either class (items of a class pair the sample does not have end at once), R[rel] is one row for the whole tile, the mask is 1.
// nt = bin tiles.  The launcher cannot know how many leaders the batch has: the kernel counts them and derives its items from the count
// (ee2_table_map.hpp; wpg, rpw and n_items are not read), so that the leaders' rows are shared among all waves, and deals consecutive
// items to different blocks (the live items of a one-class batch are the first ones: a block then holds as few of them as can be)
template <bool DIST, bool DLDS, bool TRACE, bool LO = false, bool TABLE = false>
__global__ __launch_bounds__(EE2_THREADS, 1) void edge_embed2_kernel(EdgeEmbedArgs a, const char* __restrict__ img, int nt, int wpg,
                                                                     int rpw, int n_items) {
  static_assert(!TABLE || (DIST && !TRACE), "the row table: distogram models, no trace");
  extern __shared__ __attribute__((aligned(16))) char smem[];
#ifdef EE2_PROF
  unsigned ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tlast = (unsigned)__builtin_amdgcn_s_memtime();
#endif
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, li = lane & 31;
  char* stage = smem + 2 * EE2_IMG + wave * 8192;
  float* vec = (float*)(smem + 2 * EE2_IMG + 8 * 8192);  // [b2 | b3 | gamma | beta] x 128
  char* wbl = (char*)(vec + 4 * ET2_CZ);                 // compact image of linear_b | zero unit | down_z hi | lo | bias (all optional)
  float* edg = (float*)(wbl + EE2_EPI_IMG);              // [num_bins + 1] distogram edges, the last one 1e8
  float* dl = edg + 64;                                  // DLDS: [num_bins + 1][128] distogram rows of the first layer
  if (DIST && tid <= a.num_bins) edg[tid] = tid < a.num_bins ? a.edges[tid] : 1e8f;
  if (a.wb_img && tid < EE2_WBC / 16) fd_dma16((const char*)a.wb_img + tid * 16, wbl + (tid & ~63) * 16);
  if (tid < 16) *(unsigned*)(wbl + EE2_WBC + 4 * tid) = 0u;
  if (a.pz_out) {
    fd_dma16((const char*)a.wdz_img + tid * 16, wbl + EE2_WBC + 64 + (tid & ~63) * 16);
    fd_dma16((const char*)a.wdz_img_lo + tid * 16, wbl + EE2_WBC + 64 + 8192 + (tid & ~63) * 16);
    if (tid < 32) *(float*)(wbl + EE2_WBC + 64 + 2 * 8192 + 4 * tid) = a.bdz[tid];
  }
  for (int u = 0; u < 2 * EE2_IMG / 16 / EE2_THREADS; ++u)
    fd_dma16(img + (size_t)(u * EE2_THREADS + tid) * 16, smem + (size_t)(u * EE2_THREADS + (tid & ~63)) * 16);
  if (tid < 4 * ET2_CZ) {
    const int which = tid >> 7, c = tid & 127;
    vec[tid] = which == 0 ? a.b2[c] : (which == 1 ? a.b3[c] : (which == 2 ? a.gamma[c] : a.beta[c]));
  }
  if (DLDS) {
    f32x4 t[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {  // (EE2_MAXB_LDS + 1) * 32 units of 16 B <= 3 * 512
      const int v = u * EE2_THREADS + tid;
      if (v < (a.num_bins + 1) * 32) t[u] = *(const f32x4*)(a.dtab + (long)v * 4);
    }
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int v = u * EE2_THREADS + tid;
      if (v < (a.num_bins + 1) * 32) *(f32x4*)(dl + (long)v * 4) = t[u];
    }
  }
  fd_dma_wait();
  __syncthreads();
  EE2_STAMP(0);
  const int N = a.N, nb = a.num_bins;
  const float* b2row = vec + 4 * hi;
  const f32x4 bbv = a.wb_img ? f32x4{a.bb[4 * hi], a.bb[4 * hi + 1], a.bb[4 * hi + 2], a.bb[4 * hi + 3]} : f32x4{0.f, 0.f, 0.f, 0.f};
  const Ee2Bins bins(edg, nb);
  const Ee2Table tab = TABLE ? ee2_table_of(a.table, a.B, a.n_rel, nb) : Ee2Table{};
  if (TABLE && blockIdx.x == 0 && tid < 64) {  // the zero rows of masked pairs: what the epilogue emits from a zeroed z
    for (int b = 0; b < a.B; ++b) {
      const long zr = (long)(b + 1) * tab.rps - 1;
      ((unsigned*)(tab.z + zr * ET2_CZ))[tid] = 0u;
      if (tid < 8) tab.bias[zr * 8 + tid] = 0.f + (tid < a.H ? a.bb[tid] : 0.f);
      if (tid < 32) ((unsigned short*)tab.pz)[zr * 32 + tid] = (unsigned short)fd_cvt_pk(0.f + a.bdz[tid], 0.f);
    }
  }
  Ee2TableMap tmap = {};
  if constexpr (TABLE) {  // (wave-uniform scalar loads; sample 0 always leads)
    int n_lead = 0;
    for (int s = 0; s < a.B; ++s) n_lead += a.leaders[s] == s ? 1 : 0;
    tmap = ee2_table_map(n_lead < 1 ? 1 : n_lead, nt, a.n_rel);
  }
  const int n_it = TABLE ? tmap.n_items : n_items;
  for (int item = TABLE ? wave * gridDim.x + blockIdx.x : blockIdx.x * 8 + wave; item < n_it; item += gridDim.x * 8) {
    // ---- group (sample b, key tile jt): per-key state of the 32 keys, resident for the whole walk
    int cc = 0, b, jt, i_first, i_end;
    if constexpr (TABLE) {
      const Ee2TableItem ti = ee2_table_item(tmap, item);
      cc = ti.cc; jt = ti.jt; i_first = ti.rel0; i_end = ti.rel1;
      b = 0;
      for (int s = 0, k = -1; s < a.B; ++s)  // the sample of leader ti.lead
        if (a.leaders[s] == s && ++k == ti.lead) { b = s; break; }
    } else {
      const int grp = item / wpg, part = item - grp * wpg;
      b = grp / nt; jt = grp - b * nt;
      i_first = part * rpw; i_end = (i_first + rpw < N) ? i_first + rpw : N;
    }
    const int j0 = jt * 32, n_keys = TABLE ? nb + 1 : N;  // TABLE: the walk is over rel, the "keys" are bins
    if (i_first >= i_end) continue;
    const int nvalid = n_keys - j0 < 32 ? n_keys - j0 : 32;
    const bool valid = li < nvalid;
    int rep_i = 0, rep_j = 0;  // TABLE: the first residue of class_i / class_j (wave-uniform)
    if constexpr (TABLE) {
      rep_i = rep_j = N;
      for (int k0 = 0; k0 < N && (rep_i == N || rep_j == N); k0 += 64) {
        const int k = k0 + lane;
        const int c = k < N ? (a.fixed_mask[(long)b * N + k] != 0.f ? 1 : 0) : -1;
        const unsigned long long mi_ = __ballot(c == (cc >> 1)), mj_ = __ballot(c == (cc & 1));
        if (rep_i == N && mi_) rep_i = k0 + __ffsll((long long)mi_) - 1;
        if (rep_j == N && mj_) rep_j = k0 + __ffsll((long long)mj_) - 1;
      }
      rep_i = __builtin_amdgcn_readfirstlane(rep_i);
      rep_j = __builtin_amdgcn_readfirstlane(rep_j);
      if (rep_i == N || rep_j == N) continue;  // the sample has no pair of this class pair
    }
    const int j = TABLE ? rep_j : valid ? j0 + li : N - 1;
    const long bj = (long)b * N + j;
    const int sj = TABLE ? 0 : a.seq_idx[bj];
    const float mj = TABLE ? 1.f : a.res_mask[bj];
    const float cj0 = DIST && !TABLE ? a.sc_ca[bj * 3] : 0.f, cj1 = DIST && !TABLE ? a.sc_ca[bj * 3 + 1] : 0.f,
                cj2 = DIST && !TABLE ? a.sc_ca[bj * 3 + 2] : 0.f;
    // row r of the tile at + min(r, nvalid - 1) * 128 (TABLE: the one row of class_j)
    const float* pj_base = a.pj + ((long)b * N + (TABLE ? rep_j : j0)) * ET2_CZ + 4 * li;
    // per-row scalars (wave-uniform addresses: scalar loads) -> this lane's table row ids
    // per-row scalars: requested (scalar loads) at the top of the previous row, turned into table row ids after its gather
    struct RowIn { int si; float mi, c0, c1, c2; };
    auto row_request = [&](int i) {
      const long bi = (long)b * N + i;
      if constexpr (TABLE) return RowIn{i, 1.f, 0.f, 0.f, 0.f};
      else if constexpr (DIST) return RowIn{a.seq_idx[bi], a.res_mask[bi], a.sc_ca[bi * 3], a.sc_ca[bi * 3 + 1], a.sc_ca[bi * 3 + 2]};
      else return RowIn{a.seq_idx[bi], a.res_mask[bi], 0.f, 0.f, 0.f};
    };
    auto row_ids = [&](const RowIn& r, int& rel, int& bin, float& msk) {
      msk = r.mi * mj;
      if constexpr (TABLE) {
        rel = b * a.n_rel + r.si;
        bin = valid ? j0 + li : nb;
      } else {
        rel = b * a.n_rel + r.si - sj + a.rel_off;
        if constexpr (DIST) bin = bins.of_pair(r.c0, r.c1, r.c2, cj0, cj1, cj2);
        else bin = 0;
      }
    };
    f32x4 RR[16], PJ[16], PI;
    auto request = [&](int i, int rel, const int it0, const int it1) {
      if (it0 == 0) PI = *(const f32x4*)(a.pi + ((long)b * N + (TABLE ? rep_i : i)) * ET2_CZ + 4 * li);
#pragma unroll
      for (int it = it0; it < it1; ++it) {
        const int r = 2 * it + hi;
        const int rrel = __shfl(rel, r, 64);
        RR[it] = *(const f32x4*)(a.rtab + (long)rrel * ET2_CZ + 4 * li);
        PJ[it] = *(const f32x4*)(pj_base + (TABLE ? 0 : (r < nvalid ? r : nvalid - 1) * ET2_CZ));  // (the same 16 KB for every row of the walk: L2 hits)
      }
    };
    int rel, bin;
    float msk;
    row_ids(row_request(i_first), rel, bin, msk);
    request(i_first, rel, 0, 16);
    EE2_STAMP(1);
    for (int i = i_first; i < i_end; ++i) {
      // Lane-derived LDS / global offsets are recomputed per row: left to itself hipcc hoists ~100 of them out of this loop and
      // spills them (every reload is a vmcnt wait in front of the matrix phase).
      int lane_o = lane;
      asm volatile("" : "+v"(lane_o));
      const int hi = lane_o >> 5, li = lane_o & 31;
      const float* b2row = vec + 4 * hi;
      const int i_next = i + 1 < i_end ? i + 1 : i;
      const RowIn rin = row_request(i_next);
      // ---- layer 1 has no GEMM: h1 = relu(Pi[i] + Pj[j] + R[rel] + D[bin]).  Two pairs per instruction: lanes 0..31 / 32..63
      // hold one whole 512 B row each.  The 16 bin shuffles, then the 16 distogram rows, are issued as batches (one LDS round trip
      // each instead of one per pair of rows).  Without the distogram: h1 = relu(Pi[i] + Pj[j] + R[rel])
#pragma unroll
      for (int half = 0; half < 4; ++half) {
      f32x4 DD[4];
      if constexpr (DIST) {
      int rb[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) rb[q] = __shfl(bin, 2 * (4 * half + q) + hi, 64);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        DD[q] = DLDS ? *(const f32x4*)(dl + rb[q] * ET2_CZ + 4 * li) : *(const f32x4*)(a.dtab + (long)rb[q] * ET2_CZ + 4 * li);
      __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int it = 4 * half + q, r = 2 * it + hi;
        const f32x4 x1 = PI, x2 = PJ[it], x3 = RR[it];
        // packed adds, conversion, then relu on the half-precision bit patterns (v_pk_max_i16)
        f32x2 sA, sB;
        if constexpr (DIST) {
          const f32x4 x4 = DD[q];
          sA = (f32x2{x1[0], x1[1]} + f32x2{x2[0], x2[1]}) + (f32x2{x3[0], x3[1]} + f32x2{x4[0], x4[1]});
          sB = (f32x2{x1[2], x1[3]} + f32x2{x2[2], x2[3]}) + (f32x2{x3[2], x3[3]} + f32x2{x4[2], x4[3]});
        } else {
          sA = (f32x2{x1[0], x1[1]} + f32x2{x2[0], x2[1]}) + f32x2{x3[0], x3[1]};
          sB = (f32x2{x1[2], x1[3]} + f32x2{x2[2], x2[3]}) + f32x2{x3[2], x3[3]};
        }
        typedef short s16x4 __attribute__((ext_vector_type(4)));
        const u32x2 cw = {fd_cvt_pk(sA[0], sA[1]), fd_cvt_pk(sB[0], sB[1])};
        const u32x2 pk = __builtin_bit_cast(u32x2, __builtin_elementwise_max(__builtin_bit_cast(s16x4, cw), s16x4{0, 0, 0, 0}));
        // [32 pairs][256 B] tile, 16 B unit u of row r at u ^ (r & 15)
        *(u32x2*)(stage + r * 256 + (((li >> 1) ^ (r & 15)) << 4) + 8 * (li & 1)) = pk;
      }
      }
      EE2_STAMP(2);
      const float msk_cur = msk;
      row_ids(rin, rel, bin, msk);  // the next row's ids (this row's were consumed by the gather above)
      hx8 H1[8];
#pragma unroll
      for (int s = 0; s < 8; ++s) H1[s] = fd_frag(stage + li * 256 + (((2 * s + hi) ^ (li & 15)) << 4));
      hx8 H2[8];
#pragma unroll
      for (int T = 0; T < 4; ++T) {
        f32x16 acc;  // starts as the layer bias (LDS reads straight into the accumulator: no VALU)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 bv = *(const f32x4*)(b2row + 32 * T + 8 * g);
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[4 * g + q] = bv[q];
        }
        mma_slab<8, 256>(acc, smem + T * 32 * 256, li, hi, H1);
        if constexpr (LO) mma_slab_lo(acc, img + 2 * EE2_IMG + T * 32 * 256, li, hi, H1);
        fd_hand_off(acc, H2[2 * T], H2[2 * T + 1]);
      }
      EE2_STAMP(3);
      f32x16 Y[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {  // starts as the layer bias b3
          const f32x4 bv = *(const f32x4*)(vec + ET2_CZ + 4 * hi + 32 * t + 8 * g);
#pragma unroll
          for (int q = 0; q < 4; ++q) Y[t][4 * g + q] = bv[q];
        }
        mma_slab<8, 256>(Y[t], smem + EE2_IMG + t * 32 * 256, li, hi, H2);
        if constexpr (LO) mma_slab_lo(Y[t], img + 3 * EE2_IMG + t * 32 * 256, li, hi, H2);
      }
      EE2_STAMP(4);
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      request(i_next, rel, 0, 0);  // the next row's Pi in flight under the epilogue (its R / Pj rows after it: register budget)
      __builtin_amdgcn_sched_barrier(0);
      const int rel_next = rel;
      if constexpr (TABLE) {
        const long trow = (long)b * tab.rps + ((long)cc * a.n_rel + i) * (nb + 1) + j0;  // first row of the tile
        ee_ln_epilogue<false, true>(Y, vec + 2 * ET2_CZ, vec + 3 * ET2_CZ, msk_cur, li, hi, lane, stage, tab.z + trow * ET2_CZ, nvalid, nullptr,
                                    valid, wbl, bbv, tab.bias + trow * 8, a.H, b, i, j0 + li, nt, tab.pz + trow * 32, (nvalid + 3) >> 2);
      } else {
      const long prow = ((long)b * N + i) * N + j0;  // first pair of the tile
      ee_ln_epilogue<TRACE>(Y, vec + 2 * ET2_CZ, vec + 3 * ET2_CZ, msk_cur, li, hi, lane, stage, (half_t*)a.z_out + prow * ET2_CZ, nvalid,
                     TRACE ? a.trace + (prow + (valid ? li : 0)) * ET2_CZ : nullptr, valid, a.wb_img ? wbl : nullptr, bbv,
                     a.bias_out, a.H, b, i, j0 + li, nt,
                     a.pz_out ? a.pz_out + (((long)b * N + i) * ((N + 3) >> 2) + (j0 >> 2)) * 128 : nullptr, (nvalid + 3) >> 2);
      }
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      request(i_next, rel_next, 0, 16);
      EE2_STAMP(5);
    }
  }
#ifdef EE2_PROF
  if (tid == 0 && blockIdx.x < 256)
    for (int k = 0; k < 8; ++k) ee2_prof[blockIdx.x * 8 + k] = ph[k];
#endif
}

int fd_edge_embed2(const EdgeEmbedArgs& a, const void* img, hipStream_t st, int lo) {
  const bool dist = a.num_bins > 0;  // num_bins = 0: the model has no distogram channels (sc_ca, dtab and edges are not read)
  if (a.num_bins > EE2_MAXB || (dist && a.num_bins < 3)) return FDIPT_EINVAL;
  if (dist && (!a.sc_ca || !a.dtab || !a.edges)) return FDIPT_EINVAL;
  if (a.pz_out && (!a.wb_img || !a.wdz_img || !a.wdz_img_lo || !a.bdz)) return FDIPT_EINVAL;
  const bool dlds = dist && a.num_bins <= EE2_MAXB_LDS && EE2_LDS_BASE + (a.num_bins + 1) * ET2_CZ * 4 <= EE2_LDS_MAX;  // (else the distogram rows come from L2)
  const int lds = dist ? EE2_LDS_BASE + (dlds ? (a.num_bins + 1) * ET2_CZ * 4 : 0) : EE2_LDS_NODIST;
  typedef void (*kern_t)(EdgeEmbedArgs, const char*, int, int, int, int);
  static const kern_t kerns[12] = {edge_embed2_kernel<true, false, false>, edge_embed2_kernel<true, false, true>,
                                   edge_embed2_kernel<true, true, false>,  edge_embed2_kernel<true, true, true>,
                                   edge_embed2_kernel<false, false, false>, edge_embed2_kernel<false, false, true>,
                                   edge_embed2_kernel<true, false, false, true>, edge_embed2_kernel<true, false, true, true>,
                                   edge_embed2_kernel<true, true, false, true>,  edge_embed2_kernel<true, true, true, true>,
                                   edge_embed2_kernel<false, false, false, true>, edge_embed2_kernel<false, false, true, true>};
  const int kid = (lo ? 6 : 0) + (dist ? 2 * dlds : 4) + (a.trace != nullptr);
  static FdPerDevice attr_dev[12];
  const int dev_ = fd_device();
  if (!attr_dev[kid].get(dev_)) {
    if (hipFuncSetAttribute((const void*)kerns[kid], hipFuncAttributeMaxDynamicSharedMemorySize, EE2_LDS_MAX) != hipSuccess)
      return FDIPT_ELAUNCH;
    attr_dev[kid].set(dev_, 1);
  }
  // one work item = (sample, key tile of 32, range of rpw consecutive query rows); wpg items per group so that ~2048 waves are busy
  const int nt = cdiv(a.N, 32), n_groups = a.B * nt, n_waves = 256 * 8;
  int wpg = n_waves / n_groups < 1 ? 1 : n_waves / n_groups;
  if (wpg > a.N) wpg = a.N;
  const int rpw = cdiv(a.N, wpg);
  wpg = cdiv(a.N, rpw);
  const int n_items = n_groups * wpg;
  const int cus = a.reserve_cus > 0 && a.reserve_cus < 248 ? (256 - a.reserve_cus) & ~7 : 256;  // (whole XCD rounds of 8)
  const int grid = cdiv(n_items, 8) < cus ? cdiv(n_items, 8) : cus;
  hipLaunchKernelGGL(kerns[kid], dim3(grid), dim3(EE2_THREADS), lds, st, a, (const char*)img, nt, wpg, rpw, n_items);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}

// ---- the row table: its leaders, its launch, and the spread of its records to the pairs
// Block b decides a.leaders[b]: the first sample c < b that (1) has every fixed-mask class b has, (2) whose Pi and Pj rows of the
// representatives (first residues) of b's classes carry the bits of b's, and (3) whose R rows carry the bits of b's; b itself if there
// is none.  These rows, the sample-free distogram rows and the weights are all a table row is made of, so c's rows ARE b's rows.  Bits
// are compared, not values (-0 and NaN patterns count).  The relation is transitive, so the first match is itself a leader.
// (3) is constant along a trajectory and 2.4 MB of reads at c4, so it is decided once, when the R rows are made (fdipt_sample_setup:
// ee2_rel_leaders_kernel, a.rel_lead[b] = the first sample with b's R rows); the per-step launch compares two integers.
#define EL_THREADS 1024
__global__ __launch_bounds__(EL_THREADS) void ee2_rel_leaders_kernel(int n4, const u32x4* __restrict__ rtab, int32_t* __restrict__ rel_lead) {
  const int tid = threadIdx.x, b = blockIdx.x;
  int lead = b;
  for (int c = 0; c < b; ++c) {
    const u32x4 *rb4 = rtab + (long)b * n4, *rc4 = rtab + (long)c * n4;
    int same = 1;
#pragma unroll 4
    for (int k = tid; k < n4; k += EL_THREADS) {
      const u32x4 x = rb4[k], y = rc4[k];
      same &= (x[0] == y[0]) & (x[1] == y[1]) & (x[2] == y[2]) & (x[3] == y[3]);
    }
    if (__syncthreads_and(same)) {
      lead = c;
      break;
    }
  }
  if (tid == 0) rel_lead[b] = lead;
}
int fd_ee2_rel_leaders(int B, long row_floats, const float* rtab, int32_t* rel_lead, hipStream_t st) {
  if (B < 1 || row_floats < 4 || (row_floats & 3) || row_floats / 4 > 0x7fffffffL || !rtab || !rel_lead) return FDIPT_EINVAL;
  hipLaunchKernelGGL(ee2_rel_leaders_kernel, dim3(B), dim3(EL_THREADS), 0, st, (int)(row_floats / 4), (const u32x4*)rtab, rel_lead);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
#define ELS_THREADS 512
__global__ __launch_bounds__(ELS_THREADS) void ee2_leaders_kernel(EdgeEmbedArgs a) {
  __shared__ int rep[4];  // first residue of class 0 / 1 of b, then of the candidate (N: the sample has none)
  const int tid = threadIdx.x, b = blockIdx.x, N = a.N;
  auto reps = [&](int s, int* out) {
    if (tid < 2) out[tid] = N;
    __syncthreads();
    for (int k = tid; k < N; k += ELS_THREADS) atomicMin(&out[a.fixed_mask[(long)s * N + k] != 0.f ? 1 : 0], k);
    __syncthreads();
  };
  reps(b, rep);
  const int r0 = rep[0], r1 = rep[1], rl = a.rel_lead[b];
  int lead = b;
  for (int c = 0; c < b; ++c) {
    if (a.rel_lead[c] != rl) continue;  // other R rows (block-uniform)
    reps(c, rep + 2);
    const int q0 = rep[2], q1 = rep[3];
    __syncthreads();  // (the next candidate overwrites them)
    if ((r0 < N && q0 == N) || (r1 < N && q1 == N)) continue;  // block-uniform
    int same = 1;
    if (tid < 4 * ET2_CZ) {  // (class, Pi | Pj, channel)
      const int cls = tid >> 8, ch = tid & 127, rb = cls ? r1 : r0, rc = cls ? q1 : q0;
      const unsigned* t = (const unsigned*)((tid >> 7) & 1 ? a.pj : a.pi);
      if (rb < N) same = t[((long)b * N + rb) * ET2_CZ + ch] == t[((long)c * N + rc) * ET2_CZ + ch];
    }
    if (__syncthreads_and(same)) {
      lead = c;
      break;
    }
  }
  if (tid == 0) a.leaders[b] = lead;
}
const half_t* fd_ee2_table_pz(const void* table, int B, int n_rel, int num_bins) { return ee2_table_of((void*)table, B, n_rel, num_bins).pz; }
int fd_edge_embed2_leaders(const EdgeEmbedArgs& a, hipStream_t st) {
  if (!fd_edge_embed2_table_supported(a) || !a.leaders || !a.fixed_mask || !a.pi || !a.pj || !a.rel_lead) return FDIPT_EINVAL;
  hipLaunchKernelGGL(ee2_leaders_kernel, dim3(a.B), dim3(ELS_THREADS), 0, st, a);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
int fd_edge_embed2_table_supported(const EdgeEmbedArgs& a) {
  const bool dlds = a.num_bins <= EE2_MAXB_LDS && EE2_LDS_BASE + (a.num_bins + 1) * ET2_CZ * 4 <= EE2_LDS_MAX;
  return a.num_bins >= 3 && dlds && a.H == 8 && a.N % 4 == 0 && (long)a.B * ee2_rows_per_sample(a.n_rel, a.num_bins) < (1L << 24);
}
int fd_edge_embed2_table(const EdgeEmbedArgs& a_, const void* img, hipStream_t st, int lo) {
  EdgeEmbedArgs a = a_;
  if (!fd_edge_embed2_table_supported(a) || !a.table || !a.leaders || !a.fixed_mask || !a.wb_img || !a.wdz_img || !a.wdz_img_lo || !a.bdz || a.trace)
    return FDIPT_EINVAL;
  a.pz_out = (half_t*)a.table;  // (any non-null value: the set-up loads the down_z images; the records go to the table)
  const int lds = EE2_LDS_BASE + (a.num_bins + 1) * ET2_CZ * 4;
  typedef void (*kern_t)(EdgeEmbedArgs, const char*, int, int, int, int);
  static const kern_t kerns[2] = {edge_embed2_kernel<true, true, false, false, true>, edge_embed2_kernel<true, true, false, true, true>};
  static FdPerDevice attr_dev[2];
  const int dev_ = fd_device(), kid = lo ? 1 : 0;
  if (!attr_dev[kid].get(dev_)) {
    if (hipFuncSetAttribute((const void*)kerns[kid], hipFuncAttributeMaxDynamicSharedMemorySize, EE2_LDS_MAX) != hipSuccess)
      return FDIPT_ELAUNCH;
    attr_dev[kid].set(dev_, 1);
  }
  // one work item = (class pair, leader, bin tile of 32, range of consecutive rel), laid out by the kernel from the leader count
  // (ee2_table_map.hpp); a one-class batch (de novo sampling) has a quarter of the items live.  The grid gives each of those a wave of
  // its own at the leader count that has the most of them
  const int nt = cdiv(a.num_bins + 1, 32);
  const int cus = a.reserve_cus > 0 && a.reserve_cus < 248 ? (256 - a.reserve_cus) & ~7 : 256;
  const int live = ee2_table_max_live_blocks(a.B, nt, a.n_rel), grid = live < cus ? live : cus;
  hipLaunchKernelGGL(kerns[kid], dim3(grid), dim3(EE2_THREADS), lds, st, a, (const char*)img, nt, 0, 0, 0);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}

// The spread: a wave takes SP_ROWS consecutive query rows against 32 keys, finds every pair's table row (in the rows of the sample's
// leader) exactly as the pair kernel finds its layer-1 rows (row_ids / Ee2Bins) and copies the row's records: the pair bias into the
// fragment order ipa_attn3 reads, (WPZ) pair_z into the [row][j / 4][32 d][4 j] image, and (WZ) the z row itself.  a.row_idx, when set, receives the row of every pair.
#define SP_THREADS 256
#define SP_ROWS 4
template <bool WZ, bool WPZ>
__global__ __launch_bounds__(SP_THREADS) void ee2_spread_kernel(EdgeEmbedArgs a, int nt, int wpg, int n_items) {
  __shared__ float edg[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hi = lane >> 5, li = lane & 31, N = a.N, nb = a.num_bins;
  if (tid <= nb) edg[tid] = tid < nb ? a.edges[tid] : 1e8f;
  __syncthreads();
  const Ee2Bins bins(edg, nb);
  const Ee2Table tab = ee2_table_of(a.table, a.B, a.n_rel, nb);
  const long hstride = (long)nt * nt * 1024;  // floats per (sample, head)
  const int sr = lane >> 4, sc16 = lane & 15;
  for (int item = blockIdx.x * (SP_THREADS / 64) + wave; item < n_items; item += gridDim.x * (SP_THREADS / 64)) {
    const int grp = item / wpg, part = item - grp * wpg;
    const int b = grp / nt, jt = grp - b * nt, j0 = jt * 32;
    const int lead = a.leaders[b];  // the sample whose rows b's pairs read
    const int i_first = part * SP_ROWS, i_end = (i_first + SP_ROWS < N) ? i_first + SP_ROWS : N;
    const int nvalid = N - j0 < 32 ? N - j0 : 32;
    const bool valid = li < nvalid;
    const int j = valid ? j0 + li : N - 1;
    const long bj = (long)b * N + j;
    const int sj = a.seq_idx[bj], fj = a.fixed_mask[bj] != 0.f ? 1 : 0;
    const float mj = a.res_mask[bj];
    const float cj0 = a.sc_ca[bj * 3], cj1 = a.sc_ca[bj * 3 + 1], cj2 = a.sc_ca[bj * 3 + 2];
    for (int i = i_first; i < i_end; ++i) {
      const long bi = (long)b * N + i;
      const int si = a.seq_idx[bi], fi = a.fixed_mask[bi] != 0.f ? 1 : 0;
      const float msk = a.res_mask[bi] * mj;
      const int rel = si - sj + a.rel_off;
      const int bin = bins.of_pair(a.sc_ca[bi * 3], a.sc_ca[bi * 3 + 1], a.sc_ca[bi * 3 + 2], cj0, cj1, cj2);
      const int row = lead * tab.rps + (msk != 0.f ? ((2 * fi + fj) * a.n_rel + rel) * (nb + 1) + bin : tab.rps - 1);
      if (a.row_idx && hi == 0 && valid) a.row_idx[bi * N + j] = row;
      {  // pair bias: 32 lanes = 32 consecutive keys of one head (128 B rows), heads 4 hi .. 4 hi + 3
        const f32x4 bv = *(const f32x4*)(tab.bias + (long)row * 8 + 4 * hi);
        float* bo = a.bias_out + fd_bias_frag_off((long)b * 8 + 4 * hi, nt, i, j);
        if (valid) {
#pragma unroll
          for (int r = 0; r < 4; ++r) bo[r * hstride] = bv[r];
        }
      }
      if constexpr (WPZ) {  // pair_z: lane (d = li, hi) writes the 4 keys of key group 2 g + hi
        half_t* pz_tile = a.pz_out + (bi * (N >> 2) + (j0 >> 2)) * 128;
        const unsigned short* tp = (const unsigned short*)tab.pz + li;
        unsigned short v[16];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int q = 0; q < 4; ++q) v[4 * g + q] = tp[(long)__shfl(row, 8 * g + 4 * hi + q, 64) * 32];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const u32x2 ow = {(unsigned)v[4 * g] | ((unsigned)v[4 * g + 1] << 16), (unsigned)v[4 * g + 2] | ((unsigned)v[4 * g + 3] << 16)};
          if (8 * g + 4 * hi < nvalid) *(u32x2*)(pz_tile + ((2 * g + hi) * 32 + li) * 4) = ow;
        }
      }
      if constexpr (WZ) {
        half_t* z_tile = (half_t*)a.z_out + (bi * N + j0) * ET2_CZ;
        u16x8 zr[8];
#pragma unroll
        for (int it = 0; it < 8; ++it) zr[it] = *(const u16x8*)(tab.z + (long)__shfl(row, 4 * it + sr, 64) * ET2_CZ + 8 * sc16);
#pragma unroll
        for (int it = 0; it < 8; ++it)
          if (4 * it + sr < nvalid) *(u16x8*)(z_tile + (4 * it + sr) * ET2_CZ + 8 * sc16) = zr[it];
      }
    }
  }
}
int fd_edge_embed2_spread(const EdgeEmbedArgs& a, hipStream_t st, int write_z) {
  if (!fd_edge_embed2_table_supported(a) || !a.table || !a.leaders || !a.fixed_mask || !a.bias_out || (write_z && !a.z_out)) return FDIPT_EINVAL;
  const int nt = cdiv(a.N, 32), wpg = cdiv(a.N, SP_ROWS), n_items = a.B * nt * wpg;
  const int grid = cdiv(n_items, SP_THREADS / 64);
  typedef void (*kern_t)(EdgeEmbedArgs, int, int, int);
  static const kern_t kerns[4] = {ee2_spread_kernel<false, false>, ee2_spread_kernel<false, true>, ee2_spread_kernel<true, false>, ee2_spread_kernel<true, true>};
  hipLaunchKernelGGL(kerns[(write_z ? 2 : 0) + (a.pz_out ? 1 : 0)], dim3(grid), dim3(SP_THREADS), 0, st, a, nt, wpg, n_items);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
