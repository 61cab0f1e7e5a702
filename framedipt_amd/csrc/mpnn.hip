// mpnn.hip — inverse folding on the device (include/fdipt.h, "inverse folding"): the vanilla full-backbone
// ProteinMPNN and (dims->ca_only, section 7.12) its CA-only sibling, which differs in the feature kernel alone; inference only,
// float32 throughout.
//
// Every matmul-shaped step has the same shape: the (up to 64) edges of ONE row are the rows of a 64 x IN activation tile in LDS, and
// the tile goes through a [IN][128] weight (stored transposed in the image) on v_mfma_f32_32x32x2_f32: wave w owns output columns
// 32w .. 32w+31 of both 32-row tiles, its B operand comes straight from the image (lane l reads [k + (l>>5)][32w + (l&31)]: two full
// 128-byte lines per step).  Inputs wider than 128 are staged 128 columns at a time into the one tile and accumulated in registers, a
// layer's output is written back over the tile once every wave has read it.  Edge slots past K_eff are zero rows and never gathered.
//
//   mpnn_features_kernel   block per row: CA distances to all columns, the K_eff smallest by (distance, index) through a rank count in
//                          LDS, 16 positional + 25 x 16 RBF inputs, edge_embedding, norm_edges, W_e -> h_E
//   mpnn_ca_features_kernel  the same block for the CA-only model: the same neighbours (mp_neighbours), 16 positional + 9 x 16 RBF inputs
//                          over the array-shifted traces + 7 orientation inputs (dU, Q) from the frames of the row and its neighbours
//   mpnn_enc_kernel<false> block per row: [h_V_i, h_E_ij, h_V_j] -> W1, W2, W3 (GELU), masked sum / 30, LN, FFN, LN, mask -> new h_V
//   mpnn_enc_kernel<true>  block per row: the same gather on the new h_V -> W11, W12, W13, + h_E, LN -> h_E (in place: a row's own edges)
//   mpnn_order_kernel      block per sequence: the decoding step of every row (the inverse of decoding_order)
//   mpnn_score_kernel      block per (row, sequence, backbone), one launch per decoder layer; args.unconditional: no neighbour decoded
//   mpnn_design_kernel     ONE persistent block per (sequence, backbone) walks the rows in decoding order; its h_V stack lives in the
//                          workspace and is touched by this block only, the letters live in LDS.  No block waits on another.  Tied
//                          groups and the per-row controls of the sampling epilogue: DESIGN.md section 7.11.
// Sums run in a fixed order (edge slot ascending, k ascending), so a row's bits do not depend on B or M.
#include "common.hpp"

#define MP_H 128
#define MP_LD 129   // tile row stride in floats: lane l of an A fragment reads row l&31, and 129 puts 32 rows in 32 banks
#define MP_ROWS 64
#define MP_V 21

// ---- the weight image (float offsets), in the order of the table in fdipt.h
namespace mpw {
constexpr long POS_W = 0, POS_B = POS_W + 66 * 16, EDGE_W = POS_B + 16, EDGE_G = EDGE_W + 416 * 128, EDGE_B = EDGE_G + 128, WE_W = EDGE_B + 128,
               WE_B = WE_W + 128 * 128, WS = WE_B + 128, ENC0 = WS + MP_V * 128;
// one encoder layer
constexpr long E_W1 = 0, E_B1 = E_W1 + 384 * 128, E_W2 = E_B1 + 128, E_B2 = E_W2 + 128 * 128, E_W3 = E_B2 + 128, E_B3 = E_W3 + 128 * 128, E_LN1G = E_B3 + 128,
               E_LN1B = E_LN1G + 128, E_WIN = E_LN1B + 128, E_BIN = E_WIN + 128 * 512, E_WOUT = E_BIN + 512, E_BOUT = E_WOUT + 512 * 128,
               E_LN2G = E_BOUT + 128, E_LN2B = E_LN2G + 128, E_W11 = E_LN2B + 128, E_B11 = E_W11 + 384 * 128, E_W12 = E_B11 + 128,
               E_B12 = E_W12 + 128 * 128, E_W13 = E_B12 + 128, E_B13 = E_W13 + 128 * 128, E_LN3G = E_B13 + 128, E_LN3B = E_LN3G + 128, E_SIZE = E_LN3B + 128;
constexpr long DEC0 = ENC0 + 3 * E_SIZE;
// one decoder layer
constexpr long D_W1 = 0, D_B1 = D_W1 + 512 * 128, D_W2 = D_B1 + 128, D_B2 = D_W2 + 128 * 128, D_W3 = D_B2 + 128, D_B3 = D_W3 + 128 * 128, D_LN1G = D_B3 + 128,
               D_LN1B = D_LN1G + 128, D_WIN = D_LN1B + 128, D_BIN = D_WIN + 128 * 512, D_WOUT = D_BIN + 512, D_BOUT = D_WOUT + 512 * 128,
               D_LN2G = D_BOUT + 128, D_LN2B = D_LN2G + 128, D_SIZE = D_LN2B + 128;
constexpr long OUT_W = DEC0 + 3 * D_SIZE, OUT_B = OUT_W + 128 * MP_V, TOTAL = OUT_B + MP_V;
static_assert(TOTAL == 1660485, "the parameter count of the vanilla model");
// The CA-only image is the same table with 167 rows of edge_embedding: every offset past EDGE_W lies CA_SHIFT lower (MpCtx::W).
constexpr long EDGE_IN = 416, EDGE_IN_CA = 167, CA_SHIFT = (EDGE_IN - EDGE_IN_CA) * 128;
static_assert(TOTAL - CA_SHIFT == 1628613, "the parameter count of the CA-only model, its five unread parameters left out");
}  // namespace mpw

// what every kernel needs: the caller's arguments and the workspace carved up
struct MpCtx {
  FdiptMpnnArgs a;
  int K;          // K_eff
  float* hE;      // [B,N,K,128]
  float* hV[2];   // [B,N,128] ping / pong of the encoder; the encoder's result ends in hV[1]
  float* stack;   // [3][B,M,N,128]: the decoder layers' outputs per sequence
  int32_t* pos;   // [B,M,N]: the decoding step of a row (the inverse of decoding_order)
  long shift;     // 0, or mpw::CA_SHIFT for the CA-only image
  // the image at an offset of the table past EDGE_W (every matrix and vector but the positional ones and edge_embedding itself)
  __device__ __forceinline__ const float* W(long off) const { return a.weights + (off - shift); }
};

struct MpAcc { f32x16 t[2]; };
__device__ __forceinline__ void mp_zero(MpAcc& c) {
#pragma unroll
  for (int r = 0; r < 16; ++r) c.t[0][r] = 0.f, c.t[1][r] = 0.f;
}
// acc += tile[64][0 .. kw) * Wt[kw][128]   (kw even)
__device__ __forceinline__ void mp_mma(MpAcc& c, const float* tile, const float* __restrict__ Wt, int kw, int wave, int lane) {
  const int li = lane & 31, hi = lane >> 5;
  const float* a0 = tile + li * MP_LD + hi;
  const float* a1 = a0 + 32 * MP_LD;
  const float* w = Wt + hi * MP_H + wave * 32 + li;
#pragma unroll 8
  for (int k = 0; k < kw; k += 2) {
    const float b = w[(long)k * MP_H];
    c.t[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[k], b, c.t[0], 0, 0, 0);
    c.t[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[k], b, c.t[1], 0, 0, 0);
  }
}
// tile[row][col] = f(acc, col) for the wave's 64 x 32 slab
template <class F>
__device__ __forceinline__ void mp_store(const MpAcc& c, float* tile, int wave, int lane, F&& f) {
  const int col = wave * 32 + (lane & 31);
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) tile[(t * 32 + c_row(r, lane)) * MP_LD + col] = f(c.t[t][r], col);
}
__device__ __forceinline__ float mp_gelu(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }

// LayerNorm (eps 1e-5, biased variance) of one 128-vector by ONE wave; x may be a tile row or a vector in LDS
__device__ __forceinline__ void mp_ln(float* x, const float* __restrict__ g, const float* __restrict__ b, int lane) {
  const float v0 = x[lane], v1 = x[lane + 64];
  const float mean = wave_sum(v0 + v1) * (1.f / MP_H);
  const float d0 = v0 - mean, d1 = v1 - mean;
  const float rstd = 1.f / sqrtf(wave_sum(d0 * d0 + d1 * d1) * (1.f / MP_H) + 1e-5f);
  x[lane] = d0 * rstd * g[lane] + b[lane], x[lane + 64] = d1 * rstd * g[lane + 64] + b[lane + 64];
}

// one 128-column chunk of the tile: row k < K takes src(k)[0 .. 128) (NULL: zeros), rows K .. 63 are zero
template <class F>
__device__ __forceinline__ void mp_stage(float* tile, int K, int tid, F&& src) {
  const int c = tid & (MP_H - 1);
  for (int k = tid >> 7; k < MP_ROWS; k += 2) {
    const float* p = k < K ? src(k) : nullptr;
    tile[k * MP_LD + c] = p ? p[c] : 0.f;
  }
}

// the three-layer message function over a tile whose first layer's chunks come from stage(chunk): leaves W3 h + b3 in the tile
template <int CHUNKS, class F>
__device__ __forceinline__ void mp_message(float* tile, int K, const float* __restrict__ W1, const float* __restrict__ b1, const float* __restrict__ W2,
                                           const float* __restrict__ b2, const float* __restrict__ W3, const float* __restrict__ b3, int tid, F&& stage) {
  const int lane = tid & 63, wave = tid >> 6;
  MpAcc c;
  mp_zero(c);
  for (int ch = 0; ch < CHUNKS; ++ch) {
    __syncthreads();  // the tile's last readers are done
    stage(ch);
    __syncthreads();
    mp_mma(c, tile, W1 + (long)ch * MP_H * MP_H, MP_H, wave, lane);
  }
  __syncthreads();
  mp_store(c, tile, wave, lane, [&](float v, int col) { return mp_gelu(v + b1[col]); });
  __syncthreads();
  mp_zero(c);
  mp_mma(c, tile, W2, MP_H, wave, lane);
  __syncthreads();
  mp_store(c, tile, wave, lane, [&](float v, int col) { return mp_gelu(v + b2[col]); });
  __syncthreads();
  mp_zero(c);
  mp_mma(c, tile, W3, MP_H, wave, lane);
  __syncthreads();
  mp_store(c, tile, wave, lane, [&](float v, int col) { return v + b3[col]; });
  __syncthreads();
}

// The node tail of an encoder or decoder layer: x = vi + sum_k w_k tile[k] / 30, LN1, FFN 128-512-128, LN2, times `rowmask`; the new
// vector is left in vi (LDS).  wk == NULL: every slot counts 1 (the decoder).  hid: 512 + 256 floats of LDS.
__device__ __forceinline__ void mp_node_tail(const float* tile, int K, const float* wk, float* vi, float* hid, const float* __restrict__ ln1g,
                                             const float* __restrict__ ln1b, const float* __restrict__ Win, const float* __restrict__ bin,
                                             const float* __restrict__ Wout, const float* __restrict__ bout, const float* __restrict__ ln2g,
                                             const float* __restrict__ ln2b, float rowmask, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  if (tid < MP_H) {
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += (wk ? wk[k] : 1.f) * tile[k * MP_LD + tid];
    vi[tid] += s / 30.f;
  }
  __syncthreads();
  if (wave == 0) mp_ln(vi, ln1g, ln1b, lane);
  __syncthreads();
  for (int o = tid; o < 512; o += FD_THREADS) {
    float s = bin[o];
    for (int k = 0; k < MP_H; ++k) s += vi[k] * Win[k * 512 + o];
    hid[o] = mp_gelu(s);
  }
  __syncthreads();
  {
    const int c = tid & (MP_H - 1), half = tid >> 7;
    float s = 0.f;
    for (int k = half * 256; k < half * 256 + 256; ++k) s += hid[k] * Wout[k * MP_H + c];
    hid[512 + tid] = s;
  }
  __syncthreads();
  if (tid < MP_H) vi[tid] += bout[tid] + hid[512 + tid] + hid[512 + MP_H + tid];
  __syncthreads();
  if (wave == 0) {
    mp_ln(vi, ln2g, ln2b, lane);
    vi[lane] *= rowmask, vi[lane + 64] *= rowmask;
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------ features
__device__ __constant__ signed char mp_pair_a[25] = {1, 0, 2, 3, 4, 1, 1, 1, 1, 0, 0, 0, 4, 4, 3, 0, 2, 3, 4, 2, 3, 4, 2, 3, 2};
__device__ __constant__ signed char mp_pair_b[25] = {1, 0, 2, 3, 4, 0, 2, 3, 4, 2, 3, 4, 2, 3, 2, 1, 1, 1, 1, 0, 0, 0, 4, 4, 3};

// N, CA, C, O and the rebuilt CB of a row into out[15]
__device__ __forceinline__ void mp_atoms(const float* __restrict__ row, float* out) {
  float n[3], ca[3], c[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) n[d] = row[d], ca[d] = row[3 + d], c[d] = row[6 + d], out[d] = n[d], out[3 + d] = ca[d], out[6 + d] = c[d], out[9 + d] = row[12 + d];
  const float b[3] = {ca[0] - n[0], ca[1] - n[1], ca[2] - n[2]}, cc[3] = {c[0] - ca[0], c[1] - ca[1], c[2] - ca[2]};
  const float a[3] = {b[1] * cc[2] - b[2] * cc[1], b[2] * cc[0] - b[0] * cc[2], b[0] * cc[1] - b[1] * cc[0]};
#pragma unroll
  for (int d = 0; d < 3; ++d) out[12 + d] = -0.58273431f * a[d] + 0.56802827f * b[d] - 0.54067466f * cc[d] + ca[d];
}

// The neighbours of row i of backbone b, for both feature kernels.  ca: the CA of the backbone's row 0, stride: floats per row of prot.
// Leaves in LDS sel[k] (the column of slot k < K, nearest first, ties to the lower column), dnb[k] (its adjusted distance) and posd[k]
// (its positional class), writes E_idx and the row's share of status, and ends on a barrier.  dist: FDIPT_MPNN_MAX_ROWS floats, red: one
// per wave.
__device__ __forceinline__ void mp_neighbours(const MpCtx& x, const float* __restrict__ ca, int stride, long b, int i, float* dist, float* red,
                                              float* dnb, int* sel, int* posd, int* flag) {
  const FdiptMpnnArgs& a = x.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, N = a.N, K = x.K;
  const long bi = b * N + i;
  const float mi = a.res_mask[bi];
  if (tid < MP_ROWS) sel[tid] = tid < K ? tid : 0;  // in range whatever the distances are (NaN coordinates)
  if (tid == 0) *flag = 0;
  // D = mask_2D sqrt(|dCA|^2 + 1e-6), D_adjust = D + (1 - mask_2D) max_j D
  const float cx = ca[i * stride], cy = ca[i * stride + 1], cz = ca[i * stride + 2];
  float mx = 0.f;
  for (int j = tid; j < N; j += FD_THREADS) {
    const float dx = ca[j * stride] - cx, dy = ca[j * stride + 1] - cy, dz = ca[j * stride + 2] - cz;
    const float d = mi * a.res_mask[b * N + j] * sqrtf(dx * dx + dy * dy + dz * dz + 1e-6f);
    dist[j] = d, mx = fmaxf(mx, d);
  }
  mx = wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  for (int j = tid; j < N; j += FD_THREADS) dist[j] += (1.f - mi * a.res_mask[b * N + j]) * mx;
  __syncthreads();
  // the rank of column j under (distance, index); ranks below K are the neighbours, nearest first
  for (int j = tid; j < N; j += FD_THREADS) {
    const float dj = dist[j];
    int r = 0;
    for (int q = 0; q < N; ++q) {
      const float dq = dist[q];
      r += (dq < dj || (dq == dj && q < j)) ? 1 : 0;
    }
    if (r < K && dj == dj) sel[r] = j;
  }
  __syncthreads();
  if (tid < K) {
    const int j = sel[tid];
    dnb[tid] = dist[j];
    a.E_idx[bi * K + tid] = j;
    const int same = a.chain_idx[bi] == a.chain_idx[b * N + j];
    const int off = a.residue_index[bi] - a.residue_index[b * N + j];
    posd[tid] = same ? min(max(off + 32, 0), 64) : 65;
    if (mi != 0.f && a.res_mask[b * N + j] == 0.f) *flag = 1;
  }
  __syncthreads();
  if (tid == 0 && *flag) atomicOr(a.status + b, FDIPT_MPNN_MASKED_NEIGHBOR);
}

// norm_edges and W_e over the edge_embedding outputs in the accumulators -> h_E: the tail of both feature kernels
__device__ __forceinline__ void mp_edge_tail(const MpCtx& x, MpAcc& c, float* tile, long bi, int tid) {
  const int lane = tid & 63, wave = tid >> 6, K = x.K;
  __syncthreads();
  mp_store(c, tile, wave, lane, [](float v, int) { return v; });
  __syncthreads();
  for (int k = wave; k < K; k += FD_THREADS / FD_WAVE) mp_ln(tile + k * MP_LD, x.W(mpw::EDGE_G), x.W(mpw::EDGE_B), lane);
  __syncthreads();
  mp_zero(c);
  mp_mma(c, tile, x.W(mpw::WE_W), MP_H, wave, lane);
  const int col = wave * 32 + (lane & 31);
  const float bias = x.W(mpw::WE_B)[col];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = t * 32 + c_row(r, lane);
      if (k < K) x.hE[(bi * K + k) * MP_H + col] = c.t[t][r] + bias;
    }
}

__global__ __launch_bounds__(FD_THREADS) void mpnn_features_kernel(MpCtx x) {
  __shared__ float tile[MP_ROWS * MP_LD];
  __shared__ float dist[FDIPT_MPNN_MAX_ROWS];
  __shared__ float nb[MP_ROWS * 15], me[15], red[FD_THREADS / FD_WAVE], dnb[MP_ROWS];
  __shared__ int sel[MP_ROWS], posd[MP_ROWS], flag;
  const FdiptMpnnArgs& a = x.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, N = a.N, K = x.K, i = blockIdx.x, A3 = a.atoms * 3;
  const long b = blockIdx.y, bi = b * N + i;
  const float* __restrict__ W = a.weights;
  const float* prot = a.prot + b * N * A3;
  if (tid < MP_H) x.hV[0][bi * MP_H + tid] = 0.f;
  mp_neighbours(x, prot + 3, A3, b, i, dist, red, dnb, sel, posd, &flag);
  if (tid == 0) mp_atoms(prot + i * A3, me);
  if (tid < K) mp_atoms(prot + sel[tid] * A3, nb + tid * 15);
  // edge_embedding over the 416 inputs: 16 positional, then 25 pairs x 16 RBF centres
  MpAcc c;
  mp_zero(c);
  for (int f0 = 0; f0 < 416; f0 += MP_H) {
    const int kw = min(MP_H, 416 - f0);
    __syncthreads();
    for (int e = tid; e < MP_ROWS * kw; e += FD_THREADS) {
      const int k = e / kw, f = f0 + e % kw;
      float v = 0.f;
      if (k < K) {
        if (f < 16) {
          v = W[mpw::POS_W + posd[k] * 16 + f] + W[mpw::POS_B + f];
        } else {
          const int p = (f - 16) >> 4, ce = (f - 16) & 15;
          float d;
          if (p == 0) {
            d = dnb[k];
          } else {
            const float* pa = me + 3 * mp_pair_a[p];
            const float* pb = nb + k * 15 + 3 * mp_pair_b[p];
            const float dx = pa[0] - pb[0], dy = pa[1] - pb[1], dz = pa[2] - pb[2];
            d = sqrtf(dx * dx + dy * dy + dz * dz + 1e-6f);
          }
          const float z = (d - (2.f + ce * (20.f / 15.f))) / 1.25f;
          v = expf(-z * z);
        }
      }
      tile[k * MP_LD + (f - f0)] = v;
    }
    __syncthreads();
    mp_mma(c, tile, W + mpw::EDGE_W + (long)f0 * MP_H, kw, wave, lane);
  }
  mp_edge_tail(x, c, tile, bi, tid);
}

// ---- the CA-only features
// x0 y0 + x1 y1 + x2 y2 in ONE order of operations, so that swapping the operands gives the same bits: the self edge's R is symmetric
__device__ __forceinline__ float mp_dot3(float x0, float y0, float x1, float y1, float x2, float y2) { return fmaf(x2, y2, fmaf(x1, y1, x0 * y0)); }
// v / max(|v|, 1e-12)
__device__ __forceinline__ void mp_unit(float* v) {
  const float s = 1.f / fmaxf(sqrtf(mp_dot3(v[0], v[0], v[1], v[1], v[2], v[2])), 1e-12f);
  v[0] *= s, v[1] *= s, v[2] *= s;
}
// the kept unit step q - p: the zero vector unless 3.6 < |q - p| < 4.0
__device__ __forceinline__ void mp_step(const float* p, const float* q, float* u) {
  u[0] = q[0] - p[0], u[1] = q[1] - p[1], u[2] = q[2] - p[2];
  const float len = sqrtf(mp_dot3(u[0], u[0], u[1], u[1], u[2], u[2]));
  if (!(len > 3.6f && len < 4.0f)) u[0] = u[1] = u[2] = 0.f;
  mp_unit(u);
}
// The three shifted traces of row r into t[9] (Ca[r-1], Ca[r], Ca[r+1]; rows -1 and N are the zero vector) and its frame O[9] (rows
// o_1, n_2, o_1 x n_2; zero at row 0 and at rows N-2, N-1).  No read outside [0, N).
__device__ __forceinline__ void mp_ca_row(const float* __restrict__ ca, int stride, int N, int r, float* t, float* O) {
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int q = r - 1 + s;
    const bool in = q >= 0 && q < N;
#pragma unroll
    for (int d = 0; d < 3; ++d) t[3 * s + d] = in ? ca[(long)q * stride + d] : 0.f;
  }
#pragma unroll
  for (int e = 0; e < 9; ++e) O[e] = 0.f;
  if (r < 1 || r > N - 3) return;  // (rows r-1 and r+1 exist here)
  float u2[3], u1[3];
  mp_step(t, t + 3, u2);      // the step into the row
  mp_step(t + 3, t + 6, u1);  // the step out of it
  float* o1 = O;
  float* n2 = O + 3;
  float* o3 = O + 6;
  o1[0] = u2[0] - u1[0], o1[1] = u2[1] - u1[1], o1[2] = u2[2] - u1[2];
  mp_unit(o1);
  n2[0] = u2[1] * u1[2] - u2[2] * u1[1], n2[1] = u2[2] * u1[0] - u2[0] * u1[2], n2[2] = u2[0] * u1[1] - u2[1] * u1[0];
  mp_unit(n2);
  o3[0] = o1[1] * n2[2] - o1[2] * n2[1], o3[1] = o1[2] * n2[0] - o1[0] * n2[2], o3[2] = o1[0] * n2[1] - o1[1] * n2[0];
}
// (A of row i, B of neighbour j) of the nine RBF blocks: 0 = the row before, 1 = the row, 2 = the row after
__device__ __constant__ signed char mp_ca_pair_a[9] = {1, 0, 2, 0, 0, 1, 1, 2, 2};
__device__ __constant__ signed char mp_ca_pair_b[9] = {1, 0, 2, 1, 2, 0, 2, 0, 1};

__global__ __launch_bounds__(FD_THREADS) void mpnn_ca_features_kernel(MpCtx x) {
  __shared__ float tile[MP_ROWS * MP_LD];
  __shared__ float dist[FDIPT_MPNN_MAX_ROWS];
  __shared__ float nb[MP_ROWS * 9], of[MP_ROWS * 7], me[9], Oi[9], red[FD_THREADS / FD_WAVE], dnb[MP_ROWS];
  __shared__ int sel[MP_ROWS], posd[MP_ROWS], flag;
  const FdiptMpnnArgs& a = x.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, N = a.N, K = x.K, i = blockIdx.x, A3 = a.atoms * 3;
  const long b = blockIdx.y, bi = b * N + i;
  const float* __restrict__ W = a.weights;
  const float* ca = a.prot + b * N * A3 + (a.atoms == 1 ? 0 : 3);  // the trace alone, or atom 1 of either layout
  if (tid < MP_H) x.hV[0][bi * MP_H + tid] = 0.f;
  if (tid == 0) mp_ca_row(ca, A3, N, i, me, Oi);
  mp_neighbours(x, ca, A3, b, i, dist, red, dnb, sel, posd, &flag);  // (its barriers publish me and Oi)
  if (tid < K) {
    // the orientation inputs of slot tid: dU = unit(O_i (Ca_j - Ca_i)), Q of R = O_i^T O_j
    float Oj[9], dU[3], R[9], q[4];
    mp_ca_row(ca, A3, N, sel[tid], nb + tid * 9, Oj);
    if (sel[tid] == i)  // the self edge: the very values of O_i, so that R_ab and R_ba are the same operations on swapped operands
      for (int e = 0; e < 9; ++e) Oj[e] = Oi[e];
    const float* pj = nb + tid * 9 + 3;
    const float dx = pj[0] - me[3], dy = pj[1] - me[4], dz = pj[2] - me[5];
#pragma unroll
    for (int r = 0; r < 3; ++r) dU[r] = mp_dot3(Oi[3 * r], dx, Oi[3 * r + 1], dy, Oi[3 * r + 2], dz);
    mp_unit(dU);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int s = 0; s < 3; ++s) R[3 * r + s] = mp_dot3(Oi[r], Oj[s], Oi[3 + r], Oj[3 + s], Oi[6 + r], Oj[6 + s]);
    const float anti[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    const float diag[3] = {R[0] - R[4] - R[8], -R[0] + R[4] - R[8], -R[0] - R[4] + R[8]};
#pragma unroll
    for (int r = 0; r < 3; ++r) q[r] = (anti[r] > 0.f ? 1.f : anti[r] < 0.f ? -1.f : 0.f) * (0.5f * sqrtf(fabsf(1.f + diag[r])));
    q[3] = sqrtf(fmaxf(1.f + (R[0] + R[4] + R[8]), 0.f)) / 2.f;
    const float s = 1.f / fmaxf(sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), 1e-12f);
    float* o = of + tid * 7;
    o[0] = dU[0], o[1] = dU[1], o[2] = dU[2], o[3] = q[0] * s, o[4] = q[1] * s, o[5] = q[2] * s, o[6] = q[3] * s;
  }
  // edge_embedding over the 167 inputs: 16 positional, 9 pairs x 16 RBF centres, dU and Q; the second chunk is 39 columns and a zero one
  MpAcc c;
  mp_zero(c);
  for (int f0 = 0; f0 < (int)mpw::EDGE_IN_CA; f0 += MP_H) {
    const int kw = min(MP_H, ((int)mpw::EDGE_IN_CA - f0 + 1) & ~1);  // 128, then 40
    __syncthreads();
    for (int e = tid; e < MP_ROWS * kw; e += FD_THREADS) {
      const int k = e / kw, f = f0 + e % kw;
      float v = 0.f;
      if (k < K && f < (int)mpw::EDGE_IN_CA) {
        if (f < 16) {
          v = W[mpw::POS_W + posd[k] * 16 + f] + W[mpw::POS_B + f];
        } else if (f < 160) {
          const int p = (f - 16) >> 4, ce = (f - 16) & 15;
          float d;
          if (p == 0) {
            d = dnb[k];
          } else {
            const float* pa = me + 3 * mp_ca_pair_a[p];
            const float* pb = nb + k * 9 + 3 * mp_ca_pair_b[p];
            const float dx = pa[0] - pb[0], dy = pa[1] - pb[1], dz = pa[2] - pb[2];
            d = sqrtf(dx * dx + dy * dy + dz * dz + 1e-6f);
          }
          const float z = (d - (2.f + ce * (20.f / 15.f))) / 1.25f;
          v = expf(-z * z);
        } else {
          v = of[k * 7 + (f - 160)];
        }
      }
      tile[k * MP_LD + (f - f0)] = v;
    }
    __syncthreads();
    // an even number of whole steps, then (167 is odd) one step whose second weight row does not exist: its operand is the zero column
    const int whole = min(kw, ((int)mpw::EDGE_IN_CA - f0) & ~1);
    mp_mma(c, tile, W + mpw::EDGE_W + (long)f0 * MP_H, whole, wave, lane);
    if (whole < kw) {
      const int li = lane & 31, hi = lane >> 5;
      const float bw = hi ? 0.f : W[mpw::EDGE_W + (long)(f0 + whole) * MP_H + wave * 32 + li];
      c.t[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(tile[li * MP_LD + whole + hi], bw, c.t[0], 0, 0, 0);
      c.t[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(tile[(li + 32) * MP_LD + whole + hi], bw, c.t[1], 0, 0, 0);
    }
  }
  mp_edge_tail(x, c, tile, bi, tid);
}

// ------------------------------------------------------------------------------------------------ encoder
template <bool EDGE>
__global__ __launch_bounds__(FD_THREADS) void mpnn_enc_kernel(MpCtx x, int layer, int src) {
  __shared__ float tile[MP_ROWS * MP_LD];
  __shared__ float vi[MP_H], hid[512 + FD_THREADS], wk[MP_ROWS];
  __shared__ int sel[MP_ROWS];
  const FdiptMpnnArgs& a = x.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, N = a.N, K = x.K, i = blockIdx.x;
  const long b = blockIdx.y, bi = b * N + i;
  const float* __restrict__ W = x.W(mpw::ENC0 + layer * mpw::E_SIZE);
  const float* hV = x.hV[src] + b * N * MP_H;  // node update: the layer's input; edge update: the layer's new h_V
  float* hE = x.hE + bi * K * MP_H;
  const float mi = a.res_mask[bi];
  if (tid < MP_H) vi[tid] = hV[(long)i * MP_H + tid];
  if (tid < MP_ROWS) {
    const int j = tid < K ? a.E_idx[bi * K + tid] : 0;
    sel[tid] = j, wk[tid] = tid < K ? mi * a.res_mask[b * N + j] : 0.f;
  }
  __syncthreads();
  auto stage = [&](int ch) {
    mp_stage(tile, K, tid, [&](int k) -> const float* { return ch == 0 ? vi : ch == 1 ? hE + k * MP_H : hV + (long)sel[k] * MP_H; });
  };
  if (!EDGE) {
    mp_message<3>(tile, K, W + mpw::E_W1, W + mpw::E_B1, W + mpw::E_W2, W + mpw::E_B2, W + mpw::E_W3, W + mpw::E_B3, tid, stage);
    mp_node_tail(tile, K, wk, vi, hid, W + mpw::E_LN1G, W + mpw::E_LN1B, W + mpw::E_WIN, W + mpw::E_BIN, W + mpw::E_WOUT, W + mpw::E_BOUT,
                 W + mpw::E_LN2G, W + mpw::E_LN2B, mi, tid);
    if (tid < MP_H) x.hV[src ^ 1][bi * MP_H + tid] = vi[tid];
  } else {
    mp_message<3>(tile, K, W + mpw::E_W11, W + mpw::E_B11, W + mpw::E_W12, W + mpw::E_B12, W + mpw::E_W13, W + mpw::E_B13, tid, stage);
    const int c = tid & (MP_H - 1);
    for (int k = tid >> 7; k < K; k += 2) tile[k * MP_LD + c] += hE[k * MP_H + c];
    __syncthreads();
    for (int k = wave; k < K; k += FD_THREADS / FD_WAVE) mp_ln(tile + k * MP_LD, W + mpw::E_LN3G, W + mpw::E_LN3B, lane);
    __syncthreads();
    for (int k = tid >> 7; k < K; k += 2) hE[k * MP_H + c] = tile[k * MP_LD + c];
  }
}

// ------------------------------------------------------------------------------------------------ decoder
// One decoder layer of row i of sequence (b, m).  vi (LDS) holds h_V^layer_i on entry and h_V^(layer+1)_i on return.  A neighbour j
// decoded before i contributes [h_E, W_s[letter_j], h_V^layer_j], any other [h_E, 0, h_V^enc_j].  letter(j) reads the sequence.
// lettered[k] says whether the letter of a `before` neighbour is known: always, except for the earlier members of a tied group still
// open, which give [h_E, 0, h_V^layer_j] (tied_sample writes a group's letter after its last member).
template <class L>
__device__ __forceinline__ void mp_dec_layer(const MpCtx& x, int layer, long b, long bm, int i, float* tile, float* vi, float* hid, const int* sel,
                                             const int* before, const int* lettered, int tid, L&& letter) {
  const FdiptMpnnArgs& a = x.a;
  const int N = a.N, K = x.K;
  const float* __restrict__ W = x.W(mpw::DEC0 + layer * mpw::D_SIZE);
  const float* Ws = x.W(mpw::WS);
  const float* hE = x.hE + (b * N + i) * K * MP_H;
  const float* enc = x.hV[1] + b * N * MP_H;
  const long BMN = (long)a.B * a.M * N;
  const float* cur = layer == 0 ? enc : x.stack + ((layer - 1) * BMN + bm * N) * MP_H;
  auto stage = [&](int ch) {
    mp_stage(tile, K, tid, [&](int k) -> const float* {
      const int j = sel[k];
      return ch == 0 ? vi : ch == 1 ? hE + k * MP_H : ch == 2 ? (lettered[k] ? Ws + letter(j) * MP_H : nullptr) : (before[k] ? cur : enc) + (long)j * MP_H;
    });
  };
  mp_message<4>(tile, K, W + mpw::D_W1, W + mpw::D_B1, W + mpw::D_W2, W + mpw::D_B2, W + mpw::D_W3, W + mpw::D_B3, tid, stage);
  mp_node_tail(tile, K, nullptr, vi, hid, W + mpw::D_LN1G, W + mpw::D_LN1B, W + mpw::D_WIN, W + mpw::D_BIN, W + mpw::D_WOUT, W + mpw::D_BOUT,
               W + mpw::D_LN2G, W + mpw::D_LN2B, 1.f, tid);
  if (tid < MP_H) x.stack[(layer * BMN + bm * N + i) * MP_H + tid] = vi[tid];
}

// logits[a] = W_out vi + b into lg[21] (LDS)
__device__ __forceinline__ void mp_logits(const MpCtx& x, const float* vi, float* lg, int tid) {
  const float* __restrict__ Wo = x.W(mpw::OUT_W);
  const float* __restrict__ bo = x.W(mpw::OUT_B);
  if (tid < MP_V) {
    float s = bo[tid];
    for (int k = 0; k < MP_H; ++k) s += vi[k] * Wo[k * MP_V + tid];
    lg[tid] = s;
  }
  __syncthreads();
}

__device__ __forceinline__ int mp_letter(int s) { return min(max(s, 0), MP_V - 1); }

// pos[b,m,row] = the step at which the row is decoded; N where decoding_order never names it
__global__ __launch_bounds__(FD_THREADS) void mpnn_order_kernel(MpCtx x) {
  const int N = x.a.N;
  const long bm = blockIdx.x;
  for (int t = threadIdx.x; t < N; t += FD_THREADS) x.pos[bm * N + t] = N;
  __syncthreads();
  for (int t = threadIdx.x; t < N; t += FD_THREADS) {
    const int i = x.a.decoding_order[bm * N + t];
    if (i >= 0 && i < N) x.pos[bm * N + i] = t;
  }
}

__global__ __launch_bounds__(FD_THREADS) void mpnn_score_kernel(MpCtx x, int layer) {
  __shared__ float tile[MP_ROWS * MP_LD];
  __shared__ float vi[MP_H], hid[512 + FD_THREADS], lg[MP_V];
  __shared__ int sel[MP_ROWS], before[MP_ROWS];
  const FdiptMpnnArgs& a = x.a;
  const int tid = threadIdx.x, N = a.N, K = x.K, i = blockIdx.x;
  const long b = blockIdx.z, bm = b * a.M + blockIdx.y, bi = b * N + i;
  const long BMN = (long)a.B * a.M * N;
  if (a.res_mask[bi] == 0.f) {  // the reference's mask_V: zeros in every layer; log-probabilities 0 by this project's rule
    if (tid < MP_H) x.stack[(layer * BMN + bm * N + i) * MP_H + tid] = 0.f;
    if (layer == 2 && tid < MP_V) a.log_probs[(bm * N + i) * MP_V + tid] = 0.f;
    return;
  }
  const int* pos = x.pos + bm * N;
  const int* S = a.S + bm * N;
  if (tid < MP_H) vi[tid] = (layer == 0 ? x.hV[1] + bi * MP_H : x.stack + ((layer - 1) * BMN + bm * N + i) * MP_H)[tid];
  if (tid < MP_ROWS) {
    const int j = tid < K ? a.E_idx[bi * K + tid] : 0;
    sel[tid] = j, before[tid] = !a.unconditional && tid < K && pos[j] < pos[i];  // unconditional: pos and S are never read
  }
  __syncthreads();
  mp_dec_layer(x, layer, b, bm, i, tile, vi, hid, sel, before, before, tid, [&](int j) { return mp_letter(S[j]); });
  if (layer != 2) return;
  mp_logits(x, vi, lg, tid);
  if (tid == 0) {
    float mx = lg[0], s = 0.f;
    for (int q = 1; q < MP_V; ++q) mx = fmaxf(mx, lg[q]);
    for (int q = 0; q < MP_V; ++q) s += expf(lg[q] - mx);
    const float lse = mx + logf(s);
    for (int q = 0; q < MP_V; ++q) a.log_probs[(bm * N + i) * MP_V + q] = lg[q] - lse;
  }
}

// Tied positions: consecutive steps whose rows carry the same tie_group id >= 0 are one group, steps t0 .. gend-1.
// Each member runs the decoder (earlier members count as before, without a letter), the members' logits are summed with their weights
// into acc[], and the sampling epilogue runs once, at the last member, whose controls and uniform it reads.  A group's extent comes from
// a forward scan of the order at its first step, bounded by N, so no step waits for anything and a malformed order gives defined output.
__global__ __launch_bounds__(FD_THREADS) void mpnn_design_kernel(MpCtx x) {
  __shared__ float tile[MP_ROWS * MP_LD];
  __shared__ float vi[MP_H], hid[512 + FD_THREADS], lg[MP_V], acc[MP_V];
  __shared__ int sel[MP_ROWS], before[MP_ROWS], lettered[MP_ROWS];
  __shared__ unsigned char S[FDIPT_MPNN_MAX_ROWS];      // the sequence so far: written and read by this block only
  __shared__ unsigned char known[FDIPT_MPNN_MAX_ROWS];  // the row's letter is assigned (rows without res_mask: from the start)
  const FdiptMpnnArgs& a = x.a;
  const int tid = threadIdx.x, N = a.N, K = x.K;
  const long b = blockIdx.y, bm = b * a.M + blockIdx.x;
  const long BMN = (long)a.B * a.M * N;
  const int* pos = x.pos + bm * N;
  const int* order = a.decoding_order + bm * N;
  for (int j = tid; j < N; j += FD_THREADS) S[j] = (unsigned char)mp_letter(a.S[bm * N + j]), known[j] = a.res_mask[b * N + j] == 0.f;
  __syncthreads();
  // the tie id of step s: -1 for an untied row and for a step that decodes nothing (past the end, out of range, named twice, no res_mask)
  auto tie_at = [&](int s) -> int {
    if (!a.tie_group || s >= N) return -1;
    const int r = order[s];
    if (r < 0 || r >= N || pos[r] != s || a.res_mask[b * N + r] == 0.f) return -1;
    return a.tie_group[b * N + r];
  };
  int t0 = 0, gend = 0;  // the last group opened
  for (int t = 0; t < N; ++t) {  // the loop bound is N for every block; nothing here waits on another block
    const int i = order[t];
    if (i < 0 || i >= N || pos[i] != t) continue;  // not a permutation: the row is never decoded and keeps its input letter
    const long bi = b * N + i;
    if (a.res_mask[bi] == 0.f) {
      for (int l = 0; l < 3; ++l)
        if (tid < MP_H) x.stack[(l * BMN + bm * N + i) * MP_H + tid] = 0.f;
      if (tid < MP_V) a.probs[(bm * N + i) * MP_V + tid] = 0.f;
      continue;
    }
    const bool tied = tie_at(t) >= 0;
    if (tied && t >= gend) {
      const int g = tie_at(t);
      t0 = t, gend = t + 1;
      while (tie_at(gend) == g) ++gend;
      if (tid < MP_V) acc[tid] = 0.f;  // (the threads that add to it)
    }
    if (tid < MP_H) vi[tid] = x.hV[1][bi * MP_H + tid];
    if (tid < MP_ROWS) {
      const int j = tid < K ? a.E_idx[bi * K + tid] : 0;
      sel[tid] = j, before[tid] = tid < K && pos[j] < t, lettered[tid] = before[tid] && known[j];
    }
    __syncthreads();
    for (int l = 0; l < 3; ++l) {
      mp_dec_layer(x, l, b, bm, i, tile, vi, hid, sel, before, lettered, tid, [&](int j) { return (int)S[j]; });
      __threadfence();  // the row of the stack is read back by later steps of this block
      __syncthreads();
    }
    mp_logits(x, vi, lg, tid);
    if (tied) {
      if (tid < MP_V) acc[tid] += a.tied_beta[bi] * (lg[tid] / a.temperature) / (float)(gend - t0);
      __syncthreads();
      if (t + 1 < gend) continue;  // the same for every thread: the group's letter comes with its last member
    }
    if (tid == 0) {
      const float T = a.temperature;
      float z[MP_V], mx = -INFINITY, sum = 0.f;
      if (tied) {
        for (int q = 0; q < MP_V; ++q) z[q] = acc[q] - a.omit[q] * 1e8f + a.bias[q] / T;
      } else {
        for (int q = 0; q < MP_V; ++q) z[q] = lg[q] / T - a.omit[q] * 1e8f + a.bias[q] / T;
      }
      if (a.bias_by_res)
        for (int q = 0; q < MP_V; ++q) z[q] += a.bias_by_res[bi * MP_V + q] / T;
      for (int q = 0; q < MP_V; ++q) mx = fmaxf(mx, z[q]);
      for (int q = 0; q < MP_V; ++q) z[q] = expf(z[q] - mx), sum += z[q];
      float total = 0.f;
      for (int q = 0; q < MP_V; ++q) z[q] = z[q] / sum, total += z[q];
      // the stages of the reference's flags, each only where its array is present
      const bool staged = a.pssm_bias || a.pssm_log_odds_mask || a.omit_mask;
      bool none = false;
      if (a.pssm_bias) {
        const float c = a.pssm_multi * a.pssm_coef[bi];
        for (int q = 0; q < MP_V; ++q) z[q] = (1.f - c) * z[q] + c * a.pssm_bias[bi * MP_V + q];
      }
      if (a.pssm_log_odds_mask) {
        float s = 0.f;
        for (int q = 0; q < MP_V; ++q) z[q] = z[q] * a.pssm_log_odds_mask[bi * MP_V + q] + z[q] * 0.001f, s += z[q];
        if (s > 0.f) {
          for (int q = 0; q < MP_V; ++q) z[q] = z[q] / s;
        } else {
          none = true;
        }
      }
      if (a.omit_mask) {
        float s = 0.f;
        for (int q = 0; q < MP_V; ++q) z[q] = z[q] * (1.f - a.omit_mask[bi * MP_V + q]), s += z[q];
        if (s > 0.f) {
          for (int q = 0; q < MP_V; ++q) z[q] = z[q] / s;
        } else {
          none = true;
        }
      }
      if (staged) {
        total = 0.f;
        for (int q = 0; q < MP_V; ++q) total += z[q];
      }
      // the first letter whose cumulative probability exceeds u * total; else the last letter with p > 0
      const float thr = a.u[bm * N + i] * total;
      int pick = -1, last = -1;
      float cum = 0.f;
      for (int q = 0; q < MP_V; ++q) {
        cum += z[q];
        if (z[q] > 0.f) last = q;
        if (pick < 0 && cum > thr) pick = q;
      }
      if (staged && last < 0) none = true;  // no letter left: the rows keep their input letters, probs 0
      if (pick < 0) pick = max(last, 0);
      if (none) atomicOr(a.status + b, FDIPT_MPNN_NO_LETTER);
      for (int s = tied ? t0 : t; s <= t; ++s) {  // every member takes the letter and the distribution
        const int r = s == t ? i : order[s];
        const float cm = a.chain_mask[b * N + r];
        float* pr = a.probs + (bm * N + r) * MP_V;
        if (cm != 0.f && !none) S[r] = (unsigned char)pick;
        known[r] = 1;
        for (int q = 0; q < MP_V; ++q) pr[q] = none ? 0.f : cm * z[q];
      }
    }
    __syncthreads();
  }
  for (int j = tid; j < N; j += FD_THREADS) a.S_out[bm * N + j] = S[j];
}

// ------------------------------------------------------------------------------------------------ host
static bool mp_dims_ok(const FdiptMpnnDims* d) {
  return d && d->hidden == MP_H && d->enc_layers == 3 && d->dec_layers == 3 && d->vocab == MP_V && d->k_neighbors >= 1 &&
         d->k_neighbors <= FDIPT_MPNN_MAX_NEIGHBORS && (d->ca_only == 0 || d->ca_only == 1);
}

extern "C" int64_t fdipt_mpnn_weights_floats(const FdiptMpnnDims* dims) {
  return mp_dims_ok(dims) ? (int64_t)(mpw::TOTAL - (dims->ca_only ? mpw::CA_SHIFT : 0)) : FDIPT_EINVAL;
}

// h_E, the encoder's two h_V, the three decoder outputs per sequence (floats), then the decoding steps (i32)
extern "C" size_t fdipt_mpnn_workspace(const FdiptMpnnDims* dims, int B, int N, int M) {
  if (!mp_dims_ok(dims) || B < 1 || N < 1 || M < 1) return 0;
  const size_t K = (size_t)(dims->k_neighbors < N ? dims->k_neighbors : N), bn = (size_t)B * N;
  return 4 * (bn * K * MP_H + 2 * bn * MP_H + 3 * bn * M * MP_H + bn * M);
}

static int mp_prepare(const FdiptMpnnDims* dims, const FdiptMpnnArgs* a, bool design, MpCtx& x) {
  if (!a || !mp_dims_ok(dims) || a->B < 1 || a->N < 1 || a->M < 1) return FDIPT_EINVAL;
  if (a->atoms != 37 && a->atoms != 5 && !(dims->ca_only && a->atoms == 1)) return FDIPT_EINVAL;
  if (dims->ca_only && a->N < 3) return FDIPT_EINVAL;  // the frames need three rows (the reference raises)
  if (!a->weights || !a->prot || !a->res_mask || !a->residue_index || !a->chain_idx || !a->E_idx || !a->status) return FDIPT_EINVAL;
  if ((design || !a->unconditional) && (!a->S || !a->decoding_order)) return FDIPT_EINVAL;
  if (design ? (!a->chain_mask || !a->u || !a->omit || !a->bias || !a->S_out || !a->probs || !(a->temperature > 0.f)) : !a->log_probs) return FDIPT_EINVAL;
  if (design && (((a->pssm_bias || a->pssm_log_odds_mask) && !a->pssm_coef) || (a->tie_group && !a->tied_beta))) return FDIPT_EINVAL;
  if (a->N > FDIPT_MPNN_MAX_ROWS || a->M > FDIPT_MPNN_MAX_SEQ || a->B > 65535) return FDIPT_ESIZE;  // (B is a grid's y / z extent)
  if (!a->workspace || a->workspace_bytes < fdipt_mpnn_workspace(dims, a->B, a->N, a->M)) return FDIPT_ESIZE;
  x.a = *a;
  if (design) x.a.unconditional = 0;
  else if (x.a.unconditional) x.a.decoding_order = nullptr, x.a.S = nullptr;
  x.K = dims->k_neighbors < a->N ? dims->k_neighbors : a->N;
  x.shift = dims->ca_only ? mpw::CA_SHIFT : 0;
  const size_t bn = (size_t)a->B * a->N;
  x.hE = (float*)a->workspace;
  x.hV[0] = x.hE + bn * x.K * MP_H;
  x.hV[1] = x.hV[0] + bn * MP_H;
  x.stack = x.hV[1] + bn * MP_H;
  x.pos = (int32_t*)(x.stack + 3 * bn * a->M * MP_H);
  return FDIPT_OK;
}

// features, the three encoder layers (the result ends in hV[1]) and the decoding steps
static int mp_encode(const MpCtx& x, hipStream_t s) {
  const dim3 rows((unsigned)x.a.N, (unsigned)x.a.B);
  if (hipMemsetAsync(x.a.status, 0, sizeof(int32_t) * x.a.B, s) != hipSuccess) return FDIPT_ELAUNCH;
  if (x.shift) hipLaunchKernelGGL(mpnn_ca_features_kernel, rows, dim3(FD_THREADS), 0, s, x);
  else hipLaunchKernelGGL(mpnn_features_kernel, rows, dim3(FD_THREADS), 0, s, x);
  FD_CHECK_LAUNCH();
  for (int l = 0; l < 3; ++l) {
    const int src = l & 1;  // 0 -> 1, 1 -> 0, 0 -> 1
    hipLaunchKernelGGL(mpnn_enc_kernel<false>, rows, dim3(FD_THREADS), 0, s, x, l, src);
    FD_CHECK_LAUNCH();
    hipLaunchKernelGGL(mpnn_enc_kernel<true>, rows, dim3(FD_THREADS), 0, s, x, l, src ^ 1);
    FD_CHECK_LAUNCH();
  }
  if (!x.a.decoding_order) return FDIPT_OK;  // the unconditional score: no order
  hipLaunchKernelGGL(mpnn_order_kernel, dim3((unsigned)(x.a.B * x.a.M)), dim3(FD_THREADS), 0, s, x);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}

extern "C" int fdipt_mpnn_score(const FdiptMpnnDims* dims, const FdiptMpnnArgs* args, fdipt_stream_t stream) {
  MpCtx x;
  int rc = mp_prepare(dims, args, false, x);
  if (rc != FDIPT_OK) return rc;
  if ((rc = mp_encode(x, (hipStream_t)stream)) != FDIPT_OK) return rc;
  for (int l = 0; l < 3; ++l) {
    hipLaunchKernelGGL(mpnn_score_kernel, dim3((unsigned)x.a.N, (unsigned)x.a.M, (unsigned)x.a.B), dim3(FD_THREADS), 0, (hipStream_t)stream, x, l);
    FD_CHECK_LAUNCH();
  }
  return FDIPT_OK;
}

extern "C" int fdipt_mpnn_design(const FdiptMpnnDims* dims, const FdiptMpnnArgs* args, fdipt_stream_t stream) {
  MpCtx x;
  int rc = mp_prepare(dims, args, true, x);
  if (rc != FDIPT_OK) return rc;
  if ((rc = mp_encode(x, (hipStream_t)stream)) != FDIPT_OK) return rc;
  hipLaunchKernelGGL(mpnn_design_kernel, dim3((unsigned)x.a.M, (unsigned)x.a.B), dim3(FD_THREADS), 0, (hipStream_t)stream, x);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
