// model.hip — parameter inventory, derived-weight preparation and the score-network forward schedule.
//
// fdipt_score_forward is the device-side replacement of ScoreNetwork.forward
// (framedipt/model/score_network.py:218-275) = Embedder.forward (:129-197) + IpaScore.forward
// (framedipt/model/ipa_pytorch.py:509-572).  It only enqueues kernels on the caller's stream: no allocation,
// no synchronisation, no host round-trip (the reference syncs inside the forward, so3_diffuser.py:398).
#include <math.h>
#include <string.h>

#include <vector>

#include "common.hpp"
#include "kernels.hpp"

// ------------------------------------------------------------------ inventory (== framedipt_amd/weights.py)
struct LinW { long w, b; int out, in; };
struct LNW { long g, b; int d; };
#define FD_MAX_BLOCKS 8
#define FD_MAX_TL 4
struct TfLayer { LinW inp, outp, l1, l2; LNW n1, n2; };
struct BlockW {
  long head_w;
  LinW q, kv, qp, kvp, lb, dz, out, rbf;
  LNW ipa_ln;
  LinW skip;
  TfLayer tf[FD_MAX_TL];
  LinW post, t1, t2, t3;
  LNW tln;
  LinW bb;
  LinW et_init, et1, et2, etf;
  LNW et_ln;
};
struct Inventory {
  LinW ne0, ne2, ne4; LNW neln;
  LinW ee0, ee2, ee4; LNW eeln;
  BlockW blk[FD_MAX_BLOCKS];
  LinW tor1, tor2, tor3, torf;
  std::vector<long> offsets;  // per tensor, in state_dict order; back() = total
  int d1, node_in, edge_in, d_t, cb, hid, feat_dim, proj_out;
};

// The half-precision mode of the build, or fp16x (FDIPT_PREC_F16X: the fp16 mode with split terms in the pair path; the default
// build only).  Every choice of the half-precision mode goes by half_mode; what fp16x adds goes by ForwardPlan::x and the blob's
// et4x_stream.  op_precision: the operand precision the kernels see (fp16x runs the fp16 kernels).
static bool half_mode(const FdiptDims* d) {
  return d->precision == FDIPT_PREC_HALF || (FDIPT_PREC_HALF == FDIPT_PREC_F16 && d->precision == FDIPT_PREC_F16X);
}
static int op_precision(const FdiptDims* d) { return half_mode(d) ? FDIPT_PREC_HALF : d->precision; }

static bool dims_ok(const FdiptDims* d) {
  return d && d->num_blocks >= 1 && d->num_blocks <= FD_MAX_BLOCKS && d->tfmr_layers >= 1 && d->tfmr_layers <= FD_MAX_TL &&
         d->c_s > 0 && (d->c_s % 8) == 0 && d->c_z > 0 && (d->c_z % 8) == 0 && d->no_heads > 0 && d->no_heads <= 16 &&
         d->index_embed == 32 && d->num_bins >= 0 && d->num_bins < 64 && (d->c_skip % 8) == 0 &&
         (d->precision == FDIPT_PREC_F32 || half_mode(d)) && (d->kernel_flags & ~FDIPT_KF_ALL) == 0;
}

static void build_inventory(const FdiptDims* d, Inventory& iv) {
  long off = 0;
  iv.offsets.clear();
  auto push = [&](long n) { iv.offsets.push_back(off); long o = off; off += n; return o; };
  auto lin = [&](int out, int in) { LinW l; l.out = out; l.in = in; l.w = push((long)out * in); l.b = push(out); return l; };
  auto ln = [&](int dd) { LNW l; l.d = dd; l.g = push(dd); l.b = push(dd); return l; };
  const int E = d->index_embed;
  iv.d1 = E + 1 + (d->use_aatype ? 21 : 0);
  iv.node_in = iv.d1 + E;
  iv.edge_in = 2 * iv.d1 + E + d->num_bins;
  const int cs = d->c_s, cz = d->c_z, H = d->no_heads, C = d->c_hidden, Pq = d->no_qk_points, Pv = d->no_v_points;
  iv.d_t = cs + d->c_skip;
  iv.cb = cs / 2;
  iv.hid = 2 * iv.cb + cz;
  iv.feat_dim = H * (cz / 4 + C + Pv * 4);
  iv.proj_out = 3 * H * C + 3 * H * Pq + 3 * H * (Pq + Pv);
  iv.ne0 = lin(cs, iv.node_in); iv.ne2 = lin(cs, cs); iv.ne4 = lin(cs, cs); iv.neln = ln(cs);
  iv.ee0 = lin(cz, iv.edge_in); iv.ee2 = lin(cz, cz); iv.ee4 = lin(cz, cz); iv.eeln = ln(cz);
  for (int b = 0; b < d->num_blocks; ++b) {
    BlockW& k = iv.blk[b];
    k.head_w = push(H);
    k.q = lin(H * C, cs); k.kv = lin(2 * H * C, cs); k.qp = lin(H * Pq * 3, cs); k.kvp = lin(H * (Pq + Pv) * 3, cs);
    k.lb = lin(H, cz); k.dz = lin(cz / 4, cz); k.out = lin(cs, iv.feat_dim); k.rbf = lin(1, 20);
    k.ipa_ln = ln(cs);
    k.skip = lin(d->c_skip, cs);
    for (int l = 0; l < d->tfmr_layers; ++l) {
      TfLayer& t = k.tf[l];
      t.inp = lin(3 * iv.d_t, iv.d_t); t.outp = lin(iv.d_t, iv.d_t); t.l1 = lin(iv.d_t, iv.d_t); t.l2 = lin(iv.d_t, iv.d_t);
      t.n1 = ln(iv.d_t); t.n2 = ln(iv.d_t);
    }
    k.post = lin(cs, iv.d_t);
    k.t1 = lin(cs, cs); k.t2 = lin(cs, cs); k.t3 = lin(cs, cs); k.tln = ln(cs);
    k.bb = lin(6, cs);
    if (b < d->num_blocks - 1) {
      k.et_init = lin(iv.cb, cs); k.et1 = lin(iv.hid, iv.hid); k.et2 = lin(iv.hid, iv.hid); k.etf = lin(cz, iv.hid);
      k.et_ln = ln(cz);
    }
  }
  iv.tor1 = lin(cs, cs); iv.tor2 = lin(cs, cs); iv.tor3 = lin(cs, cs); iv.torf = lin(2, cs);
  iv.offsets.push_back(off);
}

// ------------------------------------------------------------------ derived blob layout
static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
static inline int rup8(int x) { return (x + 7) & ~7; }

// A run: images reserved back to back, which an L2 warm-up touches as one range from its first member; *_run is its length in bytes
struct DSplit {  // lo images (W - half(W)) of the node-path layers that run on split operands (rowblock.hip, attention_seq.hip)
  size_t inp[FD_MAX_TL], outp[FD_MAX_TL], l1[FD_MAX_TL], l2[FD_MAX_TL], post, t1, t2, t3, et_init, r4w;
  // 16-row images (fd_chain_build_image16) of the tail's matrices, hi then lo: out_proj, FFN 1, FFN 2 per layer, post_tfmr
  size_t o16[FD_MAX_TL][2], f16[FD_MAX_TL][2], g16[FD_MAX_TL][2], p16[2];
  size_t tr16[3][2];  // ... of the transition's three matrices (transition16_kernel)
  size_t ei16[2], r416[2];  // ... of EdgeTransition's initial_embed and fold-row matrix r4w (rows folded into the transition launch)
  // runs, hi and lo alike: o16 | f16 | g16 of layer l (the last layer's ends with p16); tr16 t1 | t2 | t3; ei16 | r416; lo t1 | t2 | t3;
  // lo et_init | r4w
  unsigned tail16_run[FD_MAX_TL], tr16_run, et16_run, t_run, et_run;
};
struct DChain {  // weight images of the fused node-path chains (chain.hip, rowblock.hip: natural k order) of one trunk block
  size_t inp[FD_MAX_TL], outp[FD_MAX_TL], l1[FD_MAX_TL], l2[FD_MAX_TL], post, t1, t2, t3, et_init, a1af, b1f, r4w, r4b;
  unsigned t23_run;  // run t2 | t3
};
struct DBlock { size_t wq_m, wproj2_img, wproj2_img_lo, bproj2, wproj2p_img, wproj2p_img_lo, bproj2p, wout_m, bout_m, wout_img, wout_img_lo, wproj, wproj_img, wproj_img_lo, bproj, gamma, wb, bb, wb_img3, wb_img4, et3, et4, et4x, wdz_t, wdz_img, wdz_img_lo, wdz_imgp, wdz_imgp_lo; DChain ch; DSplit lo; };
struct DLayout {
  size_t h16_base;   // bf16 image of the whole fp32 blob (bf16 mode): element offset == fp32 element offset
  size_t ne0_pad;     // [cs, kn_pad] operand precision
  size_t w1i, w1j, w1r, dtab, edges, b1;  // fp32 pieces of the concat-free first edge-embedder layer
  size_t ee2;         // LDS images of edge-embedder layers 2/3 (register-resident bf16 kernel)
  size_t ee2x;        // fp16x: the same, followed by their lo images
  size_t ch_ne0, ch_ne2, ch_ne4, ch_tor1, ch_tor2;  // chain images: node embedder, torsion head
  size_t lo_ne0, lo_ne2, lo_ne4, lo_tor1, lo_tor2;  // lo images: node embedder, torsion head
  size_t skip16[2];                                 // ... of the stacked skip_embed matrices [num_blocks * c_skip = 256, c_s] (fused into the node embedder)
  size_t ne16[3][2], tor16[2][2];                   // 16-row images (fd_chain_build_image16; the embedder's first one zero-padded to K = 96), hi / lo
  unsigned lo_tor_run, ne16_run, tor16_run, skip16_run;  // runs: lo tor1 | tor2; ne16 hi or lo; tor16 hi or lo; skip16 hi | lo
  size_t skip_w32, skip_b;                          // skip_embed of ALL blocks stacked: [num_blocks * c_skip, c_s] fp32 (split operands: the GEMM
                                                    // splits both operands while it stages them), bias f32
  DBlock blk[FD_MAX_BLOCKS];
  size_t total;
  int kn_pad, d1_pad, esz;
};

// Conditional groups of derived images.  Each predicate decides both that blob_walk builds the group and that a path of
// plan_forward may read it.
// the register-resident half-precision pair kernels (edge_transition3/4.hip, edge_embed2) are compiled for the reference widths only:
// the edge embedder's LDS images, the EdgeTransition weight streams
static bool use_regpair(const FdiptDims* d) {
  return half_mode(d) && d->c_z == 128 && d->c_s == 256 && !(d->kernel_flags & FDIPT_KF_GENERIC_PAIR);
}
// fp16x: edge_transition4's weight stream with the final layer's lo fragments (fd_et4_build_stream lo = 1) in place of the plain one;
// no edge_transition3 stream (fp16x refuses every plan that would run it)
// The edge embedder's row table (edge_embed2.hip: fd_edge_embed2_table / fd_edge_embed2_spread).  Without aatype features the embedder's
// output for a pair is a function of (sample, fixed-mask bits of i and j, rel, bin): n_rel (num_bins + 1) rows per class pair and sample
// against N^2 pairs.  The static part of the predicate (dims, flags, shape) also decides the workspace region, which holds the four class
// pairs of a table of up to ee_table_max_rel(N) relative positions (a single chain has 2 N - 1; chain breaks add their gaps).
// EE_TABLE_CAP: bytes of one class pair's rows of the batch — the spread gathers them, so they should stay cache-resident next to the
// streams it writes (c4: 39 MB, measured).  Since the rows are shared among the samples of a group (one leader per group,
// decided on the device: embed_stage) a batch stepped at one t touches one sample's worth of the region; the sizes stay those of B leaders
#define EE_TABLE_ROW_BYTES 352
#define EE_TABLE_CAP (64L << 20)
static int ee_table_max_rel(int N) { return 5 * N / 2; }
static bool ee_table_rows_ok(int B, int N, int n_rel, int num_bins) {
  const long rows = (long)n_rel * (num_bins + 1);
  return rows <= (long)N * N / 2 && B * rows * EE_TABLE_ROW_BYTES <= EE_TABLE_CAP;
}
static bool ee_table_static(const FdiptDims* d, int B, int N) {
  const unsigned off = FDIPT_KF_UNFOLDED | FDIPT_KF_PASS_Z | FDIPT_KF_ET3 | FDIPT_KF_GENERIC_ATTN;
  if (!half_mode(d) || d->c_z != 128 || d->c_s != 256 || (d->kernel_flags & (FDIPT_KF_GENERIC_PAIR | off))) return false;
  return !d->use_aatype && d->num_bins > 0 && d->num_blocks >= 3 && N % 4 == 0 && ee_table_rows_ok(B, N, 2 * N - 1, d->num_bins);
}
static bool et4x_stream(const FdiptDims* d) { return use_regpair(d) && d->precision == FDIPT_PREC_F16X; }
// fp16x: the edge embedder's layer-2/3 images followed by their lo images (fd_ee2_build_images lo = 1) in place of the plain ones
static bool ee2x_images(const FdiptDims* d) { return use_regpair(d) && d->precision == FDIPT_PREC_F16X; }
// fused node-path kernels (chain.hip, rowblock.hip) are compiled for the reference widths only: their 32-row images, the lo images of
// split operands and the 16-row images.  (c_s 256, c_skip 64, c_z 128 fix d_t 320, cb 128, hid 384: the shapes of the 16-row kernels)
static bool use_chain(const FdiptDims* d) {
  return half_mode(d) && d->c_s == 256 && d->c_skip == 64 && d->c_z == 128 && !(d->kernel_flags & FDIPT_KF_UNFUSED_NODE);
}
// the stacked skip_embed matrices as 16-row images: a fourth layer of the 16-row node embedder, 256 rows
static bool skip16_image(const FdiptDims* d) { return use_chain(d) && d->num_blocks * d->c_skip == 256; }
// the fused IPA projection as fragment images, zero-padded to whole 128-column blocks (ipa_proj2.hip: K = c_s = 256)
static bool proj_image(const FdiptDims* d) { return half_mode(d) && d->c_s == 256; }
// merged IPA projections (ForwardPlan::merged; the o columns of linear_out keep their width: H c_s = H C): q', its bias and the
// merged linear_out
static bool merged_weights(const FdiptDims* d) { return d->c_s == d->c_hidden; }
// ... the merged projection as fragment images in fd_ipa_proj2's column order
static bool merged_image(const FdiptDims* d) {
  return proj_image(d) && merged_weights(d) && d->c_hidden % 128 == 0 && (d->no_heads * d->c_hidden) % 128 == 0;
}
// ... with the point columns regrouped for the projection's point epilogue (ipa_proj2.hip: fd_ipa_proj2_points_image)
static bool points_image(const FdiptDims* d) {
  return merged_image(d) && d->no_heads == 8 && d->c_hidden == 256 && d->no_qk_points == 8 && d->no_v_points == 12;
}
// ... the merged linear_out as hi / lo fragment images (gemm.hip: outproj_split_kernel)
static bool outproj_image(const FdiptDims* d, const Inventory& iv) { return merged_weights(d) && fd_outproj_split_supported(d->c_s, iv.feat_dim); }
// linear_b in the fragment order of the epilogues that emit the next block's pair bias (edge_transition3/4, edge_embed2)
static bool bias_images(const FdiptDims* d) { return d->c_z == 128 && d->no_heads <= 8; }
// down_z as fragment images (MFMA o_pair kernel; the epilogues that emit pair_z)
static bool dz_images(const FdiptDims* d) { return d->c_z == 128; }

// ------------------------------------------------------------------ prepare kernels
// dst[r, c] (ld_dst, operand precision) = scale * src[r, col0 + c] for c < ncols else 0
template <class T>
__global__ void copy_cols_kernel(int rows, int ncols, int ld_dst, const float* __restrict__ src, int ld_src, int col0,
                                 float scale, T* __restrict__ dst) {
  const long n = (long)rows * ld_dst;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int r = (int)(i / ld_dst), c = (int)(i % ld_dst);
    const float v = c < ncols ? scale * src[(long)r * ld_src + col0 + c] : 0.f;
    if constexpr (sizeof(T) == 4) dst[i] = v; else dst[i] = f2h(v);
  }
}
static int copy_cols(int esz, int rows, int ncols, int ld_dst, const float* src, int ld_src, int col0, float scale,
                     void* dst, hipStream_t st) {
  const long n = (long)rows * ld_dst;
  const unsigned g = (unsigned)((n + 255) / 256 > 1024 ? 1024 : (n + 255) / 256);
  if (esz == 4)
    hipLaunchKernelGGL(copy_cols_kernel<float>, dim3(g), dim3(256), 0, st, rows, ncols, ld_dst, src, ld_src, col0, scale,
                       (float*)dst);
  else
    hipLaunchKernelGGL(copy_cols_kernel<half_t>, dim3(g), dim3(256), 0, st, rows, ncols, ld_dst, src, ld_src, col0, scale,
                       (half_t*)dst);
  FD_CHECK_LAUNCH();
  return FDIPT_OK;
}
// dtab[k][c] = W1[c][col0 + k] (k < nb), dtab[nb][c] = 0 ; edges[k] = linspace(min,max,nb)[k] ; gamma
__global__ void misc_prepare_kernel(int cz, int nb, int ld_w, int col0, const float* __restrict__ w1, float min_bin,
                                    float max_bin, float* __restrict__ dtab, float* __restrict__ edges) {
  const int n = (nb + 1) * cz;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int k = i / cz, c = i % cz;
    dtab[i] = k < nb ? w1[(long)c * ld_w + col0 + k] : 0.f;
  }
  if (blockIdx.x == 0 && threadIdx.x < nb) {
    const double step = ((double)max_bin - (double)min_bin) / (double)(nb - 1);
    edges[threadIdx.x] = threadIdx.x == nb - 1 ? max_bin : (float)((double)min_bin + step * threadIdx.x);
  }
}
// dst[c][r] = src[r][c]  (down_z weight transposed for coalesced reads in opair_kernel)
__global__ void transpose_kernel(int rows, int cols, const float* __restrict__ src, float* __restrict__ dst) {
  const int n = rows * cols;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dst[(i % cols) * rows + i / cols] = src[i];
}
__global__ void gamma_kernel(int H, int Pq, const float* __restrict__ head_w, float* __restrict__ gamma) {
  const int h = threadIdx.x;
  if (h < H) {
    // softplus(w) * sqrt(1/(3*(Pq*9/2)))  (ipa_pytorch.py:265-271)
    const float sp = log1pf(expf(head_w[h]));
    gamma[h] = sp * sqrtf(1.0f / (3.0f * ((float)Pq * 9.0f / 2.0f)));
  }
}

// ------------------------------------------------------------------ merged IPA projections (prepare time, float64 accumulation)
// q . k over the keys j of a softmax row: (W_q s_i + b_q) . (W_k s_j + b_k) = s_j . W_k^T (W_q s_i + b_q) + (a constant in j, which the
// softmax drops) -> the keys are the node rows themselves and the query becomes q' = A s_i + c with A = W_k^T W_q, c = W_k^T b_q per head.
// Aq [H cs, cs], cq [H cs];  qw [H C, cs], qb [H C];  kvw [H 2C, cs] (per head: C rows of k, then C rows of v)
__global__ void merge_qk_kernel(int H, int C, int cs, const float* __restrict__ qw, const float* __restrict__ qb,
                                const float* __restrict__ kvw, float* __restrict__ Aq, float* __restrict__ cq) {
  const long n = (long)H * cs * (cs + 1);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int col = (int)(i % (cs + 1));
    const long hc = i / (cs + 1);
    const int c = (int)(hc % cs), h = (int)(hc / cs);
    double acc = 0;
    for (int dd = 0; dd < C; ++dd)
      acc += (double)kvw[((long)h * 2 * C + dd) * cs + c] * (double)(col < cs ? qw[((long)h * C + dd) * cs + col] : qb[h * C + dd]);
    if (col < cs) Aq[hc * cs + col] = (float)acc; else cq[hc] = (float)acc;
  }
}
// sum_j p_j v_j = W_v (sum_j p_j s_j) + b_v (sum_j p_j = 1): the values are the node rows, W_v moves into the output projection:
// Wm[o][h cs + c] = sum_d Wout[o][h C + d] W_v^h[d][c] for the o columns, the other columns are copied; bm = b_out + Wout[:, o cols] b_v
__global__ void merge_vo_kernel(int H, int C, int cs, int feat, const float* __restrict__ ow, const float* __restrict__ ob,
                                const float* __restrict__ kvw, const float* __restrict__ kvb, float* __restrict__ Wm,
                                float* __restrict__ bm) {
  const long n = (long)cs * (feat + 1);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int col = (int)(i % (feat + 1)), o = (int)(i / (feat + 1));
    if (col == feat) {
      double acc = ob[o];
      for (int k = 0; k < H * C; ++k) acc += (double)ow[(long)o * feat + k] * (double)kvb[(k / C) * 2 * C + C + k % C];
      bm[o] = (float)acc;
    } else if (col < H * cs) {
      const int h = col / cs, c = col % cs;
      double acc = 0;
      for (int dd = 0; dd < C; ++dd) acc += (double)ow[(long)o * feat + h * C + dd] * (double)kvw[((long)h * 2 * C + C + dd) * cs + c];
      Wm[(long)o * feat + col] = (float)acc;
    } else Wm[(long)o * feat + col] = ow[(long)o * feat + col];
  }
}

#define RC(x)                   \
  do {                          \
    int rc__ = (x);             \
    if (rc__) return rc__;      \
  } while (0)

// ------------------------------------------------------------------ the derived blob, declared once
// One walk over the blob declares every image once: the condition under which it exists, its size and its build step.  Without a
// blob (fdipt_derived_bytes, fdipt_sample_setup, the forward) it only sizes the layout; fdipt_model_prepare runs the same walk and
// launches each build step on the stream as its image is declared, so an image may be built from images declared before it.
struct Blob {
  const float* P;
  char* D;  // nullptr: size only, nothing is launched
  hipStream_t st;
  size_t o = 0;
  int rc = FDIPT_OK;  // the first failed build step (the later ones are skipped)
  template <class F> void step(bool on, F&& build) {
    if (on && D && rc == FDIPT_OK) rc = build();
  }
  // an image of `bytes` that exists when `on`; returns its offset
  template <class F> size_t img(bool on, size_t bytes, F&& build) {
    const size_t at = o;
    if (on) o = al256(o + bytes);
    step(on, [&] { return build(D + at); });
    return at;
  }
  size_t img(bool on, size_t bytes) { return img(on, bytes, [](char*) { return FDIPT_OK; }); }  // (written by a later build step)
  // a run: the images that `members` declares, back to back; returns its length
  template <class F> unsigned run(F&& members) {
    const size_t at = o;
    members();
    return (unsigned)(o - at);
  }
};

static int blob_walk(const FdiptDims* d, const Inventory& iv, DLayout& L, const float* P = nullptr, char* D = nullptr, hipStream_t st = nullptr) {
  Blob w{P, D, st};
  L = DLayout{};
  L.esz = half_mode(d) ? 2 : 4;
  L.kn_pad = rup8(iv.node_in);
  L.d1_pad = rup8(iv.d1);
  const int esz = L.esz, cs = d->c_s, cz = d->c_z, E = d->index_embed, H = d->no_heads, C = d->c_hidden, cb = iv.cb, hid = iv.hid;
  const int nsk = d->num_blocks * d->c_skip;
  const float s3 = sqrtf(1.0f / 3.0f);
  auto vec = [&](long src, int n, char* at) { return copy_cols(4, 1, n, n, P + src, n, 0, 1.f, at, st); };  // fp32 vector of P
  // fragment images of a whole matrix: 32-row (hi or lo) and 16-row (hi or lo)
  auto chain = [&](const LinW& l, int lo) {
    return w.img(true, fd_chain_image_bytes(l.out, l.in), [&](char* at) { return fd_chain_build_image(P + l.w, l.out, l.in, l.in, 0, lo, at, st); });
  };
  auto chain16 = [&](const LinW& l, int lo) {
    return w.img(true, fd_chain_image_bytes(l.out, l.in), [&](char* at) { return fd_chain_build_image16(P + l.w, l.out, l.in, l.in, l.in, lo, at, st); });
  };
  L.h16_base = w.img(half_mode(d), (size_t)iv.offsets.back() * 2,
                     [&](char* at) { return fd_f32_to_half(iv.offsets.back(), P, (half_t*)at, st); });
  // the node embedder's first layer [c_s, kn_pad] in operand precision; fp32 pieces of the concat-free first edge-embedder layer: the e_i,
  // e_j and relative-position columns, the distogram table [num_bins + 1, c_z] with the bin edges (one launch writes both; neither exists
  // for a model without the distogram, num_bins = 0), the bias
  L.ne0_pad = w.img(true, (size_t)cs * L.kn_pad * esz,
                    [&](char* at) { return copy_cols(esz, cs, iv.node_in, L.kn_pad, P + iv.ne0.w, iv.node_in, 0, 1.f, at, st); });
  L.w1i = w.img(true, (size_t)cz * L.d1_pad * 4, [&](char* at) { return copy_cols(4, cz, iv.d1, L.d1_pad, P + iv.ee0.w, iv.edge_in, 0, 1.f, at, st); });
  L.w1j = w.img(true, (size_t)cz * L.d1_pad * 4, [&](char* at) { return copy_cols(4, cz, iv.d1, L.d1_pad, P + iv.ee0.w, iv.edge_in, iv.d1, 1.f, at, st); });
  L.w1r = w.img(true, (size_t)cz * E * 4, [&](char* at) { return copy_cols(4, cz, E, E, P + iv.ee0.w, iv.edge_in, 2 * iv.d1, 1.f, at, st); });
  L.dtab = w.img(d->num_bins > 0, (size_t)(d->num_bins + 1) * cz * 4);
  L.edges = w.img(d->num_bins > 0, (size_t)d->num_bins * 4, [&](char* at) {
    hipLaunchKernelGGL(misc_prepare_kernel, dim3(16), dim3(256), 0, st, cz, d->num_bins, iv.edge_in, 2 * iv.d1 + E, P + iv.ee0.w, d->min_bin,
                       d->max_bin, (float*)(D + L.dtab), (float*)at);
    FD_CHECK_LAUNCH();
    return FDIPT_OK;
  });
  L.b1 = w.img(true, (size_t)cz * 4, [&](char* at) { return vec(iv.ee0.b, cz, at); });
  L.ee2 = w.img(use_regpair(d) && !ee2x_images(d), fd_ee2_image_bytes(), [&](char* at) { return fd_ee2_build_images(P + iv.ee2.w, P + iv.ee4.w, at, st); });
  L.ee2x = w.img(ee2x_images(d), fd_ee2_image_bytes(1), [&](char* at) { return fd_ee2_build_images(P + iv.ee2.w, P + iv.ee4.w, at, st, 1); });
  for (int b = 0; b < d->num_blocks; ++b) {
    const BlockW& k = iv.blk[b];
    DBlock& db = L.blk[b];
    const bool trunk = b < d->num_blocks - 1;  // an EdgeTransition follows
    // fused projection [q | kv | q_pts | kv_pts] rows (ipa_pytorch.py:202-239), its bias, and the same matrix as hi / lo fragment
    // images (tile-major images: stacking row blocks of 32 = concatenation), permuted where fd_ipa_proj2 takes the shapes
    const LinW* parts[4] = {&k.q, &k.kv, &k.qp, &k.kvp};
    const int row0[4] = {0, k.q.out, k.q.out + k.kv.out, k.q.out + k.kv.out + k.qp.out};
    db.wproj = w.img(true, (size_t)iv.proj_out * cs * esz, [&](char* at) {
      for (int p = 0; p < 4; ++p) RC(copy_cols(esz, parts[p]->out, cs, cs, P + parts[p]->w, cs, 0, 1.f, at + (size_t)row0[p] * cs * esz, st));
      return FDIPT_OK;
    });
    const size_t pib = (size_t)((iv.proj_out + 127) / 128) * 65536, tile = (size_t)(cs / 16) * 1024;
    auto proj_img = [&](int lo) {
      return w.img(proj_image(d), pib, [&](char* at) {
        if (hipMemsetAsync(at, 0, pib, st) != hipSuccess) return FDIPT_ELAUNCH;
        for (int p = 0; p < 4; ++p) {
          if (parts[p]->out % 32) return FDIPT_ESIZE;
          RC(fd_chain_build_image(P + parts[p]->w, parts[p]->out, cs, cs, 0, lo, at + (size_t)(row0[p] / 32) * tile, st));
        }
        return C % 128 == 0 && (H * C) % 128 == 0 ? fd_ipa_proj2_permute_image(at, H, C, cs, st) : FDIPT_OK;  // (what fd_ipa_proj2 reads)
      });
    };
    db.wproj_img = proj_img(0);
    db.wproj_img_lo = proj_img(1);
    db.bproj = w.img(true, (size_t)iv.proj_out * 4, [&](char* at) {
      for (int p = 0; p < 4; ++p) RC(vec(parts[p]->b, parts[p]->out, at + (size_t)row0[p] * 4));
      return FDIPT_OK;
    });
    // merged IPA projections (ForwardPlan::merged): q' = W_k^T (W_q s + b_q) per head as [H C, c_s] fp32 — prepare-time scratch, the
    // source of the merged projection image; merge_qk writes it with the q' part of the bias [q' | q_pts | kv_pts]
    const int HC = H * C, n2 = iv.proj_out - 2 * HC;
    db.wq_m = w.img(merged_weights(d), (size_t)HC * cs * 4);
    db.bproj2 = w.img(merged_weights(d), (size_t)n2 * 4, [&](char* at) {
      hipLaunchKernelGGL(merge_qk_kernel, dim3(512), dim3(256), 0, st, H, C, cs, P + k.q.w, P + k.q.b, P + k.kv.w, (float*)(D + db.wq_m), (float*)at);
      FD_CHECK_LAUNCH();
      RC(vec(k.qp.b, k.qp.out, at + (size_t)HC * 4));
      return vec(k.kvp.b, k.kvp.out, at + (size_t)(HC + k.qp.out) * 4);
    });
    // ... the fragment images of [q' | q_pts | kv_pts] (hi, lo; the parts' rows are whole tiles: the projection images above
    // refuse the shapes otherwise)
    const size_t mib = (size_t)((n2 + 127) / 128) * 65536;
    auto merged_img = [&](int lo) {
      return w.img(merged_image(d), mib, [&](char* at) {
        if (hipMemsetAsync(at, 0, mib, st) != hipSuccess) return FDIPT_ELAUNCH;
        const float* srcs[3] = {(const float*)(D + db.wq_m), P + k.qp.w, P + k.kvp.w};
        const int rows[3] = {HC, k.qp.out, k.kvp.out};
        for (int p = 0, r0 = 0; p < 3; r0 += rows[p++]) RC(fd_chain_build_image(srcs[p], rows[p], cs, cs, 0, lo, at + (size_t)(r0 / 32) * tile, st));
        return fd_ipa_proj2_permute_image_q(at, H, C, cs, st);
      });
    };
    db.wproj2_img = merged_img(0);
    db.wproj2_img_lo = merged_img(1);
    // ... the same with the point columns regrouped for the projection's point epilogue (the bias is written with each image)
    const size_t pcols = (size_t)fd_ipa_proj2_points_cols(H, C);
    db.bproj2p = w.img(points_image(d), pcols * 4);
    db.wproj2p_img = w.img(points_image(d), pcols / 128 * 65536, [&](char* at) {
      return fd_ipa_proj2_points_image(D + db.wproj2_img, (const float*)(D + db.bproj2), at, (float*)(D + db.bproj2p), H, C, cs, st);
    });
    db.wproj2p_img_lo = w.img(points_image(d), pcols / 128 * 65536, [&](char* at) {
      return fd_ipa_proj2_points_image(D + db.wproj2_img_lo, (const float*)(D + db.bproj2), at, (float*)(D + db.bproj2p), H, C, cs, st);
    });
    // ... linear_out with W_v folded into its o columns (merge_vo writes it with its bias), and as hi / lo fragment images
    db.wout_m = w.img(merged_weights(d), (size_t)cs * iv.feat_dim * 4);
    db.bout_m = w.img(merged_weights(d), (size_t)cs * 4, [&](char* at) {
      hipLaunchKernelGGL(merge_vo_kernel, dim3(512), dim3(256), 0, st, H, C, cs, iv.feat_dim, P + k.out.w, P + k.out.b, P + k.kv.w, P + k.kv.b,
                         (float*)(D + db.wout_m), (float*)at);
      FD_CHECK_LAUNCH();
      return FDIPT_OK;
    });
    auto outproj_img = [&](int lo) {
      return w.img(outproj_image(d, iv), fd_chain_image_bytes(cs, iv.feat_dim), [&](char* at) {
        return fd_chain_build_image((const float*)(D + db.wout_m), cs, iv.feat_dim, iv.feat_dim, 0, lo, at, st);
      });
    };
    db.wout_img = outproj_img(0);
    db.wout_img_lo = outproj_img(1);
    db.gamma = w.img(true, (size_t)H * 4, [&](char* at) {
      hipLaunchKernelGGL(gamma_kernel, dim3(1), dim3(64), 0, st, H, d->no_qk_points, P + k.head_w, (float*)at);
      FD_CHECK_LAUNCH();
      return FDIPT_OK;
    });
    // pair bias pre-scaled by sqrt(1/3) (ipa_pytorch.py:256-257); linear_b as 16 x 128 (edge_transition3 epilogue) and compact (8 head
    // rows: 2 KB) in the hand-off order of edge_transition4 / edge_embed2
    db.wb = w.img(true, (size_t)H * cz * esz, [&](char* at) { return copy_cols(esz, H, cz, cz, P + k.lb.w, cz, 0, s3, at, st); });
    db.bb = w.img(true, (size_t)H * 4, [&](char* at) { return copy_cols(4, 1, H, H, P + k.lb.b, H, 0, s3, at, st); });
    db.wb_img3 = w.img(bias_images(d), 4096, [&](char* at) { return fd_et3_build_bias_image(P + k.lb.w, H, s3, at, st); });
    db.wb_img4 = w.img(bias_images(d), 8192, [&](char* at) { return fd_et4_build_bias_image(P + k.lb.w, H, s3, at, st); });
    // down_z [c_z/4, c_z] as fragment images (MFMA o_pair kernel), of Wdz and of Wdz - half(Wdz), then both with k in the hand-off order
    // of the LayerNorm epilogues that emit pair_z; the emitting EdgeTransition (the previous block's) finds them in the last chunk of its
    // weight stream
    auto dz_img = [&](int permuted, int lo) {
      return w.img(dz_images(d), fd_chain_image_bytes(cz / 4, cz), [&](char* at) { return fd_chain_build_image(P + k.dz.w, cz / 4, cz, cz, permuted, lo, at, st); });
    };
    db.wdz_img = dz_img(0, 0);
    db.wdz_img_lo = dz_img(0, 1);
    db.wdz_imgp = dz_img(1, 0);
    db.wdz_imgp_lo = dz_img(1, 1);
    w.step(b > 0 && use_regpair(d) && !et4x_stream(d), [&] { return fd_et4_set_dz(D + L.blk[b - 1].et4, D + db.wdz_imgp, D + db.wdz_imgp_lo, st); });
    w.step(b > 0 && et4x_stream(d), [&] { return fd_et4_set_dz(D + L.blk[b - 1].et4x, D + db.wdz_imgp, D + db.wdz_imgp_lo, st, 1); });
    db.wdz_t = w.img(true, (size_t)cz * (cz / 4) * 4, [&](char* at) {  // (transposed for coalesced reads in opair_kernel)
      hipLaunchKernelGGL(transpose_kernel, dim3(16), dim3(256), 0, st, cz / 4, cz, P + k.dz.w, (float*)at);
      FD_CHECK_LAUNCH();
      return FDIPT_OK;
    });
    db.et3 = w.img(use_regpair(d) && !et4x_stream(d) && trunk, fd_et3_stream_bytes(), [&](char* at) { return fd_et3_build_stream(P + k.et1.w, P + k.et2.w, P + k.etf.w, at, st); });
    db.et4 = w.img(use_regpair(d) && !et4x_stream(d) && trunk, fd_et4_stream_bytes(), [&](char* at) { return fd_et4_build_stream(P + k.et1.w, P + k.et2.w, P + k.etf.w, at, st); });
    db.et4x = w.img(et4x_stream(d) && trunk, fd_et4_stream_bytes(1), [&](char* at) { return fd_et4_build_stream(P + k.et1.w, P + k.et2.w, P + k.etf.w, at, st, 1); });
    if (!use_chain(d)) continue;
    // ---- the fused node path: 32-row images (hi), lo images of the split operands, 16-row images (hi, lo)
    // [W1[:, e_i]; Wf[:, e_i]; W1[:, e_j]; Wf[:, e_j]] of EdgeTransition's first / final layers, the first `parts` of them stacked
    // (tile-major images: stacking = concatenation)
    auto et_rows = [&](int parts, int rows16, int lo) {
      return w.img(trunk, fd_chain_image_bytes(parts / 2 * (hid + cz), cb), [&](char* at) {
        const float* src[4] = {P + k.et1.w + cz, P + k.etf.w + cz, P + k.et1.w + cz + cb, P + k.etf.w + cz + cb};
        for (int p = 0; p < parts; at += fd_chain_image_bytes(p % 2 ? cz : hid, cb), ++p)
          RC(rows16 ? fd_chain_build_image16(src[p], p % 2 ? cz : hid, cb, cb, hid, lo, at, st)
                    : fd_chain_build_image(src[p], p % 2 ? cz : hid, cb, hid, 0, lo, at, st));
        return FDIPT_OK;
      });
    };
    DChain& c = db.ch;
    for (int l = 0; l < d->tfmr_layers; ++l) {
      c.inp[l] = chain(k.tf[l].inp, 0); c.outp[l] = chain(k.tf[l].outp, 0); c.l1[l] = chain(k.tf[l].l1, 0); c.l2[l] = chain(k.tf[l].l2, 0);
    }
    c.post = chain(k.post, 0);
    c.t1 = chain(k.t1, 0);
    c.t23_run = w.run([&] { c.t2 = chain(k.t2, 0); c.t3 = chain(k.t3, 0); });
    if (trunk) {
      c.et_init = chain(k.et_init, 0);
      c.a1af = et_rows(2, 0, 0);  // [A1 | Af] rows (rowblock.hip) and their biases [b1; bf]
      c.b1f = w.img(true, (size_t)(hid + cz) * 4, [&](char* at) {
        RC(vec(k.et1.b, hid, at));
        return vec(k.etf.b, cz, at + (size_t)hid * 4);
      });
      c.r4w = et_rows(4, 0, 0);  // edge_transition4 rows, one 1024-row image, and their biases [b1; bf; 0; 0]
      c.r4b = w.img(true, (size_t)2 * (hid + cz) * 4, [&](char* at) {
        RC(vec(k.et1.b, hid, at));
        RC(vec(k.etf.b, cz, at + (size_t)hid * 4));
        return hipMemsetAsync(at + (size_t)(hid + cz) * 4, 0, (size_t)(hid + cz) * 4, st) == hipSuccess ? FDIPT_OK : FDIPT_ELAUNCH;
      });
    }
    DSplit& s = db.lo;
    for (int l = 0; l < d->tfmr_layers; ++l) {
      s.inp[l] = chain(k.tf[l].inp, 1); s.outp[l] = chain(k.tf[l].outp, 1); s.l1[l] = chain(k.tf[l].l1, 1); s.l2[l] = chain(k.tf[l].l2, 1);
    }
    s.post = chain(k.post, 1);
    s.t_run = w.run([&] { s.t1 = chain(k.t1, 1); s.t2 = chain(k.t2, 1); s.t3 = chain(k.t3, 1); });
    if (trunk) s.et_run = w.run([&] { s.et_init = chain(k.et_init, 1); s.r4w = et_rows(4, 0, 1); });
    for (int h = 0; h < 2; ++h) {
      for (int l = 0; l < d->tfmr_layers; ++l)
        s.tail16_run[l] = w.run([&] {
          s.o16[l][h] = chain16(k.tf[l].outp, h); s.f16[l][h] = chain16(k.tf[l].l1, h); s.g16[l][h] = chain16(k.tf[l].l2, h);
          if (l + 1 == d->tfmr_layers) s.p16[h] = chain16(k.post, h);
        });
      s.tr16_run = w.run([&] { s.tr16[0][h] = chain16(k.t1, h); s.tr16[1][h] = chain16(k.t2, h); s.tr16[2][h] = chain16(k.t3, h); });
      // (mlp16_kernel<.., ETR>: the transition launch that folds EdgeTransition's row launch in)
      if (trunk) s.et16_run = w.run([&] { s.ei16[h] = chain16(k.et_init, h); s.r416[h] = et_rows(4, 1, h); });
    }
  }
  if (use_chain(d)) {  // node embedder and torsion head (iv.node_in <= 96: index_embed 32)
    auto ne0 = [&](int lo) {
      return w.img(true, fd_chain_image_bytes(cs, L.kn_pad), [&](char* at) { return fd_chain_build_image(P + iv.ne0.w, cs, iv.node_in, iv.node_in, 0, lo, at, st); });
    };
    L.lo_ne0 = ne0(1); L.lo_ne2 = chain(iv.ne2, 1); L.lo_ne4 = chain(iv.ne4, 1);
    L.lo_tor_run = w.run([&] { L.lo_tor1 = chain(iv.tor1, 1); L.lo_tor2 = chain(iv.tor2, 1); });
    for (int h = 0; h < 2; ++h)
      L.ne16_run = w.run([&] {
        L.ne16[0][h] = w.img(true, fd_chain_image_bytes(cs, 96), [&](char* at) { return fd_chain_build_image16(P + iv.ne0.w, cs, iv.node_in, 96, iv.node_in, h, at, st); });
        L.ne16[1][h] = chain16(iv.ne2, h); L.ne16[2][h] = chain16(iv.ne4, h);
      });
    for (int h = 0; h < 2; ++h) L.tor16_run = w.run([&] { L.tor16[0][h] = chain16(iv.tor1, h); L.tor16[1][h] = chain16(iv.tor2, h); });
    L.ch_ne0 = ne0(0); L.ch_ne2 = chain(iv.ne2, 0); L.ch_ne4 = chain(iv.ne4, 0); L.ch_tor1 = chain(iv.tor1, 0); L.ch_tor2 = chain(iv.tor2, 0);
  }
  // skip_embed of all blocks stacked: its bias, the matrix in fp32, and as 16-row images (from the fp32 one)
  auto skip = [&](int bias) {
    return w.img(true, (size_t)nsk * (bias ? 1 : cs) * 4, [&](char* at) {
      for (int b = 0; b < d->num_blocks; ++b) {
        const LinW& l = iv.blk[b].skip;
        RC(bias ? vec(l.b, l.out, at + (size_t)b * l.out * 4) : copy_cols(4, l.out, cs, cs, P + l.w, cs, 0, 1.f, at + (size_t)b * l.out * cs * 4, st));
      }
      return FDIPT_OK;
    });
  };
  L.skip_b = skip(1);
  L.skip_w32 = skip(0);
  L.skip16_run = w.run([&] {
    for (int h = 0; h < 2; ++h)
      L.skip16[h] = w.img(skip16_image(d), fd_chain_image_bytes(nsk, cs),
                          [&](char* at) { return fd_chain_build_image16((const float*)(D + L.skip_w32), nsk, cs, cs, cs, h, at, st); });
  });
  L.total = w.o;
  return w.rc;
}

extern "C" {

int fdipt_param_count(const FdiptDims* dims) {
  if (!dims_ok(dims)) return FDIPT_EINVAL;
  Inventory iv;
  build_inventory(dims, iv);
  return (int)iv.offsets.size() - 1;
}

int64_t fdipt_param_offset(const FdiptDims* dims, int index) {
  if (!dims_ok(dims)) return FDIPT_EINVAL;
  Inventory iv;
  build_inventory(dims, iv);
  if (index < 0 || index >= (int)iv.offsets.size()) return FDIPT_EINVAL;
  return iv.offsets[index];
}

size_t fdipt_derived_bytes(const FdiptDims* dims) {
  if (!dims_ok(dims)) return 0;
  Inventory iv;
  DLayout L;
  build_inventory(dims, iv);
  blob_walk(dims, iv, L);
  return L.total;
}

int fdipt_model_prepare(const FdiptDims* d, const float* P, void* derived, fdipt_stream_t stream) {
  if (!dims_ok(d) || !P || !derived) return FDIPT_EINVAL;
  Inventory iv;
  DLayout L;
  build_inventory(d, iv);
  return blob_walk(d, iv, L, P, (char*)derived, (hipStream_t)stream);
}

// `setup`: the R rows [B, n_rel, c_z] f32, then int32 [B]: the first sample whose R rows carry the bits of sample b's (the row table's
// leader rule reads it every step instead of comparing the rows again: edge_embed2.hip)
static size_t setup_rel_lead(const FdiptDims* dims, int B, int n_rel) { return al256((size_t)B * n_rel * dims->c_z * 4); }
size_t fdipt_setup_bytes(const FdiptDims* dims, int B, int N, int n_rel) {
  if (!dims_ok(dims) || B <= 0 || N <= 0 || n_rel <= 0) return 0;
  return setup_rel_lead(dims, B, n_rel) + al256((size_t)B * 4);
}

int fdipt_sample_setup(const FdiptDims* d, const float* P, const void* derived, int B, int N, int n_rel,
                       const float* rel_emb, void* setup, fdipt_stream_t stream) {
  if (!dims_ok(d) || !P || !derived || !rel_emb || !setup || B <= 0 || N <= 0 || n_rel <= 0) return FDIPT_EINVAL;
  Inventory iv;
  DLayout L;
  build_inventory(d, iv);
  blob_walk(d, iv, L);
  // R[b, r, :] = W1[:, 2*d1 : 2*d1+E] index_embedding(r - rel_off)   (fp32; constant along the trajectory)
  RC(fd_linear(FDIPT_PREC_F32, B * n_rel, d->c_z, d->index_embed, rel_emb, d->index_embed,
               (const char*)derived + L.w1r, d->index_embed, nullptr, nullptr, 0, nullptr, 0, (float*)setup, d->c_z,
               (hipStream_t)stream));
  return fd_ee2_rel_leaders(B, (long)n_rel * d->c_z, (const float*)setup, (int32_t*)((char*)setup + setup_rel_lead(d, B, n_rel)), (hipStream_t)stream);
}

// ------------------------------------------------------------------ workspace
struct WS {
  size_t node_feat, pte, pi, pj, h_a, h_b, node0, node, z, quat, trans, dmask, rot, proj, qp, kp, vp, bias, probs, feats,
      ipa_out, tf_in, qkv, att, x_a, x_b, ff, e, upd, psi_un, a1, af, qb, kb, vt, pts, seqimg, ipa_parts, e_bf, vpt, r4, a1img, b1img, skip_all, vt_lo, kpf, pz, ee_tab, ee_idx, ee_lead, total;
};
static void build_ws(const FdiptDims* d, const Inventory& iv, const DLayout& L, int B, int N, WS& w) {
  size_t o = 0;
  const size_t R = (size_t)B * N, NN = R * N;
  auto take = [&](size_t bytes) { size_t r = o; o = al256(o + bytes); return r; };
  const int H = d->no_heads;
  w.node_feat = take(R * L.kn_pad * 4); w.pte = take(R * L.d1_pad * 4);
  w.pi = take(R * d->c_z * 4); w.pj = take(R * d->c_z * 4);
  w.h_a = take(R * d->c_s * 4); w.h_b = take(R * d->c_s * 4); w.node0 = take(R * d->c_s * 4); w.node = take(R * d->c_s * 4);
  w.z = take(NN * d->c_z * L.esz);
  w.quat = take(R * 4 * 4); w.trans = take(R * 3 * 4); w.dmask = take(R * 4); w.rot = take(R * 9 * 4);
  w.proj = take(R * iv.proj_out * 4);
  w.qp = take(R * H * d->no_qk_points * 3 * 4); w.kp = take(R * H * d->no_qk_points * 3 * 4);
  w.vp = take(R * H * d->no_v_points * 3 * 4);
  {
    const size_t Npb = ((size_t)N + 31) / 32 * 32;
    w.bias = take((size_t)B * H * Npb * Npb * 4);  // fragment order for attention3 (>= the plain [B,H,N,N] / [B,N,N,H] forms)
  }
  w.probs = take(NN * H * 4);
  w.feats = take(R * iv.feat_dim * 4);
  w.ipa_out = take(R * d->c_s * 4);
  w.tf_in = take(R * iv.d_t * 4); w.qkv = take(R * 3 * iv.d_t * 4); w.att = take(R * iv.d_t * 4);
  w.x_a = take(R * iv.d_t * 4); w.x_b = take(R * iv.d_t * 4); w.ff = take(R * iv.d_t * 4);
  w.e = take(R * iv.cb * 4); w.upd = take(R * 8 * 4); w.psi_un = take(R * 8 * 4);
  w.a1 = take(R * iv.hid * 4); w.af = take(R * d->c_z * 4);
  {
    const size_t Np = ((size_t)N + 31) / 32 * 32, HC = (size_t)H * d->c_hidden;
    w.qb = take((size_t)B * HC * Np * 2); w.kb = take((size_t)B * HC * Np * 2); w.vt = take((size_t)B * HC * Np * 2);  // fragment-order images
    w.vt_lo = take((size_t)B * HC * Np * 2);  // V - half(V) (split P V)
    w.pts = take(R * (size_t)(iv.proj_out - 3 * HC) * 4);
  }
  w.seqimg = take(fd_seq_attention_image_bytes(B, N, d->tfmr_heads));
  w.ipa_parts = take((size_t)8 * R * d->c_s * 4);
  w.vpt = take((size_t)B * H * 96 * (((size_t)N + 31) / 32 * 32) * 2);  // v_pts hi/lo fragment image (attention3 o_pt)
  w.e_bf = take(R * iv.cb * 2);  // bf16 copy of initial_embed(node) (edge_transition3 fetches it by LDS-DMA)  // split-K partial products of the IPA output projection
  w.skip_all = take(R * (size_t)d->num_blocks * d->c_skip * 4);  // skip_embed(init_node) of all blocks
  w.r4 = take(R * (size_t)1024 * 4);  // edge_transition4: [A1 | Af | B1 | Bf] rows, then their fold-fragment images
  w.a1img = take(fd_et4_a_image_bytes(B, N));
  w.b1img = take(fd_et4_b_image_bytes(B, N));
  w.kpf = take((size_t)B * H * ((((size_t)N + 31) / 32)) * FD_KPF_FRAGS * 1024);  // key-point fragment image (attention3 point logits)
  w.pz = take(use_regpair(d) ? fd_pz_bytes(B, N) : 0);  // pair_z image of the current block (round 6: written by the producer of z)
  w.ee_tab = take(ee_table_static(d, B, N) ? fd_ee2_table_bytes(B, ee_table_max_rel(N), d->num_bins) : 0);  // the edge embedder's row table
  w.ee_idx = take(ee_table_static(d, B, N) ? NN * 4 : 0);  // ... and the table row of every pair (block 0's EdgeTransition gathers its z rows)
  w.ee_lead = take((size_t)B * 4);  // ... and the leader of every sample (int32[B]: whose rows its pairs read; a few bytes, reserved whatever the shape)
  w.total = o;
}

size_t fdipt_forward_workspace_bytes(const FdiptDims* dims, int B, int N) {
  if (!dims_ok(dims) || B <= 0 || N <= 0) return 0;
  Inventory iv;
  DLayout L;
  WS w;
  build_inventory(dims, iv);
  blob_walk(dims, iv, L);
  build_ws(dims, iv, L, B, N, w);
  return w.total;
}

}  // extern "C"

// One sub-module of the forward on caller-provided inputs (the per-op entries of include/fdipt.h): the same launch schedule
// as the full forward, cut at the sub-module's boundary.
enum { OP_ALL, OP_EMBED, OP_POINTS, OP_IPA, OP_ET };
struct OpSel {
  int kind = OP_ALL, block = 0;
  const float* node_in = nullptr;   // [B,N,c_s]                      (POINTS, IPA, ET)
  const void* z_in = nullptr;       // [B,N,N,c_z] pair type           (IPA, ET)
  void* z_out = nullptr;            // [B,N,N,c_z] pair type           (EMBED, ET)
  float* node_out = nullptr;        // [B,N,c_s]                       (EMBED)
  float* out = nullptr;             // [B,N,c_s] linear_out(features)  (IPA)
  float *qp = nullptr, *kp = nullptr, *vp = nullptr;  // global-frame points (POINTS)
};

// ------------------------------------------------------------------ kernel selection of one forward
// The library reads no environment.  FdiptDims.kernel_flags (include/fdipt.h: FDIPT_KF_*) selects the fallback paths that other
// shapes use anyway, so that parity tests can run them at the golden sizes.  Every choice below is a function of the dims, the
// flags, the shape and the op kind only: the same for every block, made once per forward.
enum NodeForm { NF_GEMM, NF_ROWBLOCK, NF_ROWS16 };  // node-path MLPs: GEMM + LayerNorm launches, 32-row row-block kernel, 16-row kernel
enum SkipAt { SKIP_PER_BLOCK, SKIP_EMBED16, SKIP_SPLITK };  // skip_embed(init_node): per block, or once for all blocks
enum OutProj { OUT_GEMM, OUT_DEDICATED, OUT_SPLITK_SPLIT };  // IPA linear_out
enum NodeRows { NR_PROJ, NR_POINTS, NR_LAUNCH };  // merged projection: who writes the node-row images (Kb / Vt / Vt_lo)
enum SeqAttn { SEQ_FUSED, SEQ_BF16, SEQ_F32, SEQ_GENERIC };  // sequence-transformer attention: in_proj writes the images / bf16 / fp32 / LDS kernel
enum PostAt { POST_TAIL, POST_CHAIN, POST_GEMM };
enum EtKind { ET_GEMM, ET_CHAIN, ET_ET3, ET_ET4 };
enum EtRows { ETR_IMAGES, ETR_ROWS, ETR_FOLDED };  // edge_transition4's per-residue rows: row-block images, rows + image pass, transition launch
struct ForwardPlan {
  int op;
  bool bf, fused_node;  // half-precision mode; the fused node path (below)
  NodeForm embed, tail, transition, torsion;
  SkipAt skip;
  OutProj outproj;
  int slices;   // split-K slices of the output projection
  bool feats_fused, ee_bias, et_bias, pz;
  bool ee_table;                       // the edge embedder as row table + spread (ee_table_static and the call's n_rel; not with trace_edge)
  bool stream;                         // FDIPT_KF_STREAM_ATTN in the half-precision mode, N <= 2048: the key-streaming attention kernels
  bool a3, probs_h16;                  // IPA path: attention3, and the MFMA o_pair fed with bf16 attention weights
  bool vpt, proj2, merged, proj_pts, vt_lo, init_fused;
  NodeRows node_rows;
  SeqAttn seq;
  PostAt post;
  bool et_widths;                      // reference widths of the EdgeTransition rows (cb 128, hidden 384, c_z 128)
  EtKind et;
  EtRows et_rows;
  bool torf_fused, bb_fold;
  bool regpair;                        // register-resident pair kernels (edge_embed2, edge_transition3/4)
  bool ipa_bias_f32, ipa_attn_f32;     // fp32 mode: the one-pass pair bias, the register-score IPA attention (where it takes the call)
  bool x;                              // fp16x: edge_transition4 on the lo stream (et4x)
  bool refused;                        // fp16x: the plan would run a kernel without its split terms (the forward answers FDIPT_EINVAL)
};
static const char kImage = 0;  // stands for an operand image in the probe arguments below (the predicates test only that it is set)

static ForwardPlan plan_forward(const FdiptDims* d, const Inventory& iv, const DLayout& L, int B, int N, int op, int n_rel, bool trace_edge,
                                bool pair_embed) {
  const unsigned f = (unsigned)d->kernel_flags;
  const bool generic_attn = f & FDIPT_KF_GENERIC_ATTN, unfolded = f & FDIPT_KF_UNFOLDED;
  const int cs = d->c_s, cz = d->c_z, H = d->no_heads, C = d->c_hidden, Pq = d->no_qk_points, Pv = d->no_v_points;
  const int Np = (N + 31) / 32 * 32;
  ForwardPlan p = {};
  p.op = op;
  p.bf = half_mode(d);
  // The fused node path (use_chain: the reference widths of the half-precision mode; FDIPT_KF_UNFUSED_NODE clears it).  Row-complete
  // fused MLPs (rowblock.hip) take the multi-layer kinds and the 320-wide transformer layers; fused chains (chain.hip) take post_tfmr
  // and EdgeTransition.initial_embed where the row-block kernels do not (they beat the GEMM + LayerNorm launches they replace at
  // B*N ~ 2400 rows on MI355X, profiles/r01_chain_vs_gemm.md).  Its dense layers run on split operands (hi + lo half-precision parts,
  // 3 MFMAs per k-step): their operand rounding dominates the error of the predicted frames and psi (tests/err_budget.py) — node
  // embedder, IPA projection and output projection, attention P V, o_pair down-projection, sequence transformer (in_proj, out_proj,
  // feed-forward), post_tfmr, transition, EdgeTransition per-residue rows, skip_embed, torsion head
  p.fused_node = use_chain(d);
  // 16-row node-path blocks pay off while they are about one round of the chip (B N <= ~4000 rows: twice the blocks of the 32-row kernels, each
  // streaming all weights, half the matrix work per block); with every CU busy anyway the 32-row kernels move half the weight bytes (measured: c4
  // with 64 samples per GPU 1.277 -> 1.246 M).  The choice goes by N alone — a sample's result must not depend on the batch it rides in.
  // (the 16-row images exist with the 32-row ones: use_chain)
  const bool rows16 = p.fused_node && !(f & FDIPT_KF_ROWS32) && N <= 512;
  p.embed = p.fused_node && (L.kn_pad == 72 || L.kn_pad == 88) ? (rows16 ? NF_ROWS16 : NF_ROWBLOCK) : NF_GEMM;
  p.torsion = p.tail = p.transition = p.fused_node ? (rows16 ? NF_ROWS16 : NF_ROWBLOCK) : NF_GEMM;
  // the IPA output projection as split-K slices that its LayerNorm sums; skip_embed(init_node) of every block depends on the
  // embedder output only: one launch for all blocks, copied behind the LayerNorm output by that LayerNorm (FDIPT_KF_UNFOLDED: per block)
  const bool splitk = p.fused_node && iv.feat_dim >= 1024;
  if (!splitk || unfolded || op != OP_ALL) p.skip = SKIP_PER_BLOCK;
  else if (p.embed == NF_ROWS16 && skip16_image(d)) p.skip = SKIP_EMBED16;  // a fourth layer of the embedder launch
  else p.skip = SKIP_SPLITK;
  // the split of x_t (ipa_pytorch.py:516-524) and the per-residue halves of the first edge-embedder layer in the feature launch
  // (FDIPT_KF_UNFOLDED: three GEMM / element-wise launches more)
  p.feats_fused = L.d1_pad <= 128 && (L.d1_pad & 3) == 0 && !unfolded && op == OP_ALL;
  // The IPA path: attention3, and behind it the MFMA o_pair kernel fed with the attention weights as half-precision rows
  Attn3Args a3 = {};
  a3.B = B; a3.N = N; a3.H = H; a3.Np = Np; a3.vpt = (const half_t*)&kImage;
  OPairArgs oa = {};
  oa.B = B; oa.N = N; oa.H = H; oa.CZ = cz; oa.CD = cz / 4; oa.wdz_img = p.bf && dz_images(d) ? &kImage : nullptr;
  // key-streaming attention (attention3.hip / attention_seq.hip: two sweeps over key chunks) for every N <= 2048; it lifts the register
  // kernels' N <= 1024 wherever this plan tests a length (IPA attention, o_pair, pair bias producers, sequence attention)
  p.stream = (f & FDIPT_KF_STREAM_ATTN) && p.bf && !generic_attn && N <= 2048;
  const int n_attn = p.stream ? 2048 : 1024;  // the attention kernels' bound on N
  const bool opair_mfma = fd_opair_mfma_eligible(op_precision(d), oa, p.stream);
  p.a3 = p.bf && cz == 128 && C == 256 && Pq == 8 && Pv == 12 && !generic_attn &&
         (p.stream ? fd_attention3_stream_supported(a3) : fd_attention3_supported(a3));
  p.probs_h16 = p.a3 && opair_mfma && 2 * Np <= 4 * N;
  // the next block's pair bias linear_b(z)/sqrt(3) from the LayerNorm epilogue of the producer of z (saves a pass over z): the
  // embedder for block 0 (register kernel only), the EdgeTransition of block b for block b + 1
  const bool bias_rule = bias_images(d) && C == 256 && Pq == 8 && Pv == 12 && N <= n_attn && !generic_attn && !unfolded;
  p.regpair = use_regpair(d);
  p.ee_bias = bias_rule && p.regpair;
  p.et_bias = bias_rule;
  // EdgeTransition: register-resident pair kernels at the reference widths, edge_transition4 (8 x 4-pair patches, N % 4 == 0) or
  // edge_transition3 (16-pair waves: any N >= 43); anything else (N < 43 with N % 4 != 0, other widths) runs the LDS-chain kernel of
  // pair_mlp.hip.  edge_transition4's rows come from the transition launch where that is the 16-row kernel (FDIPT_KF_UNFOLDED: a row
  // launch and an image pass)
  p.et_widths = iv.cb == 128 && iv.hid == 384 && cz == 128;
  const bool reg_ok = p.fused_node && p.et_widths && p.regpair;
  if (reg_ok && !(f & FDIPT_KF_ET3) && fd_edge_transition4_supported(N)) p.et = ET_ET4;
  else if (reg_ok && fd_edge_transition3_supported(N)) p.et = ET_ET3;
  else p.et = p.fused_node ? ET_CHAIN : ET_GEMM;
  p.et_rows = unfolded ? ETR_ROWS : p.et == ET_ET4 && p.transition == NF_ROWS16 && op == OP_ALL ? ETR_FOLDED : ETR_IMAGES;
  // Round 6: o_pair reads pair_z = down_z(z) + b (32 channels) emitted by the producers of the pair bias above (edge_transition4 only)
  // instead of streaming the 128 channels of z once more per block (opair_pz_kernel).  FDIPT_KF_UNFOLDED / FDIPT_KF_PASS_Z keep the pass
  // over z.  The consumer: the IPA path that reads probs_h16.
  p.pz = op == OP_ALL && p.probs_h16 && p.et == ET_ET4 && bias_rule && !(f & FDIPT_KF_PASS_Z);
  // The embedder's distinct rows once, then spread (FdiptForwardArgs.pair_embed: every pair evaluated).  Whole forwards on the edge_embed2 /
  // edge_transition4 path with both emissions; a trace wants the fp32 rows of the pair kernel.  Decided from the shape and the call's
  // n_rel (set-up data): the launches of a step do not depend on the step's inputs
  {
    EdgeEmbedArgs ep = {};
    ep.B = B; ep.N = N; ep.n_rel = n_rel; ep.num_bins = d->num_bins; ep.H = H;
    p.ee_table = ee_table_static(d, B, N) && op == OP_ALL && p.ee_bias && p.pz && !trace_edge && !pair_embed && n_rel > 0 && n_rel <= ee_table_max_rel(N) &&
                 ee_table_rows_ok(B, N, n_rel, d->num_bins) && fd_edge_embed2_table_supported(ep);
  }
  // IPA projection (attention3 path): fused projection written directly as attention operand images (Qb, Kb, Vt) + raw point columns
  p.vpt = p.a3 && Pv == 12;
  ProjArgs pj = {};
  pj.B = B; pj.N = N; pj.H = H; pj.C = C; pj.K = cs; pj.PT = iv.proj_out - 3 * H * C; pj.Np = Np; pj.lda = cs;
  pj.W_img = proj_image(d) ? &kImage : nullptr;
  pj.W_img_lo = pj.W_img && p.fused_node ? &kImage : nullptr;
  // Merged projections (the default of the fused node path): no k, no v — the node rows are keys and values of
  // every head (fd_node_images), q' = W_k^T (W_q s + b_q), W_v sits in the output projection (prepare: merge_qk / merge_vo).  40 % of
  // the projection's columns, and K / V images an eighth of the size.  Exact algebra (softmax shift invariance, linearity); the
  // per-op entries and FDIPT_KF_NO_MERGE keep the reference's formulation.
  p.merged = p.a3 && pj.W_img_lo && merged_image(d) && !(f & FDIPT_KF_NO_MERGE) && op == OP_ALL && fd_ipa_proj2_supported(pj);
  pj.merged = p.merged;
  // point epilogue (ipa_proj2.hip: p2_points_walk / p2_node_rows): the merged projection also writes the rotated points (qp, kpf, vpt,
  // rot) and the node-row images; no point launch, no fp32 point columns.  This flag decides the projection's image, the pads and
  // the launches dropped
  p.proj_pts = p.merged && !(f & FDIPT_KF_POINTS_LAUNCH) && p.vpt && points_image(d) && fd_ipa_proj2_points_supported(pj, Pq, Pv);
  if (p.proj_pts) pj.PT = fd_ipa_proj2_points_cols(H, C) - H * C;
  // second generation (activation fragments in registers, weights by LDS-DMA) where it applies, else the tiled GEMM
  p.proj2 = p.a3 && fd_ipa_proj2_supported(pj);
  // P V on split operands needs V_lo, which only the split second-generation projection (or the node-row images) writes
  p.vt_lo = p.merged || (p.proj2 && pj.W_img_lo);
  // (the node-row images ride on the point launch when that is the 16-keys-per-block kernel; else their own launch)
  p.node_rows = !p.merged || p.proj_pts ? NR_PROJ : p.vpt && (H & 1) == 0 && cs == 256 ? NR_POINTS : NR_LAUNCH;
  const int th = d->tfmr_heads, hd = iv.d_t / th;
  const bool seq_ok = p.stream ? fd_seq_attention_stream_supported(N, th, hd) : fd_seq_attention_supported(N, th, hd);
  if (p.fused_node && !generic_attn && seq_ok && fd_seq_qkv_supported(N, th, iv.d_t)) p.seq = SEQ_FUSED;
  else if (p.bf && !generic_attn && seq_ok) p.seq = SEQ_BF16;
  else if (!p.bf && !generic_attn && fd_seq_attention_f32_supported(N, th, hd, 3 * iv.d_t)) p.seq = SEQ_F32;  // scores in registers (round 5)
  else p.seq = SEQ_GENERIC;
  p.ipa_bias_f32 = !p.bf && H == 8 && cz == 128;
  p.ipa_attn_f32 = !p.bf && !generic_attn;
  // every once-per-forward fill of the trunk in one launch: sequence-attention images, value-point image, key pads
  p.init_fused = p.proj2 && p.seq == SEQ_FUSED && !unfolded;  // (proj2: C % 128 == 0; the value-point image: whole 16 B units)
  // (the attention weights go to the MFMA o_pair kernel as bf16 rows [b, i, h, Np]: half the bytes, no conversion pass; the fp32
  // buffer is reused: B N H Np bf16 <= B H N N fp32)
  // K = 2688 in 3 slices (70 KB of LDS per block = two blocks per CU: at B N = 2400 rows 456 blocks run in one round of the 256 CUs,
  // 30 us; 4 slices = 608 blocks need two rounds, 41 us).  The slice count must not depend on the batch size: the order of the
  // partial sums is part of a sample's result (sub-batches and sharded runs reproduce the whole-batch result bit for bit)
  if (!splitk) p.outproj = OUT_GEMM;
  else p.outproj = p.merged && outproj_image(d, iv) ? OUT_DEDICATED : OUT_SPLITK_SPLIT;
  p.slices = p.outproj == OUT_DEDICATED ? fd_outproj_split_slices() : 3;
  // the last layer's tail also applies post_tfmr + the node residual (FDIPT_KF_UNFOLDED: its own launch)
  p.post = !p.fused_node ? POST_GEMM : unfolded ? POST_CHAIN : POST_TAIL;
  // the last torsion layer (Linear(c_s, 2), fp32) and the backbone atoms ride on the score launch (FDIPT_KF_UNFOLDED: own launches)
  p.torf_fused = (cs & 3) == 0 && !unfolded;
  p.bb_fold = !unfolded;
  // fp16x runs only where its split kernel takes every EdgeTransition, with split operands on the node path; the flags that swap out
  // the split kernels (include/fdipt.h) are refused as well, whichever kernels they would touch at this shape
  p.x = d->precision == FDIPT_PREC_F16X;
  const unsigned x_refused = FDIPT_KF_ET3 | FDIPT_KF_GENERIC_PAIR | FDIPT_KF_GENERIC_ATTN | FDIPT_KF_UNFUSED_NODE | FDIPT_KF_STREAM_ATTN;
  // (the EdgeTransition test only where one runs: the embedder's per-op entry takes any N; N > 1024 is the key-streaming kernels' range)
  const bool runs_et = op == OP_ALL || op == OP_ET;
  p.refused = p.x && ((f & x_refused) || (runs_et && p.et != ET_ET4) || !p.fused_node || N > 1024);
  return p;
}

// ------------------------------------------------------------------ the forward's stages
// L2 warm-up hand-over (common.hpp): the weight images of the launch that follows, which the current launch touches once its own first
// loads are out.  (round 3: the lo images are touched as well — a cold image is one exposed memory round trip per weight tile of the consumer)
enum WarmOf { WARM_QKV, WARM_TAIL, WARM_POST, WARM_TRANSITION, WARM_TRANSITION32, WARM_ET_ROWS, WARM_ET_FOLDED, WARM_TORSION };
// One call of the forward: its inputs and plan, and one const member function per stage (the stages share no mutable state)
struct Fwd {
  const FdiptDims* d;
  const Inventory& iv;
  const DLayout& L;
  const WS& w;
  const ForwardPlan& p;
  const float* P;
  const char* D;
  char* W;
  const void* setup;
  const FdiptForwardArgs* a;
  hipStream_t st;
  int B, N, R, Np;
  size_t NN;
  const float* res_mask = a->res_mask;
  float* F(size_t off) const { return (float*)(W + off); }
  FdStep step() const { return FdStep{a->step_cursor, a->frame_rows, a->state_ring}; }  // which step the cursor-addressed launches work on (all zero: the pointers are the rows)
  // operand-precision view of a weight matrix of the fp32 blob
  const void* WM(const LinW& l) const { return p.bf ? (const void*)((const half_t*)(D + L.h16_base) + l.w) : (const void*)(P + l.w); }
  int lin(const LinW& l, const float* A, int lda, const float* res, int ldr, const float* rm, int relu, float* out, int ldo) const {
    return fd_linear(op_precision(d), R, l.out, l.in, A, lda, WM(l), l.in, P + l.b, res, ldr, rm, relu, out, ldo, st);
  }
  int lin32(const LinW& l, const float* A, int lda, float* out, int ldo) const {
    return fd_linear(FDIPT_PREC_F32, R, l.out, l.in, A, lda, P + l.w, l.in, P + l.b, nullptr, 0, nullptr, 0, out, ldo, st);
  }
  int d2d(void* dst, const void* src, size_t bytes) const {
    return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) == hipSuccess ? FDIPT_OK : FDIPT_ELAUNCH;
  }
  // inner traces (parity tests): rows of width `cols` (leading dimension ld) -> slot of block b
  int inner(int b, int slot, const float* src, int ld, int cols) const {
    if (!a->trace_inner) return FDIPT_OK;
    float* dst = a->trace_inner + ((size_t)(b * 4 + slot) * R) * iv.d_t;
    return hipMemcpy2DAsync(dst, (size_t)iv.d_t * 4, src, (size_t)ld * 4, (size_t)cols * 4, R, hipMemcpyDeviceToDevice, st) == hipSuccess
               ? FDIPT_OK : FDIPT_ELAUNCH;
  }
  bool first_block(int b) const { return b == 0 || p.op != OP_ALL; }  // its buffers' pads are unknown (per-op: the caller's workspace)
  // the pair bias of block b's attention was written (tiled order) by the producer of its z
  bool bias_ready(int b) const { return p.op == OP_ALL && (b == 0 ? p.ee_bias : (p.et == ET_ET3 || p.et == ET_ET4) && p.et_bias); }
  bool fold_et_rows(int b) const { return p.et_rows == ETR_FOLDED && b < d->num_blocks - 1; }
  L2Warm warm_of(int b, WarmOf next, int l = 0) const {
    const DBlock& db = L.blk[b];
    const int cs = d->c_s, dt = iv.d_t;
    const unsigned tb = (unsigned)fd_chain_image_bytes(cs, cs);
    switch (next) {
      case WARM_QKV: {  // layer l's in_proj (fd_seq_qkv)
        const unsigned n = (unsigned)fd_chain_image_bytes(3 * dt, dt);
        return L2Warm{{D + db.ch.inp[l], D + db.lo.inp[l], nullptr}, {n, n, 0}};
      }
      case WARM_TAIL: {  // layer l's tail (fd_tfmr_tail)
        // its three hi images and its three lo images (the last layer's runs end with post_tfmr)
        if (p.tail == NF_ROWS16) return L2Warm{{D + db.lo.o16[l][0], D + db.lo.o16[l][1], nullptr}, {db.lo.tail16_run[l], db.lo.tail16_run[l], 0}};
        const unsigned wimg = (unsigned)fd_chain_image_bytes(dt, dt);
        return L2Warm{{D + db.ch.outp[l], D + db.ch.l1[l], D + db.ch.l2[l]}, {wimg, wimg, wimg}};
      }
      case WARM_POST: return L2Warm{{D + db.ch.post, nullptr, nullptr}, {(unsigned)fd_chain_image_bytes(cs, dt), 0, 0}};
      case WARM_TRANSITION:
        if (p.transition == NF_ROWS16) return L2Warm{{D + db.lo.tr16[0][0], D + db.lo.tr16[0][1], nullptr}, {db.lo.tr16_run, db.lo.tr16_run, 0}};
        return L2Warm{{D + db.ch.t1, D + db.ch.t2, D + db.lo.t1}, {tb, db.ch.t23_run, db.lo.t_run}};
      case WARM_TRANSITION32:  // (the post_tfmr chain hands over the 32-row hi images whatever the transition form)
        return L2Warm{{D + db.ch.t1, D + db.ch.t2, D + db.ch.t3}, {tb, tb, tb}};
      case WARM_ET_ROWS: {  // the EdgeTransition row launch
        const unsigned ei = (unsigned)fd_chain_image_bytes(iv.cb, cs), r4 = (unsigned)fd_chain_image_bytes(2 * (iv.hid + d->c_z), iv.cb);
        return L2Warm{{D + db.ch.et_init, D + db.ch.r4w, D + db.lo.et_init}, {ei, r4, db.lo.et_run}};
      }
      case WARM_ET_FOLDED:  // the transition launch's own later-stage images (hi run, lo run)
        return L2Warm{{D + db.lo.ei16[0], D + db.lo.ei16[1], nullptr}, {db.lo.et16_run, db.lo.et16_run, 0}};
      case WARM_TORSION:
        if (p.torsion == NF_ROWS16) return L2Warm{{D + L.tor16[0][0], D + L.tor16[0][1], nullptr}, {L.tor16_run, L.tor16_run, 0}};
        return L2Warm{{D + L.ch_tor1, D + L.ch_tor2, D + L.lo_tor1}, {tb, tb, L.lo_tor_run}};
    }
    return L2Warm{};
  }
  // ---- Embedder (score_network.py:129-197)
  int embed_stage() const {
    const int cs = d->c_s, cz = d->c_z;
    RC(fd_build_feats(B, N, d->use_aatype, d->index_embed, a->aatype, a->t_emb, a->t_emb_eps, a->fixed_mask, a->idx_emb, F(w.node_feat),
                      L.kn_pad, F(w.pte), L.d1_pad, p.feats_fused ? a->rigids_t : nullptr, a->res_mask, d->coordinate_scaling, F(w.quat),
                      F(w.trans), F(w.dmask), (const float*)(D + L.w1i), (const float*)(D + L.w1j), (const float*)(D + L.b1), cz,
                      p.feats_fused ? F(w.pi) : nullptr, F(w.pj), step(), st));
    if (p.embed == NF_GEMM) {
      RC(fd_linear(op_precision(d), R, cs, L.kn_pad, F(w.node_feat), L.kn_pad, D + L.ne0_pad, L.kn_pad, P + iv.ne0.b, nullptr, 0, nullptr, 1,
                   F(w.h_a), cs, st));
      RC(lin(iv.ne2, F(w.h_a), cs, nullptr, 0, nullptr, 1, F(w.h_b), cs));
      RC(lin(iv.ne4, F(w.h_b), cs, nullptr, 0, nullptr, 0, F(w.h_a), cs));
      RC(fd_layernorm(R, cs, F(w.h_a), cs, nullptr, 0, P + iv.neln.g, P + iv.neln.b, a->res_mask, F(w.node0), cs, st));
    } else {
      const bool r16 = p.embed == NF_ROWS16;
      RowBlockArgs r;
      r.M = R; r.in = F(w.node_feat); r.ld_in = L.kn_pad;
      r.w0 = D + (r16 ? L.ne16[0][0] : L.ch_ne0); r.w1 = D + (r16 ? L.ne16[1][0] : L.ch_ne2); r.w2 = D + (r16 ? L.ne16[2][0] : L.ch_ne4);
      r.w0l = D + (r16 ? L.ne16[0][1] : L.lo_ne0); r.w1l = D + (r16 ? L.ne16[1][1] : L.lo_ne2); r.w2l = D + (r16 ? L.ne16[2][1] : L.lo_ne4);
      r.b0 = P + iv.ne0.b; r.b1 = P + iv.ne2.b; r.b2 = P + iv.ne4.b;
      r.gamma = P + iv.neln.g; r.beta = P + iv.neln.b; r.rowmask_post = a->res_mask; r.out = F(w.node0); r.ld_out = cs;
      if (p.skip == SKIP_EMBED16) {  // skip_embed(init_node) of all blocks as a fourth layer of the same launch
        r.w3 = D + L.skip16[0]; r.w3l = D + L.skip16[1]; r.b3 = (const float*)(D + L.skip_b);
        r.out2 = F(w.skip_all); r.ld_out2 = d->num_blocks * d->c_skip;
        // (the kernel touches its own last stage's images while it starts: they were last read a whole step ago, and so were its own
        // hi / lo runs)
        r.warm = L2Warm{{r.w0, r.w0l, r.w3}, {L.ne16_run, L.ne16_run, L.skip16_run}};
      }
      if (r16) RC(fd_node_embed16(r, L.kn_pad, st));
      else RC(fd_rowblock(L.kn_pad == 72 ? FD_RB_NODE_EMBED_72 : FD_RB_NODE_EMBED_88, r, st));
    }
    if (!p.feats_fused) {
      RC(fd_linear(FDIPT_PREC_F32, R, cz, L.d1_pad, F(w.pte), L.d1_pad, D + L.w1i, L.d1_pad, (const float*)(D + L.b1), nullptr, 0,
                   nullptr, 0, F(w.pi), cz, st));
      RC(fd_linear(FDIPT_PREC_F32, R, cz, L.d1_pad, F(w.pte), L.d1_pad, D + L.w1j, L.d1_pad, nullptr, nullptr, 0, nullptr, 0,
                   F(w.pj), cz, st));
    }
    EdgeEmbedArgs ea;
    ea.B = B; ea.N = N; ea.n_rel = a->n_rel; ea.rel_off = a->rel_off; ea.num_bins = d->num_bins;
    ea.pi = F(w.pi); ea.pj = F(w.pj); ea.rtab = (const float*)setup; ea.dtab = d->num_bins > 0 ? (const float*)(D + L.dtab) : nullptr;
    ea.edges = d->num_bins > 0 ? (const float*)(D + L.edges) : nullptr; ea.seq_idx = a->seq_idx; ea.sc_ca = a->sc_ca_t;
    ea.w2 = WM(iv.ee2); ea.w3 = WM(iv.ee4); ea.b2 = P + iv.ee2.b; ea.b3 = P + iv.ee4.b;
    ea.gamma = P + iv.eeln.g; ea.beta = P + iv.eeln.b; ea.res_mask = a->res_mask; ea.z_out = W + w.z;
    ea.trace = a->trace_edge; ea.reserve_cus = a->reserve_cus;
    ea.wb_img = p.ee_bias ? D + L.blk[0].wb_img4 : nullptr; ea.bb = (const float*)(D + L.blk[0].bb); ea.bias_out = F(w.bias); ea.H = d->no_heads;
    if (p.pz) {
      ea.wdz_img = D + L.blk[0].wdz_imgp; ea.wdz_img_lo = D + L.blk[0].wdz_imgp_lo; ea.bdz = P + iv.blk[0].dz.b; ea.pz_out = (half_t*)(W + w.pz);
    }
    if (p.ee_table) {  // the distinct rows once, then their records to the pairs
      // z0 itself is never written: its only reader, block 0's EdgeTransition, gathers the rows from the table (edge_transition_stage)
      // Samples whose layer-1 rows are bit-identical (a batch stepped at one t) share one set of rows: the device decides who leads
      // (w.ee_lead), the table launch evaluates the leaders' rows, the spread points every pair into its leader's rows.  The region
      // stays sized for B leaders: the host does not know the grouping
      ea.fixed_mask = a->fixed_mask; ea.table = W + w.ee_tab; ea.row_idx = (int32_t*)(W + w.ee_idx); ea.leaders = (int32_t*)(W + w.ee_lead);
      ea.rel_lead = (const int32_t*)((const char*)setup + setup_rel_lead(d, B, a->n_rel));
      RC(fd_edge_embed2_leaders(ea, st));
      RC(fd_edge_embed2_table(ea, D + (p.x ? L.ee2x : L.ee2), st, p.x));
      ea.pz_out = nullptr;  // no pair_z image either: block 0's o_pair gathers the records through the row index (ipa_attend)
      RC(fd_edge_embed2_spread(ea, st, 0));
    } else if (p.regpair) RC(fd_edge_embed2(ea, D + (p.x ? L.ee2x : L.ee2), st, p.x));
    else RC(fd_edge_embed(op_precision(d), cz, ea, st));
    return FDIPT_OK;
  }
  // ---- IPA (ipa_pytorch.py:244-330), part 1: the fused q | kv | q_pts | kv_pts projection and the global-frame points
  int ipa_project(int b, const float* node) const {
    const DBlock& db = L.blk[b];
    const int cs = d->c_s, H = d->no_heads, C = d->c_hidden, Pq = d->no_qk_points, Pv = d->no_v_points, PT = iv.proj_out - 3 * H * C;
    PointsArgs pa;
    pa.B = B; pa.N = N; pa.H = H; pa.Pq = Pq; pa.Pv = Pv; pa.quat = F(w.quat); pa.trans = F(w.trans);
    pa.qp = F(w.qp); pa.kp = F(w.kp); pa.vp = F(w.vp); pa.rot = F(w.rot);
    pa.vpt = p.vpt ? (unsigned short*)(W + w.vpt) : nullptr; pa.Np = Np;
    if (!p.a3) {  // fp32 activations for the LDS / register attention kernels
      RC(fd_linear(op_precision(d), R, iv.proj_out, cs, node, cs, D + db.wproj, cs, (const float*)(D + db.bproj), nullptr, 0,
                   nullptr, 0, F(w.proj), iv.proj_out, st));
      pa.proj = F(w.proj); pa.ld = iv.proj_out; pa.q_off = 3 * H * C; pa.kv_off = 3 * H * C + 3 * H * Pq;
      return fd_points(pa, st);
    }
    pa.kpf = (unsigned short*)(W + w.kpf); pa.gamma = (const float*)(D + db.gamma); pa.res_mask = a->res_mask;
    ProjArgs pj;
    pj.B = B; pj.N = N; pj.H = H; pj.C = C; pj.K = cs; pj.PT = PT; pj.Np = Np; pj.A = node; pj.lda = cs;
    pj.W = D + db.wproj; pj.bias = (const float*)(D + db.bproj); pj.qscale = sqrtf(1.0f / (3.0f * (float)C));
    pj.Qb = (half_t*)(W + w.qb); pj.Kb = (half_t*)(W + w.kb); pj.Vt = (half_t*)(W + w.vt); pj.pts = F(w.pts);
    pj.zero_pads = first_block(b);
    pj.W_img = proj_image(d) ? D + db.wproj_img : nullptr;
    pj.W_img_lo = pj.W_img && p.fused_node ? D + db.wproj_img_lo : nullptr;
    if (p.merged) { pj.merged = 1; pj.W_img = D + db.wproj2_img; pj.W_img_lo = D + db.wproj2_img_lo; pj.bias = (const float*)(D + db.bproj2); }
    if (p.proj_pts) {
      pj.pts_img = 1; pj.W_img = D + db.wproj2p_img; pj.W_img_lo = D + db.wproj2p_img_lo; pj.bias = (const float*)(D + db.bproj2p);
      pj.PT = fd_ipa_proj2_points_cols(H, C) - H * C;
      pj.quat = pa.quat; pj.trans = pa.trans; pj.gamma = pa.gamma; pj.res_mask = pa.res_mask; pj.rot = pa.rot; pj.qp = pa.qp;
      pj.kpf = pa.kpf; pj.vpt = pa.vpt;
    }
    if (p.vt_lo && p.node_rows == NR_PROJ) pj.Vt_lo = (half_t*)(W + w.vt_lo);
    // padded keys and rows 72..95 of the value-point image are never written: zero once per forward (on the launch that zeroes
    // the padded keys of Kb / Vt when the second-generation projection runs)
    const size_t vpt_bytes = (size_t)B * H * 96 * Np * 2;
    bool vpt_zero = pa.vpt && first_block(b);
    if (p.proj2) {
      const bool key_pads = Np > N && p.node_rows == NR_PROJ;  // (fd_node_images writes the padded keys of its images itself)
      if (pj.zero_pads && p.init_fused) {
        SeqInitExtra sx = {vpt_zero ? W + w.vpt : nullptr, vpt_zero ? (long)(vpt_bytes >> 4) : 0L, key_pads ? (void*)pj.Kb : nullptr,
                           (void*)pj.Vt, (long)B * H, C, (void*)pj.Vt_lo};
        RC(fd_seq_images_init(B, N, d->tfmr_heads, a->res_mask, W + w.seqimg, sx, st, p.stream));
        vpt_zero = false;
      } else if (pj.zero_pads && (key_pads || vpt_zero)) {
        ProjArgs pz = pj; pz.W_img = nullptr;
        if (p.node_rows != NR_PROJ) pz.Np = pz.N;  // (no key pads to zero)
        RC(fd_ipa_proj_zero_pads(pz, vpt_zero ? W + w.vpt : nullptr, vpt_zero ? vpt_bytes : 0, st));
        vpt_zero = false;
      }
      RC(fd_ipa_proj2(pj, st));
      half_t* vt_lo = (half_t*)(W + w.vt_lo);  // (the node-row launches: merged projection, which runs on split operands)
      if (p.node_rows == NR_POINTS) { pa.node = node; pa.ld_node = cs; pa.nKb = pj.Kb; pa.nVt = pj.Vt; pa.nVt_lo = vt_lo; }
      if (p.node_rows == NR_LAUNCH) RC(fd_node_images(B, N, Np, node, cs, pj.Kb, pj.Vt, vt_lo, st));
    } else RC(fd_ipa_proj(pj, st));
    if (vpt_zero && hipMemsetAsync(W + w.vpt, 0, vpt_bytes, st) != hipSuccess) return FDIPT_ELAUNCH;
    pa.proj = F(w.pts); pa.ld = PT; pa.q_off = 0; pa.kv_off = 3 * H * Pq;
    if (!p.proj_pts) RC(fd_points(pa, st));
    return FDIPT_OK;
  }
  // ---- IPA, part 2: pair bias, attention (features o and the point features) and o_pair (from z, or from the pair_z image)
  int ipa_attend(int b) const {
    const DBlock& db = L.blk[b];
    const int cz = d->c_z, H = d->no_heads, C = d->c_hidden, Pv = d->no_v_points, feat = iv.feat_dim;
    OPairArgs oa;
    oa.B = B; oa.N = N; oa.H = H; oa.CZ = cz; oa.CD = cz / 4; oa.z = W + w.z; oa.probs = F(w.probs); oa.probs_h16 = nullptr;
    oa.probs_np = 0; oa.out_h16 = nullptr; oa.wdz = (const float*)(D + db.wdz_t); oa.wdz_img = p.bf && dz_images(d) ? D + db.wdz_img : nullptr;
    oa.wdz_img_lo = oa.wdz_img && p.fused_node ? D + db.wdz_img_lo : nullptr; oa.bdz = P + iv.blk[b].dz.b;
    oa.out = F(w.feats); oa.out_ld = feat; oa.off = H * C + 4 * H * Pv;
    if (p.a3) {
      Attn3Args a3;
      a3.B = B; a3.N = N; a3.H = H; a3.Np = Np; a3.Qb = (const half_t*)(W + w.qb); a3.Kb = (const half_t*)(W + w.kb);
      a3.Vt = (const half_t*)(W + w.vt); a3.Vt_lo = p.vt_lo ? (const half_t*)(W + w.vt_lo) : nullptr; a3.kv_per_sample = p.merged;
      a3.bias = F(w.bias); a3.res_mask = res_mask; a3.qp = F(w.qp); a3.kp = F(w.kp); a3.vp = F(w.vp); a3.vpt = (const half_t*)(W + w.vpt);
      a3.kpf = (const half_t*)(W + w.kpf); a3.gamma = (const float*)(D + db.gamma); a3.rot = F(w.rot); a3.trans = F(w.trans);
      a3.probs = F(w.probs); a3.probs_h16 = nullptr; a3.out_h16 = nullptr; a3.out = F(w.feats); a3.out_ld = feat; a3.pt_off = H * C;
      if (!bias_ready(b))
        RC(fd_pair_bias2(B, N, H, W + w.z, D + db.wb, (const float*)(D + db.bb), F(w.bias), 1, st));
      if (p.probs_h16) { a3.probs_h16 = (half_t*)(W + w.probs); oa.probs_h16 = a3.probs_h16; oa.probs_np = Np; }
      RC(p.stream ? fd_attention3_stream(a3, st) : fd_attention3(a3, st));
    } else {
      const long ld = iv.proj_out;
      AttnArgs aa;
      aa.B = B; aa.N = N; aa.H = H;
      aa.q = F(w.proj); aa.q_ld = ld; aa.q_hs = C;
      aa.k = F(w.proj) + H * C; aa.k_ld = ld; aa.k_hs = 2 * C;
      aa.v = F(w.proj) + H * C + C; aa.v_ld = ld; aa.v_hs = 2 * C;
      aa.C = C; aa.Dv = C; aa.scale = sqrtf(1.0f / (3.0f * (float)C));
      aa.bias = F(w.bias); aa.res_mask = res_mask; aa.qp = F(w.qp); aa.kp = F(w.kp); aa.vp = F(w.vp); aa.Pq = d->no_qk_points; aa.Pv = Pv;
      aa.gamma = (const float*)(D + db.gamma); aa.rot = F(w.rot); aa.trans = F(w.trans); aa.probs = F(w.probs);
      aa.out = F(w.feats); aa.out_ld = feat; aa.pt_off = H * C; aa.lds_s = 0;
      if (p.ipa_bias_f32)
        RC(fd_pair_bias_f32((long)NN, H, cz, F(w.z), (const float*)(D + db.wb), (const float*)(D + db.bb), F(w.bias), st));  // [B,N,N,H]
      else
        RC(fd_linear_z(op_precision(d), (long)NN, H, cz, W + w.z, D + db.wb, (const float*)(D + db.bb), F(w.bias), st));  // [B,N,N,H]
      if (p.ipa_attn_f32 && fd_ipa_attention_f32_supported(aa)) RC(fd_ipa_attention_f32(aa, st));  // scores in registers (round 5)
      else RC(fd_attention(op_precision(d), 1, aa, st));
    }
    if (p.pz) {  // (z itself may not have been stored)
      if (!oa.probs_h16) return FDIPT_EINVAL;
      if (p.ee_table && b == 0) {  // the embedder wrote no image: the records of the (L2-resident) leaders' rows, by row index
        oa.pz_idx = (const int32_t*)(W + w.ee_idx);
        oa.pz_rows = fd_ee2_table_pz(W + w.ee_tab, B, a->n_rel, d->num_bins);
      } else oa.pz = (const half_t*)(W + w.pz);
      return fd_opair_pz(oa, st);
    }
    return fd_opair(op_precision(d), oa, st, p.stream);
  }
  // ---- IPA, part 3: node = LN(node + linear_out(features)) in tf_in[:, :cs]; tf_in[:, cs:] = skip_embed(init_node)   (ipa:531-535)
  int ipa_out(int b, const float* node) const {
    const BlockW& k = iv.blk[b];
    const DBlock& db = L.blk[b];
    const int cs = d->c_s, dt = iv.d_t, feat = iv.feat_dim;
    const float* wout = p.merged ? (const float*)(D + db.wout_m) : P + k.out.w;
    const float* bout = p.merged ? (const float*)(D + db.bout_m) : P + k.out.b;
    if (p.outproj == OUT_GEMM) {  // (skip_embed per block: the batched launches need the split-K LayerNorm)
      RC(lin(k.out, F(w.feats), feat, nullptr, 0, res_mask, 0, F(w.ipa_out), cs));
      RC(fd_layernorm(R, cs, node, cs, F(w.ipa_out), cs, P + k.ipa_ln.g, P + k.ipa_ln.b, nullptr, F(w.tf_in), dt, st));
      RC(inner(b, 0, F(w.ipa_out), cs, cs));
      RC(inner(b, 1, F(w.tf_in), dt, cs));
      return lin(k.skip, F(w.node0), cs, nullptr, 0, nullptr, 0, F(w.tf_in) + cs, dt);
    }
    if (p.outproj == OUT_DEDICATED)
      RC(fd_outproj_split(R, cs, feat, F(w.feats), feat, D + db.wout_img, D + db.wout_img_lo, bout, res_mask, F(w.ipa_parts), (long)R * cs, cs, st));
    else
      RC(fd_linear_splitk_split(R, cs, feat, p.slices, F(w.feats), feat, wout, feat, bout, res_mask, F(w.ipa_parts), (long)R * cs, cs, st));
    // the slices summed in the LayerNorm, which also copies skip_embed(init_node) of this block behind its output when that ran batched
    const bool skip_batched = p.skip != SKIP_PER_BLOCK;
    const L2Warm warm = warm_of(b, WARM_QKV, 0);
    RC(fd_layernorm_parts(R, cs, node, cs, F(w.ipa_parts), cs, p.slices, (long)R * cs, P + k.ipa_ln.g, P + k.ipa_ln.b, nullptr,
                          F(w.tf_in), dt, skip_batched ? F(w.skip_all) + (size_t)b * d->c_skip : nullptr,
                          d->num_blocks * d->c_skip, d->c_skip, p.seq == SEQ_FUSED ? &warm : nullptr, st));
    if (!skip_batched) RC(lin(k.skip, F(w.node0), cs, nullptr, 0, nullptr, 0, F(w.tf_in) + cs, dt));
    return FDIPT_OK;
  }
  // ---- nn.TransformerEncoder, post-norm (ipa:433-443,536-538) on tf_in -> *x_out (not written when post_tfmr rides on the last tail:
  // that tail writes node + post_tfmr(x) to h_a)
  int seq_stage(int b, const float** x_out) const {
    const BlockW& k = iv.blk[b];
    const DBlock& db = L.blk[b];
    const int dt = iv.d_t, cs = d->c_s, th = d->tfmr_heads, hd = dt / th;
    const float* x = F(w.tf_in);
    for (int l = 0; l < d->tfmr_layers; ++l) {
      const TfLayer& t = k.tf[l];
      const bool last = l + 1 == d->tfmr_layers;
      if (p.seq == SEQ_FUSED) {  // default bf16 path: in_proj writes the attention operand images directly (attention_seq.hip)
        if (b == 0 && l == 0 && !p.init_fused) RC(fd_seq_images_init(B, N, th, res_mask, W + w.seqimg, SeqInitExtra{}, st, p.stream));
        RC(fd_seq_qkv(B, N, th, x, dt, D + db.ch.inp[l], D + db.lo.inp[l], P + t.inp.b, 1.0f / sqrtf((float)hd),
                      W + w.seqimg, st));
        const L2Warm wt = warm_of(b, WARM_TAIL, l);  // ... and the attention touches the weights of the layer's tail kernel, launched next
        RC(fd_seq_attention_run(B, N, th, W + w.seqimg, F(w.att), dt, &wt, st, p.stream));
      } else {
        RC(lin(t.inp, x, dt, nullptr, 0, nullptr, 0, F(w.qkv), 3 * dt));
        AttnArgs ta = {};
        ta.B = B; ta.N = N; ta.H = th;
        ta.q = F(w.qkv); ta.k = F(w.qkv) + dt; ta.v = F(w.qkv) + 2 * dt;
        ta.q_ld = ta.k_ld = ta.v_ld = 3 * dt; ta.q_hs = ta.k_hs = ta.v_hs = hd;
        ta.C = hd; ta.Dv = hd; ta.scale = 1.0f / sqrtf((float)hd); ta.res_mask = res_mask; ta.out = F(w.att); ta.out_ld = dt;
        if (p.seq == SEQ_BF16) RC(fd_seq_attention(B, N, th, F(w.qkv), 3 * dt, ta.scale, res_mask, W + w.seqimg, F(w.att), dt, st, p.stream));
        else if (p.seq == SEQ_F32) RC(fd_seq_attention_f32(B, N, th, F(w.qkv), 3 * dt, ta.scale, res_mask, F(w.att), dt, st));
        else RC(fd_attention(op_precision(d), 0, ta, st));
      }
      // x_a = norm1(x + out_proj(att)); x_b = norm2(x_a + linear2(relu(linear1(x_a))))
      if (p.tail == NF_GEMM) {
        RC(lin(t.outp, F(w.att), dt, nullptr, 0, nullptr, 0, F(w.ff), dt));
        RC(fd_layernorm(R, dt, x, dt, F(w.ff), dt, P + t.n1.g, P + t.n1.b, nullptr, F(w.x_a), dt, st));
        RC(lin(t.l1, F(w.x_a), dt, nullptr, 0, nullptr, 1, F(w.ff), dt));
        RC(lin(t.l2, F(w.ff), dt, nullptr, 0, nullptr, 0, F(w.att), dt));
        RC(fd_layernorm(R, dt, F(w.x_a), dt, F(w.att), dt, P + t.n2.g, P + t.n2.b, nullptr, F(w.x_b), dt, st));
        x = F(w.x_b);  // next layer: norm1 reads x_b -> x_a, norm2 reads x_a/att -> x_b (no aliasing)
        continue;
      }
      const bool r16 = p.tail == NF_ROWS16;  // 16-row blocks (150 blocks at 2400 rows)
      TfmrTailArgs tt;
      tt.M = R; tt.ld = dt; tt.att = F(w.att); tt.x = x;
      tt.wo = D + (r16 ? db.lo.o16[l][0] : db.ch.outp[l]); tt.w1 = D + (r16 ? db.lo.f16[l][0] : db.ch.l1[l]); tt.w2 = D + (r16 ? db.lo.g16[l][0] : db.ch.l2[l]);
      tt.wol = D + (r16 ? db.lo.o16[l][1] : db.lo.outp[l]); tt.w1l = D + (r16 ? db.lo.f16[l][1] : db.lo.l1[l]); tt.w2l = D + (r16 ? db.lo.g16[l][1] : db.lo.l2[l]);
      tt.bo = P + t.outp.b; tt.g1 = P + t.n1.g; tt.be1 = P + t.n1.b; tt.b1 = P + t.l1.b; tt.b2 = P + t.l2.b; tt.g2 = P + t.n2.g;
      tt.be2 = P + t.n2.b; tt.out = x == F(w.x_b) ? F(w.x_a) : F(w.x_b);
      tt.rows16 = r16;
      const bool post_here = last && p.post == POST_TAIL;
      if (post_here) {
        tt.wp = D + (r16 ? db.lo.p16[0] : db.ch.post); tt.wpl = D + (r16 ? db.lo.p16[1] : db.lo.post);
        tt.bp = P + k.post.b; tt.pres = F(w.tf_in); tt.ld_pres = dt; tt.pout = F(w.h_a); tt.ld_pout = cs;
      }
      // next launch: the following layer's in_proj, or the transition / post_tfmr
      if (!last) tt.warm = p.seq == SEQ_FUSED ? warm_of(b, WARM_QKV, l + 1) : L2Warm{};
      else tt.warm = warm_of(b, post_here ? WARM_TRANSITION : WARM_POST);
      RC(fd_tfmr_tail(tt, st));
      x = tt.out;
    }
    *x_out = x;
    return FDIPT_OK;
  }
  // ---- node = node + post_tfmr(x); StructureModuleTransition; mask (ipa:539-541, 36-58); BackboneUpdate + compose_q_update_vec
  // (ipa:542-547): the new node rows in w.node
  int transition_stage(int b, const float* x) const {
    const BlockW& k = iv.blk[b];
    const DBlock& db = L.blk[b];
    const int cs = d->c_s, dt = iv.d_t;
    if (p.post == POST_CHAIN) {
      ChainArgs c;
      c.M = R; c.in = x; c.ld_in = dt; c.w[0] = D + db.ch.post; c.b[0] = P + k.post.b; c.residual = F(w.tf_in); c.ld_res = dt;
      c.out = F(w.h_a); c.ld_out = cs;
      c.warm = warm_of(b, WARM_TRANSITION32);
      RC(fd_chain(FD_CHAIN_POST, c, st));
    } else if (p.post == POST_GEMM) RC(lin(k.post, x, dt, F(w.tf_in), dt, nullptr, 0, F(w.h_a), cs));
    if (p.transition == NF_GEMM) {
      RC(lin(k.t1, F(w.h_a), cs, nullptr, 0, nullptr, 1, F(w.h_b), cs));
      RC(lin(k.t2, F(w.h_b), cs, nullptr, 0, nullptr, 1, F(w.ipa_out), cs));
      RC(lin(k.t3, F(w.ipa_out), cs, F(w.h_a), cs, nullptr, 0, F(w.h_b), cs));
      RC(fd_layernorm(R, cs, F(w.h_b), cs, nullptr, 0, P + k.tln.g, P + k.tln.b, a->res_mask, F(w.node), cs, st));
      // bb_update(node*diffuse_mask) differs from bb_update(node) only on rows whose update is masked out below, so the input mask is
      // not materialised
      RC(lin32(k.bb, F(w.node), cs, F(w.upd), 8));
      RC(inner(b, 3, F(w.upd), 8, 6));
      return fd_compose_q_update(R, F(w.quat), F(w.trans), F(w.upd), 8, F(w.dmask), st);
    }
    // ... with BackboneUpdate + compose_q_update_vec fused in (the fp32 Linear c_s -> 6 is a per-row dot product)
    const bool r16 = p.transition == NF_ROWS16;  // 16-row blocks (rowblock.hip: transition16_kernel)
    RowBlockArgs r;
    r.M = R; r.in = F(w.h_a); r.ld_in = cs;
    r.w0 = D + (r16 ? db.lo.tr16[0][0] : db.ch.t1); r.w1 = D + (r16 ? db.lo.tr16[1][0] : db.ch.t2); r.w2 = D + (r16 ? db.lo.tr16[2][0] : db.ch.t3);
    r.w0l = D + (r16 ? db.lo.tr16[0][1] : db.lo.t1); r.w1l = D + (r16 ? db.lo.tr16[1][1] : db.lo.t2); r.w2l = D + (r16 ? db.lo.tr16[2][1] : db.lo.t3);
    r.b0 = P + k.t1.b; r.b1 = P + k.t2.b; r.b2 = P + k.t3.b; r.residual = F(w.h_a); r.ld_res = cs; r.gamma = P + k.tln.g; r.beta = P + k.tln.b;
    r.rowmask_post = a->res_mask; r.out = F(w.node); r.ld_out = cs; r.bb_w = P + k.bb.w; r.bb_b = P + k.bb.b;
    r.upd_mask = F(w.dmask); r.quat = F(w.quat); r.trans = F(w.trans);
    // next launch: the EdgeTransition row launch, or the torsion head
    if (b < d->num_blocks - 1 && p.et_widths) r.warm = warm_of(b, WARM_ET_ROWS);
    else if (b == d->num_blocks - 1) r.warm = warm_of(b, WARM_TORSION);
    if (fold_et_rows(b)) {
      // EdgeTransition's row launch (e = initial_embed(node), fold columns -> edge_transition4's images) folded into this launch: the
      // rows it needs are this launch's output rows
      r.we0 = D + db.lo.ei16[0]; r.we0l = D + db.lo.ei16[1]; r.we1 = D + db.lo.r416[0]; r.we1l = D + db.lo.r416[1];
      r.be0 = P + k.et_init.b; r.be1 = (const float*)(D + db.ch.r4b);
      r.img_a = W + w.a1img; r.img_b = W + w.b1img; r.img_B = B; r.img_N = N;
      r.warm = warm_of(b, WARM_ET_FOLDED);
    }
    if (r16) return fd_transition16(r, st);
    return fd_rowblock(FD_RB_TRANSITION_BB, r, st);
  }
  // ---- EdgeTransition of block b (ipa:565-572 / 60-96): z <- EdgeTransition(node, z)
  int edge_transition_stage(int b, const float* node) const {
    const BlockW& k = iv.blk[b];
    const DBlock& db = L.blk[b];
    const int cs = d->c_s, cz = d->c_z;
    // the per-residue rows: e = initial_embed(node) and the e_i / e_j parts of the concat-free layers in ONE row-block launch
    RowBlockArgs r;
    r.M = R; r.in = node; r.ld_in = cs; r.w0 = D + db.ch.et_init; r.b0 = P + k.et_init.b;
    if (p.et == ET_ET4 && !fold_et_rows(b)) {  // [A1 | Af | B1 | Bf] as edge_transition4's fold-fragment images
      r.w1 = D + db.ch.r4w; r.b1 = (const float*)(D + db.ch.r4b); r.out = F(w.r4); r.ld_out = 1024;
      r.img_a = W + w.a1img; r.img_b = W + w.b1img; r.img_B = B; r.img_N = N;
      if (p.et_rows == ETR_ROWS) {
        RC(fd_rowblock(FD_RB_ET4_ROWS, r, st));
        RC(fd_et4_row_images(F(w.r4), B, N, W + w.a1img, W + w.b1img, st));
      } else {  // the row-block epilogue writes the fold-fragment images itself
        r.w0l = D + db.lo.et_init; r.w1l = D + db.lo.r4w;
        RC(fd_rowblock(FD_RB_ET4_IMAGES, r, st));
      }
    } else if (p.et == ET_ET3) {  // A1 | Af rows and e in half precision
      r.w1 = D + db.ch.a1af; r.b1 = (const float*)(D + db.ch.b1f); r.out = F(w.a1); r.ld_out = iv.hid; r.out2 = F(w.af); r.ld_out2 = cz;
      r.split = iv.hid; r.hid_h16 = (unsigned short*)(W + w.e_bf);
      RC(fd_rowblock(FD_RB_ET_ROWS, r, st));
    } else if (p.et == ET_CHAIN) {
      ChainArgs c;
      c.M = R; c.in = node; c.ld_in = cs; c.w[0] = D + db.ch.et_init; c.b[0] = P + k.et_init.b; c.out_h16 = (unsigned short*)(W + w.e_bf);
      c.out = F(w.e); c.ld_out = iv.cb;
      RC(fd_chain(FD_CHAIN_ETINIT, c, st));
    } else if (p.et == ET_GEMM) {
      RC(lin(k.et_init, node, cs, nullptr, 0, nullptr, 0, F(w.e), iv.cb));
      if (p.bf) RC(fd_f32_to_half((long)R * iv.cb, F(w.e), (half_t*)(W + w.e_bf), st));
    }
    float* tr_ptr = a->trace_edge ? a->trace_edge + (size_t)(b + 1) * NN * cz : nullptr;
    if (a->ev_start && a->ev_start[b]) hipEventRecord((hipEvent_t)a->ev_start[b], st);
    if (p.et == ET_ET4 || p.et == ET_ET3) {
      ET2Args t2;
      t2.B = B; t2.N = N; t2.z_in = (const half_t*)(W + w.z); t2.z_out = (half_t*)(W + w.z); t2.e = F(w.e);
      t2.e_h16 = (const half_t*)(W + w.e_bf);
      t2.a1 = F(w.a1); t2.af = F(w.af); t2.stream = D + (p.et == ET_ET3 ? db.et3 : p.x ? db.et4x : db.et4); t2.b2 = P + k.et2.b; t2.gamma = P + k.et_ln.g;
      t2.beta = P + k.et_ln.b; t2.res_mask = a->res_mask; t2.trace = tr_ptr;
      // the next block's attention consumes linear_b(z') in fragment order when it runs attention3
      // (end to end +0.8 % at N = 300: the launch grows by about as much as the pair_bias2 launch it replaces, the gain
      //  is the z re-read that disappears; FDIPT_KF_UNFOLDED restores the separate pass)
      const DBlock& next = L.blk[b + 1];
      t2.wb_img = p.et_bias ? D + (p.et == ET_ET4 ? next.wb_img4 : next.wb_img3) : nullptr;
      t2.a1_img = W + w.a1img; t2.b1_img = W + w.b1img;
      t2.bb = (const float*)(D + next.bb); t2.bias_out = F(w.bias); t2.H = d->no_heads; t2.reserve_cus = a->reserve_cus;
      if (p.pz) {
        t2.bdz = P + iv.blk[b + 1].dz.b; t2.pz_out = (half_t*)(W + w.pz);  // (down_z itself: the last chunk of the weight stream)
        // the last EdgeTransition of the trunk: block b + 1 takes bias and pair_z from this epilogue and no launch reads z' itself
        if (b + 1 == d->num_blocks - 1 && !tr_ptr) t2.z_out = nullptr;
      }
      t2.clock = a->clock_out;
      if (p.ee_table && b == 0) {  // z0 lives in the embedder's row table only (its z rows lead the table)
        t2.z_in = (const half_t*)(W + w.ee_tab); t2.z_idx = (const int32_t*)(W + w.ee_idx);
      }
      if (p.et == ET_ET4) RC(fd_edge_transition4(t2, st, p.x));
      else RC(fd_edge_transition3(t2, st));
    } else {
      EdgeTransArgs ta;
      ta.B = B; ta.N = N; ta.z_in = W + w.z; ta.z_out = W + w.z; ta.e = F(w.e);
      ta.w1 = WM(k.et1); ta.w2 = WM(k.et2); ta.wf = WM(k.etf); ta.b1 = P + k.et1.b; ta.b2 = P + k.et2.b; ta.bf = P + k.etf.b;
      ta.gamma = P + k.et_ln.g; ta.beta = P + k.et_ln.b; ta.res_mask = a->res_mask; ta.trace = tr_ptr; ta.clock = a->clock_out;
      RC(fd_edge_transition(op_precision(d), cz, iv.cb, ta, st));
    }
    if (a->ev_stop && a->ev_stop[b]) hipEventRecord((hipEvent_t)a->ev_stop[b], st);
    return FDIPT_OK;
  }
  // ---- heads: torsion (ipa:332-363), tensor_7, scores (ipa:552-564), backbone (sn:269-273)
  int heads_stage(const float* node) const {
    const int cs = d->c_s;
    if (p.torsion == NF_GEMM) {
      RC(lin(iv.tor1, node, cs, nullptr, 0, nullptr, 1, F(w.h_a), cs));
      RC(lin(iv.tor2, F(w.h_a), cs, node, cs, nullptr, 0, F(w.h_b), cs));
    } else {
      const bool r16 = p.torsion == NF_ROWS16;
      RowBlockArgs r;
      r.M = R; r.in = node; r.ld_in = cs; r.w0 = D + (r16 ? L.tor16[0][0] : L.ch_tor1); r.w1 = D + (r16 ? L.tor16[1][0] : L.ch_tor2);
      r.w0l = D + (r16 ? L.tor16[0][1] : L.lo_tor1); r.w1l = D + (r16 ? L.tor16[1][1] : L.lo_tor2);
      r.b0 = P + iv.tor1.b; r.b1 = P + iv.tor2.b; r.residual = node; r.ld_res = cs; r.out = F(w.h_b); r.ld_out = cs;
      if (r16) RC(fd_torsion16(r, st));
      else RC(fd_rowblock(FD_RB_TORSION, r, st));
    }
    if (!p.torf_fused) RC(lin32(iv.torf, F(w.h_b), cs, F(w.psi_un), 8));
    // tensor_7 / psi epilogue, R^3 score and IGSO(3) score in one launch (frames.hip); the backbone atoms of the finished frames ride on it
    // (one atom per lane of a residue's 16) unless the launch folds are off
    const bool atoms = a->atom37 || a->atom14;
    if (atoms && !a->bb_tables) return FDIPT_EINVAL;
    const bool bb_fold = atoms && p.bb_fold;
    RC(fd_score_tail(B, N, a->rigids_t, F(w.quat), F(w.trans), d->coordinate_scaling, F(w.psi_un), 8, a->gt_psi, a->fixed_mask,
                     a->res_mask, a->so3_sigma, a->t, d->r3_min_b, d->r3_max_b, a->rigids, a->psi, a->rot_score, a->trans_score,
                     a->ca_out, p.torf_fused ? F(w.h_b) : nullptr, cs, cs, P + iv.torf.w, P + iv.torf.b, a->so3_score_table,
                     a->so3_omega_edges, a->so3_num_omega, a->aatype, bb_fold ? a->bb_tables : nullptr, bb_fold ? a->atom37 : nullptr,
                     bb_fold ? a->atom14 : nullptr, step(), st));
    // kept frames: the row of the map, nothing on a step that keeps none (atom14 is not built)
    if (atoms && !bb_fold && (a->atom37 || !a->frame_rows))
      RC(fd_backbone(R, a->rigids, nullptr, nullptr, 0, a->psi, a->aatype, a->bb_tables, a->atom37, a->frame_rows ? nullptr : a->atom14, st, step()));
    return FDIPT_OK;
  }
};

static int forward_impl(const FdiptDims* d, const float* P, const void* derived, const void* setup,
                        const FdiptForwardArgs* a, void* workspace, size_t workspace_bytes, fdipt_stream_t stream, const OpSel& op) {
  if (!dims_ok(d) || !P || !derived || !a || !workspace) return FDIPT_EINVAL;
  if (a->B <= 0 || a->N <= 0 || !a->res_mask) return FDIPT_EINVAL;
  if (op.kind == OP_ALL || op.kind == OP_EMBED) {
    if (!setup || !a->fixed_mask || (!a->sc_ca_t && d->num_bins > 0) || !a->seq_idx || !a->idx_emb || !a->t_emb) return FDIPT_EINVAL;
    if (d->use_aatype && (!a->aatype || !a->t_emb_eps)) return FDIPT_EINVAL;
  }
  if (op.kind == OP_ALL && (!a->rigids_t || !a->gt_psi || !a->t || !a->so3_sigma || !a->psi || !a->rot_score || !a->trans_score ||
                            !a->rigids))
    return FDIPT_EINVAL;
  if ((op.kind == OP_POINTS || op.kind == OP_IPA) && !a->rigids_t) return FDIPT_EINVAL;
  if (!FdStep{a->step_cursor, a->frame_rows, a->state_ring}.valid()) return FDIPT_EINVAL;  // kept-frame addressing is the cursor's
  if (op.kind != OP_ALL && op.kind != OP_EMBED && (op.block < 0 || op.block >= d->num_blocks - (op.kind == OP_ET ? 1 : 0))) return FDIPT_EINVAL;
  Inventory iv;
  DLayout L;
  WS w;
  build_inventory(d, iv);
  blob_walk(d, iv, L);
  const int B = a->B, N = a->N, R = B * N;
  build_ws(d, iv, L, B, N, w);
  if (workspace_bytes < w.total) return FDIPT_ESIZE;
  if ((long)B * N * N > 2000000000L / 1) return FDIPT_ESIZE;
  const ForwardPlan p = plan_forward(d, iv, L, B, N, op.kind, a->n_rel, a->trace_edge != nullptr, a->pair_embed != 0);
  if (p.refused) return FDIPT_EINVAL;
  const Fwd f = {d, iv, L, w, p, P, (const char*)derived, (char*)workspace, setup, a, (hipStream_t)stream, B, N, R, (N + 31) / 32 * 32, (size_t)R * N};
  if (a->trace_inner && (p.fused_node || p.outproj != OUT_GEMM)) return FDIPT_EINVAL;  // fused node path: the tensors never exist
  const size_t node_bytes = (size_t)R * d->c_s * 4, z_bytes = f.NN * d->c_z * L.esz;
  if (op.kind == OP_ALL || op.kind == OP_EMBED) RC(f.embed_stage());
  if (op.kind == OP_EMBED) {
    if (op.node_out) RC(f.d2d(op.node_out, f.F(w.node0), node_bytes));
    if (op.z_out) RC(f.d2d(op.z_out, f.W + w.z, z_bytes));
    return FDIPT_OK;
  }
  if (a->trace_node && op.kind == OP_ALL) RC(f.d2d(a->trace_node, f.F(w.node0), node_bytes));
  if (!p.feats_fused && a->rigids_t)
    RC(fd_split_rigids(R, a->rigids_t, d->coordinate_scaling, a->res_mask, a->fixed_mask ? a->fixed_mask : a->res_mask, f.F(w.quat),
                       f.F(w.trans), f.F(w.dmask), f.step(), f.st));
  if (op.kind != OP_ALL) {  // per-op entry: the sub-module's inputs come from the caller; one block, cut at the sub-module's boundary
    if (!op.node_in) return FDIPT_EINVAL;
    RC(f.d2d(f.F(w.node), op.node_in, node_bytes));
    if (op.kind != OP_POINTS) {
      if (!op.z_in) return FDIPT_EINVAL;
      RC(f.d2d(f.W + w.z, op.z_in, z_bytes));
    }
    const int b = op.block;
    if (op.kind == OP_ET) {
      RC(f.edge_transition_stage(b, f.F(w.node)));
      if (!op.z_out) return FDIPT_EINVAL;
      return f.d2d(op.z_out, f.W + w.z, z_bytes);
    }
    RC(f.ipa_project(b, f.F(w.node)));
    if (op.kind == OP_POINTS) {
      if (!op.qp || !op.kp || !op.vp) return FDIPT_EINVAL;
      const size_t qk = (size_t)R * d->no_heads * d->no_qk_points * 3 * 4;
      RC(f.d2d(op.qp, f.F(w.qp), qk));
      RC(f.d2d(op.kp, f.F(w.kp), qk));
      return f.d2d(op.vp, f.F(w.vp), (size_t)R * d->no_heads * d->no_v_points * 3 * 4);
    }
    RC(f.ipa_attend(b));
    // linear_out(features) * mask as one GEMM (the forward sums split-K slices in its LayerNorm)
    RC(f.lin(iv.blk[b].out, f.F(w.feats), iv.feat_dim, nullptr, 0, a->res_mask, 0, f.F(w.ipa_out), d->c_s));
    if (!op.out) return FDIPT_EINVAL;
    return f.d2d(op.out, f.F(w.ipa_out), node_bytes);
  }
  const int cs = d->c_s, nsk = d->num_blocks * d->c_skip;
  if (p.skip == SKIP_SPLITK)
    RC(fd_linear_splitk_split(R, nsk, cs, 1, f.F(w.node0), cs, (const float*)(f.D + L.skip_w32), cs, (const float*)(f.D + L.skip_b),
                              nullptr, f.F(w.skip_all), 0, nsk, f.st));
  const float* node = f.F(w.node0);
  for (int b = 0; b < d->num_blocks; ++b) {
    const float* x;
    RC(f.ipa_project(b, node));
    RC(f.ipa_attend(b));
    RC(f.ipa_out(b, node));
    RC(f.seq_stage(b, &x));
    RC(f.inner(b, 2, x, iv.d_t, iv.d_t));
    RC(f.transition_stage(b, x));
    node = f.F(w.node);
    if (b < d->num_blocks - 1) RC(f.edge_transition_stage(b, node));
    if (a->trace_node) RC(f.d2d(a->trace_node + (size_t)(b + 1) * R * cs, node, node_bytes));
  }
  return f.heads_stage(node);
}

extern "C" {

int64_t fdipt_embed_table_rows(const FdiptDims* d, int B, int N, int n_rel) {
  if (!dims_ok(d) || B <= 0 || N <= 0 || n_rel <= 0) return 0;
  Inventory iv;
  DLayout L;
  build_inventory(d, iv);
  blob_walk(d, iv, L);
  const ForwardPlan p = plan_forward(d, iv, L, B, N, OP_ALL, n_rel, false, false);
  return p.ee_table && !p.refused ? (int64_t)n_rel * (d->num_bins + 1) : 0;
}

int fdipt_embed_table_leaders(const FdiptDims* d, const void* workspace, int B, int N, int n_rel, int32_t* out_dev) {
  if (!workspace || !out_dev || fdipt_embed_table_rows(d, B, N, n_rel) <= 0) return FDIPT_EINVAL;
  Inventory iv;
  DLayout L;
  WS w;
  build_inventory(d, iv);
  blob_walk(d, iv, L);
  build_ws(d, iv, L, B, N, w);
  if (hipDeviceSynchronize() != hipSuccess) return FDIPT_ELAUNCH;  // (a diagnostic entry: whatever stream the forward ran on)
  return hipMemcpy(out_dev, (const char*)workspace + w.ee_lead, (size_t)B * 4, hipMemcpyDeviceToDevice) == hipSuccess ? FDIPT_OK : FDIPT_ELAUNCH;
}

int fdipt_score_forward(const FdiptDims* d, const float* P, const void* derived, const void* setup,
                        const FdiptForwardArgs* a, void* workspace, size_t workspace_bytes, fdipt_stream_t stream) {
  return forward_impl(d, P, derived, setup, a, workspace, workspace_bytes, stream, OpSel{});
}

int fdipt_edge_embed_fwd(const FdiptDims* d, const float* P, const void* derived, const void* setup, const FdiptForwardArgs* a,
                         float* node_out, void* z_out, void* workspace, size_t workspace_bytes, fdipt_stream_t stream) {
  OpSel op;
  op.kind = OP_EMBED; op.node_out = node_out; op.z_out = z_out;
  return forward_impl(d, P, derived, setup, a, workspace, workspace_bytes, stream, op);
}

static FdiptForwardArgs op_args(int B, int N, const float* rigids_t, const float* res_mask) {
  FdiptForwardArgs a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.N = N; a.rigids_t = rigids_t; a.res_mask = res_mask;
  return a;
}
int fdipt_ipa_project_points(const FdiptDims* d, const float* P, const void* derived, int block, int B, int N, const float* node,
                             const float* rigids, const float* res_mask, float* q_pts, float* k_pts, float* v_pts,
                             void* workspace, size_t workspace_bytes, fdipt_stream_t stream) {
  OpSel op;
  op.kind = OP_POINTS; op.block = block; op.node_in = node; op.qp = q_pts; op.kp = k_pts; op.vp = v_pts;
  const FdiptForwardArgs a = op_args(B, N, rigids, res_mask);
  return forward_impl(d, P, derived, nullptr, &a, workspace, workspace_bytes, stream, op);
}
int fdipt_ipa_attention_fwd(const FdiptDims* d, const float* P, const void* derived, int block, int B, int N, const float* node,
                            const void* z, const float* rigids, const float* res_mask, float* out, void* workspace,
                            size_t workspace_bytes, fdipt_stream_t stream) {
  OpSel op;
  op.kind = OP_IPA; op.block = block; op.node_in = node; op.z_in = z; op.out = out;
  const FdiptForwardArgs a = op_args(B, N, rigids, res_mask);
  return forward_impl(d, P, derived, nullptr, &a, workspace, workspace_bytes, stream, op);
}
int fdipt_edge_transition_fwd(const FdiptDims* d, const float* P, const void* derived, int block, int B, int N, const float* node,
                              const float* res_mask, const void* z_in, void* z_out, void* workspace, size_t workspace_bytes,
                              fdipt_stream_t stream) {
  OpSel op;
  op.kind = OP_ET; op.block = block; op.node_in = node; op.z_in = z_in; op.z_out = z_out;
  const FdiptForwardArgs a = op_args(B, N, nullptr, res_mask);
  return forward_impl(d, P, derived, nullptr, &a, workspace, workspace_bytes, stream, op);
}

int fdipt_event_create(void** ev_host) {
  if (!ev_host) return FDIPT_EINVAL;
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return FDIPT_ELAUNCH;
  *ev_host = (void*)e;
  return FDIPT_OK;
}
int fdipt_event_destroy(void* ev) { return hipEventDestroy((hipEvent_t)ev) == hipSuccess ? FDIPT_OK : FDIPT_ELAUNCH; }
int fdipt_event_record(void* ev, fdipt_stream_t s) {
  return hipEventRecord((hipEvent_t)ev, (hipStream_t)s) == hipSuccess ? FDIPT_OK : FDIPT_ELAUNCH;
}
int fdipt_event_elapsed_ms(void* start, void* stop, float* ms_host) {
  if (!ms_host) return FDIPT_EINVAL;
  if (hipEventSynchronize((hipEvent_t)stop) != hipSuccess) return FDIPT_ELAUNCH;
  return hipEventElapsedTime(ms_host, (hipEvent_t)start, (hipEvent_t)stop) == hipSuccess ? FDIPT_OK : FDIPT_ELAUNCH;
}

}  // extern "C"
