/*
 * fdipt.h — C ABI of libfdipt_hip.so: MI355X (gfx950) kernels for the FrameDiPT sampler hot path.
 *
 * The reference (instadeepai/FrameDiPT) is pure Python/PyTorch and has no FFI; this ABI is the
 * boundary a maintainer binds with ctypes.  Each entry point names the
 * reference function(s) it replaces (paths relative to the reference repository root).
 *
 * Conventions
 *   - every function returns 0 on success, a negative FDIPT_E* code otherwise; no exceptions,
 *     no allocation, no global mutable state; one hipStream_t per call (passed as void*).  Calls for different devices
 *     are independent, and so are calls on different streams of one device as long as they share no output / workspace buffer
 *     (forwards of TWO sub-batches may be in flight together: FdiptForwardArgs.reserve_cus; verified bit-identical to the
 *     sequential result in long soaks for two streams, NOT for three or more — DESIGN.md section 5 — so the Python host
 *     refuses more than two).  No device-side state survives a call outside caller-owned buffers; the only atomics
 *     (the optional clock probe, the optional step cursor of the device-resident loop) target a caller-owned buffer.
 *   - all pointers are DEVICE pointers unless the name ends in _host; the caller (PyTorch) owns
 *     every buffer, including the workspace (query sizes with the *_bytes functions).
 *   - layouts are row-major contiguous, residue-major.  Quaternions are scalar-first (w,x,y,z);
 *     tensor_7 = quat(4) | translation in Angstrom (3)   (openfold/utils/rigid_utils.py:1200-1230).
 *   - "f32"/"f64" in a parameter comment is the element type of the buffer.
 *   - the Python binding is derived from this file (framedipt_amd/_header.py), which reads one declaration style and refuses the rest:
 *     `[const] type* name` with the star at the type and one name per pointer, a name on every parameter, FDIPT_* macros that are plain
 *     integers; a scalar pointer parameter into HOST memory ends in _host and is bound with its pointee type, every other pointer as void*.
 */
#ifndef FDIPT_H
#define FDIPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FDIPT_OK 0
#define FDIPT_EINVAL (-1)   /* bad argument (null pointer, size out of range)            */
#define FDIPT_ELAUNCH (-2)  /* HIP launch error (hipGetLastError != hipSuccess)          */
#define FDIPT_ESIZE (-3)    /* workspace too small / N beyond the compiled LDS tiling     */

/* GEMM operand precision of the score network (accumulation is always fp32). */
#define FDIPT_PREC_F32 0  /* v_mfma_f32_32x32x2_f32: exact fp32, parity mode               */
#define FDIPT_PREC_BF16 1 /* v_mfma_f32_32x32x16_bf16: bf16 operands, pair rep kept in bf16.  Only in a library built
                             with -DFDIPT_HALF_BF16 (development comparison); the default build answers FDIPT_EINVAL */
#define FDIPT_PREC_F16 2  /* v_mfma_f32_32x32x16_f16: fp16 operands (11 significant bits, same MFMA rate as bf16), pair
                             rep kept in fp16; frames, points, softmax statistics, LayerNorm and scores stay fp32/fp64.
                             Throughput mode of the default build */
#define FDIPT_PREC_F16X 3 /* the fp16 mode plus split (hi + lo) weight terms where its own operand rounding costs most: the
                             EdgeTransition final layer and the edge embedder's layers 2 and 3 run W_lo h alongside W_hi h
                             (W_lo = W - fp16(W)).  Same parameters as FDIPT_PREC_F16, a different derived blob; pair rep in fp16.
                             Default build only (the -DFDIPT_HALF_BF16 library answers FDIPT_EINVAL).  Reference widths and N <= 1024
                             only; the forward and fdipt_edge_transition_fwd also need edge_transition4 (N % 4 == 0, N >= 8), while
                             fdipt_edge_embed_fwd takes any N.  FDIPT_EINVAL from the forward and the per-op entries otherwise,
                             and for every flag that swaps out a split kernel or the split operands: FDIPT_KF_ET3,
                             FDIPT_KF_GENERIC_PAIR, FDIPT_KF_GENERIC_ATTN, FDIPT_KF_UNFUSED_NODE, FDIPT_KF_STREAM_ATTN.  Accepted flags: FDIPT_KF_UNFOLDED, FDIPT_KF_NO_MERGE, FDIPT_KF_ROWS32,
                             FDIPT_KF_PASS_Z, FDIPT_KF_POINTS_LAUNCH */

/* FdiptDims.kernel_flags: run a fallback path of the half-precision mode at shapes where the default selection would not
 * (each of them is what some other shape uses anyway; parity tests run them at the golden sizes).  Same flags for
 * fdipt_model_prepare and every forward of a model. */
#define FDIPT_KF_ET3 1           /* EdgeTransition: the 16-pair-wave kernel (default for N % 4 != 0) for every N >= 43   */
#define FDIPT_KF_GENERIC_PAIR 2  /* EdgeTransition / edge embedder: the any-width LDS-chain kernels                      */
#define FDIPT_KF_GENERIC_ATTN 4  /* attention: the LDS-score kernels (the fallback for non-reference widths) in both modes */
#define FDIPT_KF_UNFUSED_NODE 8  /* node path as plain GEMM + LayerNorm launches (default for non-reference widths)     */
#define FDIPT_KF_UNFOLDED 16     /* launch folds off: pair bias / feature split / torsion head / fills as own launches  */
/* (bit 32 is retired and unassigned: FDIPT_EINVAL like any unknown bit) */
#define FDIPT_KF_NO_MERGE 64     /* IPA projections in the reference's formulation (k and v explicit) instead of the merged one
                                    (keys = values = the node rows, W_k folded into the query, W_v into the output projection)  */
#define FDIPT_KF_ROWS32 128      /* node path: the 32-row-block kernels (the default for N > 512) instead of the 16-row ones (tails, transition,
                                    node embedder, torsion head) for every N                                                  */
#define FDIPT_KF_PASS_Z 256      /* o_pair as its own pass over the 128 channels of z (round 5's path: sum_j a z, then down_z) instead of the
                                    pair_z image emitted by the producers of z (round 6); the last EdgeTransition then keeps its z' store */
#define FDIPT_KF_POINTS_LAUNCH 512 /* merged IPA projection: the rotated points and the node-row images by their own launch (points16_kernel)
                                    instead of the projection's epilogue                                                       */
#define FDIPT_KF_STREAM_ATTN 1024 /* half-precision mode: the IPA and sequence-transformer attentions on the key-streaming kernels (two sweeps
                                    over key chunks, LDS and registers independent of N) for every N, and the forward accepts N <= 2048
                                    instead of 1024.  No effect in the fp32 mode or with FDIPT_KF_GENERIC_ATTN (which takes precedence):
                                    there N > 1024 stays FDIPT_ESIZE.  N > 2048 is FDIPT_ESIZE with or without the flag          */
#define FDIPT_KF_ALL 2015

typedef void* fdipt_stream_t; /* hipStream_t */

/* ---------------------------------------------------------------- model description -------- */
/* Dimensions of ScoreNetwork (framedipt/model/score_network.py:200-216, config/base.yaml:55-79). */
typedef struct FdiptDims {
  int32_t c_s;         /* node_embed_size = ipa.c_s           (256) */
  int32_t c_z;         /* edge_embed_size = ipa.c_z           (128) */
  int32_t c_hidden;    /* ipa.c_hidden                         (256) */
  int32_t c_skip;      /* ipa.c_skip                           (64)  */
  int32_t no_heads;    /* ipa.no_heads                         (8)   */
  int32_t no_qk_points; /* ipa.no_qk_points                    (8)   */
  int32_t no_v_points; /* ipa.no_v_points                      (12)  */
  int32_t tfmr_heads;  /* ipa.seq_tfmr_num_heads               (4)   */
  int32_t tfmr_layers; /* ipa.seq_tfmr_num_layers              (2)   */
  int32_t num_blocks;  /* ipa.num_blocks                       (4)   */
  int32_t index_embed; /* embed.index_embed_size               (32)  */
  int32_t num_bins;    /* embed.num_bins                       (22); 0 = the model has no distogram channels (embed_self_conditioning
                          False, score_network.py:95-96): the edge embedder's first layer takes 2 d1 + index_embed inputs, and
                          min_bin / max_bin are ignored */
  int32_t use_aatype;  /* 1: node features carry a 21-way aatype one-hot (inpainting / input_aatype) */
  int32_t precision;   /* FDIPT_PREC_*                                                    */
  int32_t kernel_flags; /* FDIPT_KF_* bits; 0 = default kernel selection                  */
  float min_bin;       /* embed.min_bin (1e-5) */
  float max_bin;       /* embed.max_bin (20)   */
  float coordinate_scaling; /* ipa.coordinate_scaling = diffuser.r3.coordinate_scaling (0.1) */
  float r3_min_b;      /* diffuser.r3.min_b (0.1) */
  float r3_max_b;      /* diffuser.r3.max_b (20)  */
} FdiptDims;

/* Number of parameter tensors / total fp32 elements of the reference state_dict for `dims`
 * (same order as ScoreNetwork(...).state_dict(); framedipt_amd/weights.py:param_shapes). */
int fdipt_param_count(const FdiptDims* dims);
int64_t fdipt_param_offset(const FdiptDims* dims, int index); /* element offset of tensor `index` in the flat blob; index==count -> total */

/* Bytes of the derived-weights blob (operand-precision copies, fused / split matrices). */
size_t fdipt_derived_bytes(const FdiptDims* dims);
/* Build the derived blob from the flat fp32 state_dict blob (device, order above).  Once per model. */
int fdipt_model_prepare(const FdiptDims* dims, const float* params_f32, void* derived, fdipt_stream_t stream);

/* ---------------------------------------------------------------- per-batch sample setup ---- */
/* Constant-per-trajectory tables of a batch of B samples with N residues each:
 *   seq_idx [B,N] i32; idx_emb [B,N,index_embed] f32 = get_index_embedding(seq_idx) and
 *   rel_emb [B,n_rel,index_embed] f32 = get_index_embedding(r - rel_off), r in [0,n_rel) — both evaluated
 *   by the host exactly as the reference does in float32 (framedipt/model/score_network.py:17-38).
 * Produces in `setup` the relative-position part of the first edge-embedder layer
 * (score_network.py:98-105,184-187 restructured: concat-free first layer), [B,n_rel,c_z] f32, and behind it int32 [B]: the first
 * sample whose rows carry the same bits as sample b's (all zero when rel_emb is what is written above; the forward's row table reads
 * it, see fdipt_embed_table_leaders).  A `setup` is used with the B and n_rel it was made for and is not edited in place. */
size_t fdipt_setup_bytes(const FdiptDims* dims, int B, int N, int n_rel);
int fdipt_sample_setup(const FdiptDims* dims, const float* params_f32, const void* derived, int B, int N, int n_rel,
                       const float* rel_emb, void* setup, fdipt_stream_t stream);

/* ---------------------------------------------------------------- score network forward ---- */
/* Replaces ScoreNetwork.forward (framedipt/model/score_network.py:218-275) = Embedder.forward (:129-197)
 * + IpaScore.forward (framedipt/model/ipa_pytorch.py:509-572) + compute_backbone
 * (framedipt/protein/all_atom.py:147-176), for a batch of B equally sized samples. */
typedef struct FdiptForwardArgs {
  int32_t B, N, n_rel, rel_off;   /* rel index of pair (i,j) = seq_idx[i]-seq_idx[j]+rel_off          */
  const float* rigids_t;          /* [B,N,7] f32  input frames x_t                                     */
  const float* res_mask;          /* [B,N]   f32                                                      */
  const float* fixed_mask;        /* [B,N]   f32  1 = motif residue (not diffused)                    */
  const float* sc_ca_t;           /* [B,N,3] f32  self-conditioning CA positions (Angstrom); may be NULL exactly when
                                     dims->num_bins == 0 (nothing reads it then)                        */
  const int32_t* seq_idx;         /* [B,N]   i32                                                      */
  const float* idx_emb;           /* [B,N,index_embed] f32                                            */
  const int32_t* aatype;          /* [B,N] i32 pre-processed aatype (0..20) or NULL (de novo)         */
  const float* gt_psi;            /* [B,N,2] f32 torsion_angles_sin_cos[...,2,:]                      */
  const float* t;                 /* [B] f32 diffusion time                                           */
  const float* t_emb;             /* [B,index_embed] f32 get_timestep_embedding(t)   (host, float32)  */
  const float* t_emb_eps;         /* [index_embed]   f32 get_timestep_embedding(1e-5) (inpainting)    */
  const double* so3_sigma;        /* [B] f64 discrete_sigma[t_to_idx(t)] (so3_diffuser.py:398)        */
  const void* bb_tables;          /* residue tables for fdipt_backbone_atoms (needed iff atom37/atom14 != NULL) */
  /* outputs */
  float* psi;                     /* [B,N,2]  f32 */
  double* rot_score;              /* [B,N,3]  f64 */
  float* trans_score;             /* [B,N,3]  f32 */
  float* rigids;                  /* [B,N,7]  f32 predicted x_0 frames */
  float* atom37;                  /* [B,N,37,3] f32 or NULL */
  float* atom14;                  /* [B,N,14,3] f32 or NULL */
  /* optional traces for parity tests (NULL to skip): node / pair representation after each block */
  float* trace_node;              /* [num_blocks+1,B,N,c_s] f32: [0]=embedder output               */
  float* trace_edge;              /* [num_blocks,B,N,N,c_z] f32: [0]=embedder output, [b+1]=EdgeTransition b */
  /* optional, parity tests of the per-block sub-modules: [num_blocks,4,B,N,c_s+c_skip] f32 with slot 0 = IPA output
   * (ipa_pytorch.py:531, first c_s columns), 1 = post-IPA LayerNorm (:532, c_s), 2 = sequence-transformer output (:536-538,
   * c_s+c_skip), 3 = BackboneUpdate output (:542-545, 6).  Only the unfused node path keeps these tensors in memory: fp32
   * precision, or FDIPT_KF_UNFUSED_NODE | FDIPT_KF_UNFOLDED; FDIPT_EINVAL otherwise.  NULL to skip. */
  float* trace_inner;
  /* optional profiling: hipEvent_t pairs recorded on `stream` around every EdgeTransition launch
   * (num_blocks-1 pairs, created with fdipt_event_create); NULL to skip */
  void** ev_start;                /* host array of events */
  void** ev_stop;
  /* optional: contiguous copy of the predicted CA positions rigids[...,4:] ([B,N,3] f32, Angstrom), written at the end of
   * the forward.  May alias sc_ca_t (read at the start): the sampler's self-conditioning hand-over
   * (experiments/utils.py:361-366,571-578) then costs no copy.  NULL to skip. */
  float* ca_out;
  /* Concurrent sub-batches (one forward per HIP stream): the persistent pair kernels (edge embedder, EdgeTransition) start
   * on all CUs but `reserve_cus` of them, so that the latency-bound node-path launches of another stream keep finding free
   * CUs while they run.  0 = use every CU (single stream). */
  int32_t reserve_cus;
  /* optional: 1 = the edge embedder evaluates every pair (edge_embed2_kernel) where the default (0) evaluates the distinct
   * (class_i, class_j, rel, bin) rows once and spreads them (fdipt_embed_table_rows says where that is).  Same results; a switch for
   * parity tests, like FdiptDims.kernel_flags, kept per call because it touches no derived image.  (It sits in what was padding
   * behind reserve_cus: no other member moves.) */
  int32_t pair_embed;
  /* optional profiling: device buffer of 3 x uint64 (caller-owned, zeroed by the caller).  Thread 0 of every EdgeTransition
   * block adds its shader-clock cycles (s_memtime), its 100 MHz ticks (s_memrealtime) and 1 to [0], [1], [2]: the clock the
   * kernel's blocks actually ran at = [0] / [1] / 10 GHz (bench.py: roofline.clock_ghz).  NULL (the default): the kernels
   * execute no atomics and keep no state outside the caller's buffers. */
  unsigned long long* clock_out;
  /* optional: so3.use_cached_score = True (so3_diffuser.py:389-396) — the rotation-score norm is looked up instead of evaluated:
   * so3_score_table [B, so3_num_omega] f64 = the row of the reference's _score_norms table at each sample's t,
   * so3_omega_edges [so3_num_omega - 1] f64 = discrete_omega[:-1]; index = torch.bucketize(omega, edges).  NULL: the series. */
  const double* so3_score_table;
  const double* so3_omega_edges;
  int32_t so3_num_omega;
  /* optional: step cursor of a device-resident reverse loop (experiments/utils.py:584-602, the `for t in reverse_steps` loop).
   * NULL (the default): every pointer above is what its comment says.  Non-NULL: a device int32[2] = { step index k, ticket }, and
   * the per-step inputs / outputs are BASES of step-major arrays of which the kernels read / write row k = step_cursor[0]:
   *   rigids_t [T+1,B,N,7] (x_t of step k = row k: the rigid trajectory itself), t [T,B], t_emb [T,B,index_embed], so3_sigma [T,B],
   *   so3_score_table [T,B,so3_num_omega], atom37 [T,B,N,37,3] (rigid_0_traj).
   * The launch sequence then does not depend on k: a step (this forward + fdipt_se3_reverse_step_indexed, which advances the
   * cursor) can be captured once as a HIP graph and replayed for every step of every trajectory of the shape. */
  const int32_t* step_cursor;
  /* optional, with step_cursor only (kept-frame trajectories): frame_rows is a device int32[T] row map — step k writes its rigid_0_traj
   * frame to row frame_rows[k] of atom37 [n_kept,B,N,37,3], or builds no backbone atoms at all where frame_rows[k] == -1 (the decision is
   * uniform per launch, read from the map at the cursor: the launch sequence stays independent of k).  NULL: row k, as above. */
  const int32_t* frame_rows;
  /* optional, with step_cursor only: 1 = rigids_t is a two-row state ring [2,B,N,7] and x_t of step k is row k & 1 (the reverse step
   * writes x_{t-1} to row (k + 1) & 1: FdiptReverseIndexed.state_ring).  0: row k of the step-major [T+1,B,N,7], as above. */
  int32_t state_ring;
} FdiptForwardArgs;

size_t fdipt_forward_workspace_bytes(const FdiptDims* dims, int B, int N);
/* Rows per sample and class pair of the edge embedder's row table, n_rel * (num_bins + 1), where a whole forward of this shape and
 * n_rel (FdiptForwardArgs.n_rel) takes the table path when no pair trace is requested; 0 where it evaluates every pair: fp32, models
 * with aatype features or without a distogram, the kernel flags that swap out the pair kernels or their emissions, N % 4 != 0,
 * n_rel > 5 N / 2, rows > N * N / 2, or more than 64 MB of rows (352 B each) in the batch.  On that path fixed_mask and res_mask must
 * hold 0 or 1. */
int64_t fdipt_embed_table_rows(const FdiptDims* dims, int B, int N, int n_rel);
/* On the table path samples whose first-layer rows carry the same bits share one set of table rows: sample b reads the rows of its
 * leader, the first sample b' <= b that has every fixed-mask class b has and whose per-class first-layer rows (functions of t_emb[b]
 * and the class) and relative-position rows (`setup`, compared by fdipt_sample_setup) are bit-identical to b's; b itself where
 * there is none.  The forward decides this on the device from its own inputs (a batch stepped at one t has the single leader 0; per-sample t makes every sample lead).
 * Copies the int32 [B] leaders the last forward of this shape left in `workspace` to out_dev (device memory), after a device
 * synchronisation.  FDIPT_EINVAL where fdipt_embed_table_rows is 0. */
int fdipt_embed_table_leaders(const FdiptDims* dims, const void* workspace, int B, int N, int n_rel, int32_t* out_dev);
int fdipt_score_forward(const FdiptDims* dims, const float* params_f32, const void* derived, const void* setup,
                        const FdiptForwardArgs* args, void* workspace, size_t workspace_bytes, fdipt_stream_t stream);

/* ---------------------------------------------------------------- sub-modules of the forward ---- */
/* The forward's launch schedule cut at a sub-module boundary, on caller-provided inputs (callers that assemble their own
 * network, per-module parity tests).  Same model handles (dims / params / derived) and workspace as fdipt_score_forward;
 * "pair type" = float in FDIPT_PREC_F32, IEEE half in FDIPT_PREC_F16.  node [B,N,c_s] f32, z [B,N,N,c_z] pair type,
 * rigids [B,N,7] f32 tensor_7 in Angstrom (scaled by coordinate_scaling inside, ipa_pytorch.py:524), res_mask [B,N] f32. */
/* Embedder.forward (framedipt/model/score_network.py:129-197): node and pair embeddings, masked as score_network.py:236-237.
 * Reads B, N, n_rel, rel_off, res_mask, fixed_mask, sc_ca_t, seq_idx, idx_emb, aatype, t_emb, t_emb_eps of `args`. */
int fdipt_edge_embed_fwd(const FdiptDims* dims, const float* params_f32, const void* derived, const void* setup,
                         const FdiptForwardArgs* args, float* node_out, void* z_out, void* workspace, size_t workspace_bytes,
                         fdipt_stream_t stream);
/* Point projections of InvariantPointAttention `block` in the global frame (ipa_pytorch.py:213-239): q_pts, k_pts
 * [B,N,H,no_qk_points,3] and v_pts [B,N,H,no_v_points,3] f32, in scaled units (nm). */
int fdipt_ipa_project_points(const FdiptDims* dims, const float* params_f32, const void* derived, int block, int B, int N,
                             const float* node, const float* rigids, const float* res_mask, float* q_pts, float* k_pts,
                             float* v_pts, void* workspace, size_t workspace_bytes, fdipt_stream_t stream);
/* InvariantPointAttention.forward of `block` (ipa_pytorch.py:170-329: projections, logits with pair bias and point distances,
 * softmax, o / o_pt / o_pair, linear_out) times res_mask (:531): out [B,N,c_s] f32. */
int fdipt_ipa_attention_fwd(const FdiptDims* dims, const float* params_f32, const void* derived, int block, int B, int N,
                            const float* node, const void* z, const float* rigids, const float* res_mask, float* out,
                            void* workspace, size_t workspace_bytes, fdipt_stream_t stream);
/* EdgeTransition.forward of `block` < num_blocks - 1 (ipa_pytorch.py:84-102) times the pair mask (:549): z_out may alias z_in. */
int fdipt_edge_transition_fwd(const FdiptDims* dims, const float* params_f32, const void* derived, int block, int B, int N,
                              const float* node, const float* res_mask, const void* z_in, void* z_out, void* workspace,
                              size_t workspace_bytes, fdipt_stream_t stream);

/* ---------------------------------------------------------------- reverse step ------------- */
/* Replaces SE3Diffuser.reverse (framedipt/diffusion/se3_diffuser.py:346-401) with
 * _extract_trans_rots (:16-23), SO3Diffuser.reverse (so3_diffuser.py:569-602), compose_rotvec
 * (framedipt/data/transforms.py:33-46, SciPy Rotation conventions), R3Diffuser.reverse
 * (r3_diffuser.py:344-385), _assemble_rigid (:26-36) and Rigid.to_tensor_7 (rigid_utils.py:1200-1212),
 * fused, float64 internally.  z_rot/z_trans are N(0,1) draws (host noise tape; scaled by noise_scale here).
 * out_rot (optional) receives the float32 rotation matrices of x_{t-1} as the reference's Rigid holds them. */
int fdipt_se3_reverse_step(int B, int N, const float* rigids_t, const double* rot_score, const float* trans_score,
                           const float* diffuse_mask /* [B,N] f32 or NULL */, const double* z_rot, const double* z_trans,
                           double t, double dt, double noise_scale, int center, int diffuse_rot, int diffuse_trans,
                           double so3_min_sigma, double so3_max_sigma, double r3_min_b, double r3_max_b,
                           double coordinate_scaling, float* rigids_out /* [B,N,7] */, float* out_rot /* [B,N,3,3] or NULL */,
                           fdipt_stream_t stream);
/* The same step followed by all_atom.compute_backbone on x_{t-1} (experiments/utils.py:376-388: the atom37 frame of the
 * trajectory) in the same launch: psi [B,N,2], aatype [B,N] or NULL, tables as for fdipt_backbone_atoms, atom37 [B,N,37,3].
 * rigids_out must not alias rigids_t. */
int fdipt_se3_reverse_step_atoms(int B, int N, const float* rigids_t, const double* rot_score, const float* trans_score,
                                 const float* diffuse_mask, const double* z_rot, const double* z_trans, double t, double dt,
                                 double noise_scale, int center, int diffuse_rot, int diffuse_trans, double so3_min_sigma,
                                 double so3_max_sigma, double r3_min_b, double r3_max_b, double coordinate_scaling,
                                 float* rigids_out, float* out_rot, const float* psi, const int32_t* aatype,
                                 const void* tables, float* atom37, fdipt_stream_t stream);

/* ... and the step's row of trans_traj (experiments/utils.py:390-400) from the same launch:
 * trans_traj[b,i] = diffuse_mask * trans(pred_rigids) + traj_fixed_mask * trans(x_{t-1}); pred_rigids [B,N,7] = the forward's x_0
 * prediction, traj_fixed_mask [B,N] = fixed_mask * res_mask.  trans_traj == NULL: exactly fdipt_se3_reverse_step_atoms. */
int fdipt_se3_reverse_step_traj(int B, int N, const float* rigids_t, const double* rot_score, const float* trans_score,
                                const float* diffuse_mask, const double* z_rot, const double* z_trans, double t, double dt,
                                double noise_scale, int center, int diffuse_rot, int diffuse_trans, double so3_min_sigma,
                                double so3_max_sigma, double r3_min_b, double r3_max_b, double coordinate_scaling,
                                float* rigids_out, float* out_rot, const float* psi, const int32_t* aatype,
                                const void* tables, float* atom37, const float* pred_rigids, const float* traj_fixed_mask,
                                float* trans_traj, fdipt_stream_t stream);

/* The same fused step (reverse + backbone frame + trans_traj row) of a device-resident loop, addressed through a step cursor:
 * one step k = step_cursor[0] of the `for t in reverse_steps` loop (experiments/utils.py:584-602 -> one_step_inference :292-412).
 * Reads x_t = rigid_traj[k], writes x_{t-1} = rigid_traj[k+1], prot_traj[k], trans_traj[k]; uses z_rot[k], z_trans[k],
 * t = t_table[k]; the last block to finish sets step_cursor[0] = k + 1 (step_cursor[1] is its ticket, 0 between launches).  The
 * launch arguments do not depend on k, so a captured HIP graph of a step replays for every k. */
typedef struct FdiptReverseIndexed {
  int32_t B, N;
  float* rigid_traj;             /* [T+1,B,N,7] f32: row 0 = x_T */
  const double* rot_score;       /* [B,N,3] f64 (the forward's output buffer) */
  const float* trans_score;      /* [B,N,3] f32 */
  const float* diffuse_mask;     /* [B,N] f32 or NULL */
  const double* z_rot;           /* [T-1,B,N,3] f64 N(0,1) */
  const double* z_trans;         /* [T-1,B,N,3] f64 N(0,1) */
  const double* t_table;         /* [T] f64: reverse_steps (device) */
  double dt, noise_scale;
  int32_t center, diffuse_rot, diffuse_trans;
  double so3_min_sigma, so3_max_sigma, r3_min_b, r3_max_b, coordinate_scaling;
  const float* psi;              /* [B,N,2] f32 (forward output) */
  const int32_t* aatype;         /* [B,N] i32 or NULL */
  const void* bb_tables;
  float* prot_traj;              /* [T,B,N,37,3] f32 or NULL */
  const float* pred_rigids;      /* [B,N,7] f32 (forward output) */
  const float* traj_fixed_mask;  /* [B,N] f32 */
  float* trans_traj;             /* [T,B,N,3] f32 or NULL */
  int32_t* step_cursor;          /* device int32[2] */
  /* kept-frame trajectories (all three zero: the addressing above).  frame_rows: device int32[T], step k writes prot_traj / trans_traj /
   * kept_rigids at row frame_rows[k] of arrays with n_kept rows; -1 = the step keeps no frame: the kernel skips the backbone-frame
   * construction and the trans_traj row (uniform per launch).  NULL: row k. */
  const int32_t* frame_rows;
  /* 1 = rigid_traj is a two-row state ring [2,B,N,7]: reads x_t = row k & 1, writes x_{t-1} = row (k + 1) & 1.  0: rows k and k + 1. */
  int32_t state_ring;
  /* [n_kept,B,N,7] f32 or NULL: x_{t-1} of the kept steps (a copy of the state row, written on kept steps only) */
  float* kept_rigids;
} FdiptReverseIndexed;
int fdipt_se3_reverse_step_indexed(const FdiptReverseIndexed* args, fdipt_stream_t stream);
/* ---------------------------------------------------------------- device noise (opt-in) ---- */
/* The *_gen entries take the samples' 64-bit noise keys (noise_keys [B] u64, device) in place of the z_rot / z_trans rows and draw the
 * N(0,1) values inside the step kernel.  Generator (framedipt_amd/csrc/philox.hpp; restated in NumPy by tests/noise_ref.py):
 *   Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85, ten rounds)
 *   key     = (low word, high word) of the sample's noise key
 *   counter = (residue index i within the sample, step index k, purpose, call index j)
 *   purpose = 0 reverse-step rotation, 1 reverse-step translation, 2 forward-step rotation, 3 forward-step translation
 *   j = 0 gives components x, y; j = 1 gives z (its second normal is discarded)
 *   uniform = ((a >> 5) * 2^26 + (b >> 6) + 0.5) * 2^-53 in (0, 1): output words 0, 1 -> u0, words 2, 3 -> u1
 *   normal  = Box-Muller in float64: r = sqrt(-2 log u0), z0 = r cos(2 pi u1), z1 = r sin(2 pi u1)
 * CONTRACT: the value of a draw depends on (key, purpose, k, i, component) only.  Not on B, the sample's position in the batch, the
 * padded N, the grid, the precision mode, graph or eager execution, or the number of ranks.  A step computes exactly what the tape
 * entry computes on the rows fdipt_noise_fill writes for the same keys, bit for bit.
 *
 * out [n_steps,B,N,3] f64: the draws of steps k_begin .. k_begin + n_steps - 1 for one purpose, through the device function the step
 * kernels call. */
int fdipt_noise_fill(int B, int N, const uint64_t* noise_keys, int purpose, int k_begin, int n_steps, double* out,
                     fdipt_stream_t stream);
/* fdipt_se3_reverse_step_traj with the draws of step index `step` (purposes 0 and 1) in place of z_rot / z_trans. */
int fdipt_se3_reverse_step_traj_gen(int B, int N, const float* rigids_t, const double* rot_score, const float* trans_score,
                                    const float* diffuse_mask, const uint64_t* noise_keys, int step, double t, double dt,
                                    double noise_scale, int center, int diffuse_rot, int diffuse_trans, double so3_min_sigma,
                                    double so3_max_sigma, double r3_min_b, double r3_max_b, double coordinate_scaling,
                                    float* rigids_out, float* out_rot, const float* psi, const int32_t* aatype,
                                    const void* tables, float* atom37, const float* pred_rigids, const float* traj_fixed_mask,
                                    float* trans_traj, fdipt_stream_t stream);
/* fdipt_se3_reverse_step_indexed with args->z_rot == args->z_trans == NULL: the step index of the draws is step_cursor[0]. */
int fdipt_se3_reverse_step_indexed_gen(const FdiptReverseIndexed* args, const uint64_t* noise_keys, fdipt_stream_t stream);
/* compute_backbone of n = B*N frames (tensor_7) into row step_cursor[0] of atom37_rows [T,n,37,3] (rigid_0_traj rows built with the
 * caller's aatype view, experiments/utils.py:397-402). */
int fdipt_backbone_atoms_indexed(int n, const float* t7, const float* psi, const int32_t* aatype, const void* tables,
                                 float* atom37_rows, const int32_t* step_cursor, fdipt_stream_t s);

/* fdipt_backbone_atoms_indexed of a kept-frame loop: the frames go to row frame_rows[step_cursor[0]] of atom37_rows [n_kept,n,37,3]
 * (frame_rows: device int32[T], as in FdiptForwardArgs); a step whose row is -1 builds nothing. */
int fdipt_backbone_atoms_kept(int n, const float* t7, const float* psi, const int32_t* aatype, const void* tables,
                              float* atom37_rows, const int32_t* step_cursor, const int32_t* frame_rows, fdipt_stream_t s);

/* ---------------------------------------------------------------- EigenFold confidence score (f4) */
/* SE3Diffuser.forward: one-step forward noising q(x_t | x_{t-1}) (framedipt/diffusion/se3_diffuser.py:50-95; r3_diffuser.py:122-161
 * with center=False; so3_diffuser.py:408-443).  State = what the reference carries between steps: float32 rotation matrices
 * rot [B,N,3,3] and translations trans [B,N,3] in Angstrom; z_* are N(0,1) draws (float64); diffuse_mask [B,N] or NULL.
 * rigids_t (optional, [B,N,7]) receives Rigid.to_tensor_7 of the result (the next forward's input). */
int fdipt_se3_forward_step(int B, int N, const float* rot_t_1, const float* trans_t_1, const float* diffuse_mask, const double* z_rot,
                           const double* z_trans, double t_1, double dt, double noise_scale, double so3_min_sigma, double so3_max_sigma,
                           double r3_min_b, double r3_max_b, double coordinate_scaling, float* rot_t, float* trans_t, float* rigids_t,
                           fdipt_stream_t stream);
/* ... with the draws of step index `step` (purposes 2 and 3 of the device noise above) in place of z_rot / z_trans. */
int fdipt_se3_forward_step_gen(int B, int N, const float* rot_t_1, const float* trans_t_1, const float* diffuse_mask,
                               const uint64_t* noise_keys, int step, double t_1, double dt, double noise_scale, double so3_min_sigma,
                               double so3_max_sigma, double r3_min_b, double r3_max_b, double coordinate_scaling, float* rot_t,
                               float* trans_t, float* rigids_t, fdipt_stream_t stream);
/* SE3Diffuser.log_prob_backward / log_prob_forward (se3_diffuser.py:97-196; r3_diffuser.py:163-260; so3_diffuser.py:99-119,466-567;
 * r3_utils.py:10-42) of one step, summed over the diffused residues of each sample in float64:
 * out[b] = { log p_trans(x_{t-1}|x_t), log p_rot(x_{t-1}|x_t), log q_trans(x_t|x_{t-1}), log q_rot(x_t|x_{t-1}) }.
 * rot_score [B,N,3] float64 / trans_score [B,N,3] float32 are the model's scores at time t; both NULL: forward terms only. */
int fdipt_se3_step_log_prob(int B, int N, const float* rot_t, const float* trans_t, const float* rot_t_1, const float* trans_t_1,
                            const double* rot_score, const float* trans_score, const float* diffuse_mask, double t, double t_1, double dt,
                            double so3_min_sigma, double so3_max_sigma, double r3_min_b, double r3_max_b, double coordinate_scaling,
                            double* out, fdipt_stream_t stream);
/* Terminal term of logp_confidence_score (experiments/utils.py:846-866): out[b] = { sum log N(0,1)(scaled trans_T), log(1/pi^2) * n_diffused } */
int fdipt_se3_prior_log_prob(int B, int N, const float* trans_T, const float* diffuse_mask, double coordinate_scaling, double* out,
                             fdipt_stream_t stream);

/* ---------------------------------------------------------------- sample selection (opt-in) */
/* The five selected structures of evaluation/utils/sample_selection.py (get_selected_models :568-615) from the samples of a complex,
 * over the backbone atoms C, N, CA, O (BACKBONE_ATOMS order = atom37 columns 2, 0, 1, 4) of its diffused residues, in float64:
 * get_mean_coordinates (:163), get_median_coordinates (:216 -> weiszfeld_geometric_median :82), gaussian_density_estimation (:63) with
 * get_mode_index (:256), get_closest_index (:281) against the mean and the median.  One launch serves G groups (complexes) of the B
 * samples of atom37: group g = samples member[group_start[g] .. group_start[g + 1] - 1], S <= 64 of them, L = the number of rows with
 * diffuse_mask != 0 of its FIRST member (the caller makes sure that a group's members share the mask); S and L differ freely between
 * the groups of a launch.  One block per group; all max_iterations Weiszfeld iterations run inside the launch, as iterations on the
 * weights w of the iterate mu + sum_s w_s (x_s - mu) (mu = the mean, w = 1/S at the start): with the Gram matrix G of the centred
 * samples, d_s = sqrt(max(G_ss - 2 (G w)_s + w'G w, 0)) and w_s = (1 / d_s) / sum_r (1 / d_r).  Exactly max_iterations iterations, no
 * convergence test - as the reference - with one divergence: where the reference divides by a distance of exactly 0 (and returns NaN;
 * always for S = 1) the iteration stops, the median is that sample (w = e_s, lowest s) and FDIPT_SELECT_ZERO_DISTANCE is set. */
#define FDIPT_SELECT_MAX_SAMPLES 64
#define FDIPT_SELECT_ZERO_DISTANCE 1 /* status bit: the iteration met a distance of exactly 0 and returned that sample           */
#define FDIPT_SELECT_SKIPPED 2       /* status bit: the device data contradict the host counts (S, L, a member index out of range):
                                        the group's other outputs were not written                                             */
typedef struct FdiptSelectArgs {
  int32_t B, N, G, L_max;            /* samples, residues per sample, groups, capacity of the coordinate outputs in residues        */
  const float* atom37;               /* [B,N,37,3] f32                                                                              */
  const float* diffuse_mask;         /* [B,N] f32                                                                                   */
  const int32_t* group_start;        /* [G+1] i32, ascending from 0                                                                 */
  const int32_t* member;             /* [group_start[G]] i32 sample indices, group after group                                      */
  const int32_t* group_start_host;   /* HOST copy of group_start: the entry validates the group sizes with it                       */
  const int32_t* n_diffused_host;    /* HOST [G] i32: L of every group, 1 <= L <= L_max (the kernel counts again from the mask)     */
  double sigma;                      /* std of the Gaussian kernel of the density (reference default 30.0)                          */
  int32_t max_iterations;            /* Weiszfeld iterations (reference default 10000)                                              */
  /* outputs; per-sample arrays are indexed like `member` (position group_start[g] + s) */
  double* mean;                      /* [G,L_max,4,3] f64, rows >= L untouched                                                      */
  double* median;                    /* [G,L_max,4,3] f64                                                                           */
  double* weights;                   /* [group_start[G]] f64: w of the median, sums to 1                                            */
  double* density;                   /* [group_start[G]] f64: sum_r exp(-|x_s - x_r|^2 / sigma^2)                                   */
  double* dist_to_mean;              /* [group_start[G]] f64: sum over atoms of |x_s,a - mean_a|                                    */
  double* dist_to_median;            /* [group_start[G]] f64                                                                        */
  int32_t* index;                    /* [G,3] i32: mode (argmax density), mean_closest, median_closest (argmin); lowest index on ties */
  int32_t* status;                   /* [G] i32: FDIPT_SELECT_* bits                                                                */
  int32_t* n_diffused;               /* [G] i32: L as the kernel counted it                                                         */
  void* workspace;
  size_t workspace_bytes;
} FdiptSelectArgs;
size_t fdipt_select_workspace_bytes(int G, int B, int L_max);
/* FDIPT_ESIZE: a group of more than FDIPT_SELECT_MAX_SAMPLES samples, workspace too small.  FDIPT_EINVAL: an empty group, L = 0 or
 * L > L_max, a null pointer, sigma <= 0, max_iterations < 0. */
int fdipt_sample_select(const FdiptSelectArgs* args, fdipt_stream_t stream);

/* ---------------------------------------------------------------- sample evaluation (opt-in) */
/* The numbers of the reference's evaluation tables for B samples against R ground-truth structures, in float64, in one launch:
 * (a) backbone deviation without superposition over atom37 columns 2, 0, 1, 4 (C, N, CA, O) of the diffused residues
 *     (evaluation/utils/metrics.py: residue_backbone_rmsd :146, chain_backbone_rmsd :71, backbone_rmsd :25);
 * (b) phi, psi, omega in degrees (calc_dihedrals :926 per chain over the rows of res_mask: phi = 0 at a chain's first residue, psi =
 *     omega = 0 at its last) of sample and ground truth, and angle_error_with_sign (:308) of (ground truth, sample);
 * (c) ca_ca_distance / ca_ca_clashes (framedipt/analysis/metrics.py:185-218) over the rows with any non-zero coordinate, bonds between
 *     consecutive kept rows whatever their chains, clashes = pairs at 0 < distance < 1.5, as a fraction of the pairs at distance > 0;
 * (d) the superposition of the CA atoms of the align_mask rows onto the ground truth by the best proper rotation (rigid_transform_3D,
 *     data/transforms.py:77; here Horn's quaternion eigenproblem): x -> rotation x + translation.
 * A chain is a run of consecutive rows with res_mask != 0 and one chain_idx.  A region is a maximal run of diffused rows (diffuse_mask
 * != 0 and res_mask != 0) of one chain; the host plans the table, the kernel checks it against the masks and skips a sample it does
 * not describe.  Angles are stored in the order phi, psi, omega.  N is bounded by what a launch can address. */
#define FDIPT_EVAL_NAN_DIHEDRAL 1         /* status bit: a dihedral of the sample or its ground truth is NaN (coincident atoms)     */
#define FDIPT_EVAL_DEGENERATE_ALIGNMENT 2 /* status bit: fewer than 3 aligned rows or a covariance whose best rotation is not unique
                                             (the two largest eigenvalues of Horn's matrix within 1e-9 of its size): finite outputs  */
#define FDIPT_EVAL_SKIPPED 4              /* status bit: the region table or ref_index contradicts the device data: only status and
                                             n_diffused were written                                                                 */
typedef struct FdiptEvalArgs {
  int32_t B, N, R, n_regions, max_regions; /* samples, residues, ground-truth rows, rows of region_rows, stride of region_bb_rmsd   */
  const float* atom37;               /* [B,N,37,3] f32                                                                              */
  const float* ref37;                /* [R,N,37,3] f32                                                                              */
  const int32_t* ref_index;          /* [B] i32: ground-truth row of each sample                                                    */
  const float* diffuse_mask;         /* [B,N] f32                                                                                   */
  const float* res_mask;             /* [B,N] f32                                                                                   */
  const float* align_mask;           /* [B,N] f32                                                                                   */
  const int32_t* chain_idx;          /* [B,N] i32                                                                                   */
  const int32_t* region_start;       /* [B+1] i32, ascending from 0: sample b owns regions region_start[b] .. region_start[b+1] - 1 */
  const int32_t* region_rows;        /* [n_regions,2] i32: first and last row of every region                                       */
  const int32_t* ref_index_host;     /* HOST copy of ref_index: the entry validates it                                              */
  const int32_t* region_start_host;  /* HOST copy of region_start                                                                   */
  /* outputs */
  double* res_bb_rmsd;               /* [B,N] f64: sqrt(mean over the 4 atoms of |d|^2) at diffused rows, 0 elsewhere               */
  double* region_bb_rmsd;            /* [B,max_regions] f64: sqrt(sum |d|^2 / atoms) per region, entries past a sample's own untouched */
  double* bb_rmsd;                   /* [B] f64: the same over all regions                                                          */
  double* dihedral;                  /* [B,3,N] f64: phi, psi, omega of the samples in degrees                                      */
  double* gt_dihedral;               /* [R,3,N] f64: of the ground truth, with the chains of the first sample that names the row    */
  double* angle_error;               /* [B,3,N] f64: signed error ground truth - sample (residue_signed_angle_error :1088)            */
  double* ca_ca_bond_dev;            /* [B] f64: mean |d - 3.80209737096| over consecutive kept CA; NaN without a bond              */
  double* ca_ca_valid_percent;       /* [B] f64: fraction of those d < 3.80209737096 + 0.1                                          */
  int32_t* num_ca_steric_clashes;    /* [B] i32                                                                                     */
  double* ca_steric_clash_percent;   /* [B] f64: clashes / pairs at distance > 0; NaN without such a pair                           */
  double* aligned_mean_dev;          /* [B] f64: MEAN of the per-atom distances after the superposition (calc_aligned_rmsd's number) */
  double* aligned_rmsd;              /* [B] f64: their root mean square                                                             */
  double* rotation;                  /* [B,3,3] f64                                                                                 */
  double* translation;               /* [B,3] f64                                                                                   */
  int32_t* reflection;               /* [B] i32: rigid_transform_3D's reflection_detected (det of the covariance < 0)               */
  int32_t* status;                   /* [B] i32: FDIPT_EVAL_* bits                                                                  */
  int32_t* n_diffused;               /* [B] i32: diffused rows as the kernel counted them                                           */
  void* workspace;
  size_t workspace_bytes;
} FdiptEvalArgs;
size_t fdipt_eval_workspace_bytes(int B, int N);
/* FDIPT_EINVAL: a null pointer, R = 0, a ref_index out of range, a region_start that does not ascend from 0 to n_regions or gives a
 * sample more than max_regions regions.  FDIPT_ESIZE: workspace too small. */
int fdipt_sample_evaluate(const FdiptEvalArgs* args, fdipt_stream_t stream);

/* ---------------------------------------------------------------- structural violations (opt-in) */
/* The structural-violation block of the reference's metric tables (framedipt/analysis/metrics.py:protein_metrics through
 * openfold/np/relax/amber_minimize.py:get_violation_metrics: openfold/utils/loss.py find_structural_violations :1105 and
 * compute_violation_metrics :1272, tolerance factor 12, overlap tolerance 1.5) for B samples, in float64, in two launches on one
 * stream.  Every residue is ALA, as create_full_prot makes it without aatype: five atoms per row, atom37 columns 0..4 = N, CA, C, CB,
 * O, and that is the order of every per-atom output here (the reference's atom14 order is N, CA, C, O, CB).
 * A row with res_mask = 0 does not exist: the terms are those of the reference on the sample with these rows removed (a bond joins a
 * row to the next existing one).  A row with res_mask != 0 and keep_mask = 0 exists with its five atoms at the origin, as
 * make_atom14_positions leaves an undiffused row: it clashes with its like and enters the bond and angle terms.
 * residue_index is used literally: a bond counts in the means and the masks where the difference of the indices is exactly 1; rows
 * i, j form a clash pair where residue_index[i] < residue_index[j], with C(i) - N(j) exempt where residue_index[i] + 1 ==
 * residue_index[j].  Sums run in a fixed order that depends on the sample's own existing rows only.  N is bounded by what a launch can
 * address. */
#define FDIPT_VIOLATION_CONSTANTS 61 /* doubles fdipt_violation_constants writes */
typedef struct FdiptViolationArgs {
  int32_t B, N, atoms;               /* samples, residues, atoms per row of prot: 37 or 5 (columns 0..4 are read)                   */
  const float* prot;                 /* [B,N,atoms,3] f32                                                                           */
  const float* res_mask;             /* [B,N] f32: the row exists                                                                   */
  const float* keep_mask;            /* [B,N] f32: the row keeps its coordinates (0: they are read as zero)                         */
  const int32_t* residue_index;      /* [B,N] i32                                                                                   */
  /* outputs: [B] */
  double* bonds_c_n_loss_mean;       /* between_residue_bond_loss :712: sum of the masked flat-bottom errors / (bonds + 1e-6)       */
  double* angles_ca_c_n_loss_mean;   /* its stddev is the C-N bond length's, as the reference has it                                */
  double* angles_c_n_ca_loss_mean;
  double* clashes_mean_loss;         /* between_residue_clash_loss :871: sum of the errors / (1e-6 + n_clash_pairs)                 */
  double* violations_extreme_ca_ca_distance; /* :1235; this and the next four: count / (1e-4 + rows or bonds) (masked_mean)         */
  double* violations_between_residue_bond;
  double* violations_between_residue_clash;
  double* violations_within_residue;
  double* violations_per_residue;
  double* radius_of_gyration;        /* root mean square distance of the atoms of the kept rows from their centroid; NaN without one */
  int32_t* num_residue_violations;   /* rows of total_per_residue_violations_mask                                                   */
  int64_t* n_clash_pairs;            /* atom pairs of the clash mask                                                                */
  /* outputs: [B,N], zero at rows that do not exist */
  double* connections_per_residue_loss_sum;
  uint8_t* connections_per_residue_violation_mask;
  uint8_t* total_per_residue_violations_mask;
  /* outputs: [B,N,5] */
  double* clashes_per_atom_loss_sum; /* every pair's error is credited to both of its atoms                                         */
  uint8_t* clashes_per_atom_clash_mask;
  double* within_per_atom_loss_sum;  /* within_residue_violations :1018: the 5 x 5 error matrix summed along both axes              */
  uint8_t* within_per_atom_violations;
  void* workspace;
  size_t workspace_bytes;
} FdiptViolationArgs;
size_t fdipt_sample_violations_workspace(int B, int N);
/* FDIPT_EINVAL: a null pointer, B or N < 1, atoms not 37 or 5.  FDIPT_ESIZE: workspace too small, more row tiles than a grid holds. */
int fdipt_sample_violations(const FdiptViolationArgs* args, fdipt_stream_t stream);
/* The constants of the kernel as it uses them: van der Waals radii of C, N, O; C-N length, its stddev and 12 stddev (float32 values, as
 * the reference forms them); cos CA-C-N and the stddev it is given; cos C-N-CA and its stddev; ca_ca; then the ALA lower and upper
 * within-residue bounds, 5 x 5 each in the order N, CA, C, CB, O.  Returns FDIPT_VIOLATION_CONSTANTS. */
int fdipt_violation_constants(double* out_host);

/* ---------------------------------------------------------------- secondary structure (opt-in) */
/* Kabsch & Sander's secondary structure in the simplified alphabet coil / helix / strand, the SHAPE_METRICS of the reference's metric
 * tables (framedipt/analysis/metrics.py:calc_mdtraj_metrics: md.compute_dssp(traj, simplified=True) of the written PDB), for B samples,
 * in float64, in one launch of a block per sample.  The contract is DESIGN.md section 7.6; no mdtraj was at hand to compare with.
 * A row exists where res_mask != 0 and each of N, CA, C, O (atom37 columns 0, 1, 2, 4) has a non-zero coordinate; the existing rows
 * are compacted in order and everything else speaks of the compacted rows.  A break lies before a row whose chain_idx differs from the
 * row before or whose N is more than 2.5 A from that row's C.  E(donor, acceptor) = -27.888 (1/|HO| - 1/|HC| + 1/|NC| - 1/|NO|), H one
 * Angstrom from N along the previous row's O -> C, rounded to three decimals (halves away from zero), not below -9.9; evaluated for CA
 * within 9 A, the donor no proline, the acceptor neither the donor nor the row before it.  A donor keeps its two lowest energies below
 * 0 (the lower index on a tie); a bond is a kept acceptor below -0.5.  Turns (n = 3, 4, 5), parallel and antiparallel bridges, ladders
 * and the bulge pass, then strand, alpha (overrides strand), 3-10 and pi helices in this order.  Every integer output depends on the
 * sample's own existing rows only: rows appended behind a sample and its batch mates change no bit.  N is bounded by what a launch can
 * address (the ladder list: 40 N < 2^31). */
#define FDIPT_DSSP_COIL 0
#define FDIPT_DSSP_HELIX 1             /* alpha, 3-10 or pi                                                                         */
#define FDIPT_DSSP_STRAND 2            /* a row of a ladder: bridges, ladders' interiors, bulge gaps                                */
#define FDIPT_DSSP_ABSENT 255          /* ss at a row that does not exist                                                           */
#define FDIPT_DSSP_BRIDGES_PER_ROW 8   /* bridges (i, .) of one row i under the two-slot limit: 2 donors x 2 slots x 2 acceptors    */
#define FDIPT_DSSP_BRIDGE_OVERFLOW 1   /* status: a row held more bridges than FDIPT_DSSP_BRIDGES_PER_ROW; the fractions are NaN    */
#define FDIPT_DSSP_LADDER_OVERFLOW 2   /* status: more ladders than FDIPT_DSSP_BRIDGES_PER_ROW x N; the fractions are NaN           */
typedef struct FdiptDsspArgs {
  int32_t B, N, atoms;               /* samples, residues, atoms per row of prot: 37 or 5 (columns 0, 1, 2, 4 are read)             */
  const float* prot;                 /* [B,N,atoms,3] f32                                                                           */
  const float* res_mask;             /* [B,N] f32                                                                                   */
  const int32_t* chain_idx;          /* [B,N] i32                                                                                   */
  const uint8_t* is_proline;         /* [B,N] u8: the row donates no hydrogen bond                                                  */
  uint8_t* ss;                       /* [B,N] u8: FDIPT_DSSP_COIL / HELIX / STRAND, FDIPT_DSSP_ABSENT at a row that does not exist  */
  /* outputs: [B] */
  double* helix_percent;             /* counts over n_rows; NaN where n_rows = 0 or status != 0                                     */
  double* strand_percent;
  double* coil_percent;
  double* non_coil_percent;          /* (helix + strand) / n_rows                                                                   */
  int32_t* n_rows;                   /* rows that exist                                                                             */
  int32_t* n_hbonds;                 /* (donor, acceptor) pairs that are bonds                                                      */
  int32_t* n_bridges;
  int32_t* n_ladders;                /* after the bulge pass                                                                        */
  int32_t* status;                   /* FDIPT_DSSP_*_OVERFLOW bits                                                                  */
  /* outputs: [B,N,2], the donor's two slots; -1 and 0 where a slot is empty or the row does not exist */
  int32_t* acceptor;                 /* row of the input                                                                            */
  double* acceptor_energy;           /* kcal/mol, rounded                                                                           */
  void* workspace;
  size_t workspace_bytes;
} FdiptDsspArgs;
size_t fdipt_sample_dssp_workspace(int B, int N);
/* FDIPT_EINVAL: a null pointer, B or N < 1, atoms not 37 or 5.  FDIPT_ESIZE: workspace too small, N beyond the ladder list's index. */
int fdipt_sample_dssp(const FdiptDsspArgs* args, fdipt_stream_t stream);

/* ---------------------------------------------------------------- solvent accessibility (opt-in) */
/* Shrake & Rupley's solvent-accessible surface area per atom and per residue and the relative value, the ASA / RSA block of the
 * reference's TCR metric table (evaluation/utils/metrics.py:get_sasa: Bio.PDB.SASA.ShrakeRupley().compute(model, level="R") over the
 * whole complex), for B samples, in float64 with contraction off, in three launches on one stream.  The contract is DESIGN.md section
 * 7.7; no Biopython was at hand to compare with.  Atom (b, r, a) exists where res_mask[b,r] != 0 and atom_mask[b,r,a] != 0; all existing
 * atoms of a sample form one set.  Point k of atom i is p = sphere[k] * R_i + c_i (R = atom_radius[a], probe included); it is buried when
 * another existing atom j of the sample has ((dx dx + dy dy) + dz dz) <= R_j R_j, d = p - c_j.  accessible = points not buried;
 * atom_sasa = accessible * (R_i R_i * (4 pi / n_points)); residue_sasa = its atoms' sum in ascending column order from 0.0;
 * rsa = residue_sasa / max_sasa.  Absent atoms and rows give 0 and 0.0.  Every output of a sample depends on that sample's existing
 * atoms only: rows padded behind it and its batch mates change no bit. */
typedef struct FdiptSasaArgs {
  int32_t B, N, atoms, n_points;     /* samples, residues, atoms per row of prot: 37 or 5; sphere points: 1 .. 1024                 */
  const float* prot;                 /* [B,N,atoms,3] f32                                                                           */
  const float* res_mask;             /* [B,N] f32                                                                                   */
  const uint8_t* atom_mask;          /* [B,N,atoms] u8                                                                              */
  const double* atom_radius;         /* [atoms] f64: radius per atom column, the probe radius already added                         */
  const double* sphere;              /* [n_points,3] f64: unit points (the caller's table; no sine or cosine on the device)         */
  const double* max_sasa;            /* [B,N] f64: the denominator of rsa (NaN gives NaN)                                           */
  /* outputs */
  int32_t* accessible;               /* [B,N,atoms] i32: points of the atom that no other atom buries                               */
  double* atom_sasa;                 /* [B,N,atoms] f64, square Angstrom                                                            */
  double* residue_sasa;              /* [B,N] f64                                                                                   */
  double* rsa;                       /* [B,N] f64                                                                                   */
  int32_t* n_atoms;                  /* [B] i32: atoms that exist                                                                   */
  void* workspace;
  size_t workspace_bytes;
} FdiptSasaArgs;
size_t fdipt_sample_sasa_workspace(int B, int N, int atoms);
/* FDIPT_EINVAL: a null pointer, B or N < 1, atoms not 37 or 5, n_points outside 1 .. 1024.  FDIPT_ESIZE: workspace too small, or more
 * work items than a grid holds (B > 65535, B x N x atoms >= 2^31). */
int fdipt_sample_sasa(const FdiptSasaArgs* args, fdipt_stream_t stream);

/* ---------------------------------------------------------------- TM-score (opt-in) */
/* The TM-score of a GIVEN residue correspondence (row i with row i), Zhang & Skolnick's TMscore search over seed superpositions, for P
 * pairs of structures, in float64 with contraction off, in one launch of a block per pair.  It is the quantity behind the reference's
 * tm_score keys (framedipt/analysis/metrics.py:protein_metrics, experiments/inference.py) where the alignment is the identity, and a
 * lower bound of tmtools.tm_align's score in the all-against-all matrix of evaluation/eval_denovo.py:hierarchy_diversity: TM-align's
 * alignment search is NOT built, and no tmtools was at hand to compare with.  The contract is DESIGN.md section 7.8.
 * x, y: the CA atoms of the rows where both structures' masks are set, in ascending row order, float32 widened; n their number;
 * L = norm_length of the pair where given and > 0, else n.  d0 = 1.24 cbrt(L - 15) - 1.8 for L > 21, else 0.5; d_search = min(max(d0,
 * 4.5), 8).  S(R, t) = sum over all n rows of d0^2 / (d0^2 + |R x_i + t - y_i|^2); tm = max S / L.  Fragment lengths n >> k, k = 0..4,
 * while the value exceeds 4, then 4 (n below 4: n); a seed is (length l, start s), every s in 0 .. n - l, numbered level-major,
 * start-minor.  Per seed: superpose the fragment (Horn, proper rotation), score all rows, select the rows with |d|^2 < cut^2 (cut =
 * d_search - 1 in the first pass, d_search + 1 later; + 0.5 while fewer than 3 rows are inside and n > 3, up to 10^4), stop where the
 * set equals the set just superposed or after 20 refinements, else superpose the set and score again.  The result is the first seed in
 * seed order that holds the largest score, with the transform at which it reached it.  Every output of a pair depends on that pair's
 * masked rows only: batch mates, rows appended behind a structure and the pair's place in the list change no bit. */
#define FDIPT_TM_MAX_ROWS 1024       /* N beyond: FDIPT_ESIZE (two traces and the seeds' selected sets live in LDS)                  */
#define FDIPT_TM_TOO_SHORT 1         /* status: n < 3, no search; tm = NaN                                                          */
#define FDIPT_TM_SKIPPED 2           /* status: a structure index of the pair is out of range; tm = NaN                             */
#define FDIPT_TM_NOT_FINITE 4        /* status: no seed scored (coordinates that are not finite); tm = NaN                          */
typedef struct FdiptTmArgs {
  int32_t S, N, atoms, ca;           /* structures, rows, atoms per row of prot: 37 or 5; the CA column (1 in both layouts)         */
  int32_t S_b, atoms_b;              /* of prot_b (ignored where prot_b is NULL)                                                    */
  int32_t P;                         /* pairs                                                                                       */
  const float* prot;                 /* [S,N,atoms,3] f32                                                                           */
  const float* mask;                 /* [S,N] f32                                                                                   */
  const float* prot_b;               /* [S_b,N,atoms_b,3] f32 or NULL: the second structure of a pair comes from here, else from prot */
  const float* mask_b;               /* [S_b,N] f32 (with prot_b)                                                                   */
  const int32_t* pairs;              /* [P,2] i32: (index into prot, index into prot_b or prot); x is the first, y the second       */
  const int32_t* norm_length;        /* [P] i32 or NULL: L of the pair where > 0                                                    */
  /* outputs: [P] */
  double* tm;                        /* f64: max S / L; NaN with a status bit                                                       */
  double* rotation;                  /* [P,3,3] f64: R x + t ~ y at the best seed's best pass; the identity with a status bit       */
  double* translation;               /* [P,3] f64                                                                                   */
  int32_t* n_aligned;                /* i32: n                                                                                      */
  double* d0;                        /* f64                                                                                         */
  int32_t* best_seed;                /* i32: the seed number of the result; -1 with a status bit                                    */
  int32_t* passes;                   /* i32: superpositions scored over all seeds of the pair (a diagnostic)                        */
  int32_t* status;                   /* i32: FDIPT_TM_* bits                                                                        */
  void* workspace;                   /* may be NULL: fdipt_sample_tm_score_workspace is 0 (the search lives in LDS and registers)   */
  size_t workspace_bytes;
} FdiptTmArgs;
size_t fdipt_sample_tm_score_workspace(int S, int N, int P);
/* FDIPT_EINVAL: a null pointer, S, N or P < 1, atoms not 37 or 5, ca outside 0 .. 4.  FDIPT_ESIZE: N > FDIPT_TM_MAX_ROWS. */
int fdipt_sample_tm_score(const FdiptTmArgs* args, fdipt_stream_t stream);

/* ---------------------------------------------------------------- TM-align search (opt-in) */
/* A sequence-independent structural alignment search for P pairs of CA traces, in float64 with contraction off, a block per pair: the
 * quantity evaluation/eval_denovo.py:hierarchy_diversity takes from tmtools.tm_align for its all-against-all matrix.  The contract is
 * DESIGN.md section 7.9; it is modelled on Zhang & Skolnick's TM-align (its search parameters, three of its initial alignments, its
 * heuristic dynamic-programming iteration, the d8 filter, final scores per chain length) and is this project's own: no tmtools and no
 * TM-align source was at hand, and NO parity with tm_align is claimed.
 * x: the CA atoms of the rows of the first structure whose mask is set, ascending, float32 widened, n1 rows; y likewise for the second
 * structure, n2 rows (the two are compacted separately; N_b may differ from N_a).  Ls = min(n1, n2); d0s = (Ls <= 19 ? 0.168 : 1.24
 * cbrt(Ls - 15) - 1.8) + 0.8; ds = min(max(d0s, 4.5), 8); d8 = 1.5 Ls^0.3 + 3.5.  Initial alignments: I1 the best gapless threading
 * by the fast score, I2 a dynamic programme on the secondary structure of the traces, I3 one on secondary structure plus distance
 * under the better of their two transforms.  Each is scored by the seed search of the TM-score block above (fragment starts 40 apart,
 * pairs beyond d8 not scored) and iterated: dynamic programme on d0s^2 / (d0s^2 + d^2) under the search's transform with gap penalty
 * -0.6 then 0, up to 30 times each, until the score settles.  The best alignment loses its pairs beyond d8 and is scored by the full
 * search (start step 1, no d8) once per normalisation length.  Every output of a pair depends on that pair's masked rows only.
 * inits = FDIPT_TMA_INITS_ALL (opt-in; the default mode keeps every bit) runs two more initial alignments behind I1 - I3 through the same
 * iteration: I4, the best of a grid of local superpositions of fragment pairs, each extended by a dynamic programme and ranked by the fast
 * score, and I5, the best gapless threading of the longest unbroken run of the trace whose run is shorter (section 7.9's addendum). */
#define FDIPT_TMA_MAX_ROWS 512       /* N_a or N_b beyond: FDIPT_ESIZE (the traces and the programme's directions live in LDS)       */
#define FDIPT_TMA_TOO_SHORT 1        /* status: n1 < 5 or n2 < 5, no search; tm = NaN                                               */
#define FDIPT_TMA_SKIPPED 2          /* status: a structure index of the pair is out of range; tm = NaN                             */
#define FDIPT_TMA_NOT_FINITE 4       /* status: a coordinate of a set row is not finite, no search; tm = NaN                        */
#define FDIPT_TMA_NO_ALIGNMENT 8     /* status: fewer than 3 pairs of the best alignment lie within d8; tm = NaN                    */
#define FDIPT_TMA_INITS_DEFAULT 0    /* inits: I1, I2, I3; init_tm and init_dp hold 3 entries per pair                              */
#define FDIPT_TMA_INITS_ALL 1        /* inits: I1 .. I5; init_tm and init_dp hold 5 entries per pair                                */
typedef struct FdiptTmAlignArgs {
  int32_t S, N_a, atoms, ca;         /* structures, rows, atoms per row of prot: 37 or 5; the CA column (1 in both layouts)         */
  int32_t S_b, N_b, atoms_b;         /* of prot_b (where prot_b is NULL: S_b and atoms_b ignored, N_b = N_a)                        */
  int32_t P;                         /* pairs                                                                                       */
  const float* prot;                 /* [S,N_a,atoms,3] f32                                                                         */
  const float* mask;                 /* [S,N_a] f32                                                                                 */
  const float* prot_b;               /* [S_b,N_b,atoms_b,3] f32 or NULL: the second structure of a pair comes from here, else from prot */
  const float* mask_b;               /* [S_b,N_b] f32 (with prot_b)                                                                 */
  const int32_t* pairs;              /* [P,2] i32: (index into prot, index into prot_b or prot); x is the first, y the second       */
  /* outputs: [P] */
  double* tm;                        /* f64: tm_b, what hierarchy_diversity takes; NaN with a status bit                            */
  double* tm_a;                      /* f64: the final search's S / n1 with d0(n1)                                                  */
  double* tm_b;                      /* f64: the final search's S / n2 with d0(n2)                                                  */
  double* rotation;                  /* [P,3,3] f64: R x + t ~ y of the tm_b search; the identity with a status bit                 */
  double* translation;               /* [P,3] f64                                                                                   */
  int32_t* alignment;                /* [P,N_b] i32: the row of the first structure aligned with each row of the second, or -1      */
  int32_t* n_aligned;                /* i32: aligned pairs (within d8)                                                              */
  double* rmsd;                      /* f64: of the aligned pairs under the returned transform                                      */
  double* d0_a;                      /* f64: d0(n1)                                                                                 */
  double* d0_b;                      /* f64: d0(n2)                                                                                 */
  double* init_tm;                   /* [P,3] f64 ([P,5] with FDIPT_TMA_INITS_ALL): S / Ls of each initial alignment before its     */
                                     /* iteration; -1 where it was skipped                                                          */
  int32_t* init_dp;                  /* [P,3] i32 ([P,5] with FDIPT_TMA_INITS_ALL): dynamic programmes of each one's iteration      */
  int32_t* best_init;                /* i32: the initial alignment whose iteration gave the result (0 .. 2, 0 .. 4 with             */
                                     /* FDIPT_TMA_INITS_ALL); -1 with a status bit before it                                        */
  int32_t* status;                   /* i32: FDIPT_TMA_* bits                                                                       */
  void* workspace;                   /* may be NULL: fdipt_sample_tm_align_workspace is 0 (the search lives in LDS and registers)   */
  size_t workspace_bytes;
  int32_t inits;                     /* FDIPT_TMA_INITS_DEFAULT or FDIPT_TMA_INITS_ALL (last: the fields before it keep their place) */
} FdiptTmAlignArgs;
size_t fdipt_sample_tm_align_workspace(int S, int N_a, int N_b, int P);
/* FDIPT_EINVAL: a null pointer, S, N_a, N_b or P < 1, atoms not 37 or 5, ca outside 0 .. 4, inits none of the two.  FDIPT_ESIZE: N_a
 * or N_b > FDIPT_TMA_MAX_ROWS. */
int fdipt_sample_tm_align(const FdiptTmAlignArgs* args, fdipt_stream_t stream);

/* ---------------------------------------------------------------- structure search (opt-in) */
/* The novelty of samples: for each of Q queries, the top_k entries of a packed, ragged set of D CA traces under the alignment search of
 * the block above (the pair is (query, entry): tm_q is its tm_a, tm_t its tm_b), exactly what that search gives for every pair - bit
 * for bit, csrc/tmalign_body.hpp is the one body.  The contract is DESIGN.md section 7.15.  No parity with foldseek is claimed.
 * The caller plans the work: plan_entries lists entry indices bucket by bucket, bucket b being plan_entries[bucket_start[b] ..
 * bucket_start[b + 1]) with every entry of at most bucket_cap[b] rows.  Per bucket, in the order given: one launch of a block per
 * (query, entry) whose LDS is sized for (N_q, bucket_cap[b]), writing the pair's scores into the [Q,D] arrays; then one launch that
 * folds the bucket into each query's running list of the top_k (ranked score descending, entry index ascending; a score that is NaN
 * or below min_score never enters) and sets the query's floor = max(min_score, the top_k-th ranked score held), min_score while fewer
 * are held.  With prune, a block whose bound - min(n1, n2) / n1 for FDIPT_SEARCH_RANK_QUERY, min(n1, n2) / n2 for ..._TARGET, a score
 * being a sum of min(n1, n2) terms of at most 1 - is STRICTLY below the floor leaves with FDIPT_SEARCH_PRUNED.  The floor changes
 * between launches only: a call is deterministic for a given plan.  An entry that no bucket lists keeps NaN scores; one of more than
 * FDIPT_TMA_MAX_ROWS rows is marked FDIPT_SEARCH_TOO_LONG.  With details the Q x top_k hits run once more with every output. */
#define FDIPT_SEARCH_MAX_K 64
#define FDIPT_SEARCH_PRUNED 16       /* pair status: not scored, its length bound lies strictly below the query's floor             */
#define FDIPT_SEARCH_TOO_LONG 32     /* pair status: the entry has more than FDIPT_TMA_MAX_ROWS rows; skipped                        */
#define FDIPT_SEARCH_RANK_QUERY 0    /* rank_by: tm_q, the score normalised by the query's rows                                      */
#define FDIPT_SEARCH_RANK_TARGET 1   /* rank_by: tm_t, the score normalised by the entry's rows                                      */
typedef struct FdiptSearchArgs {
  int32_t Q, N_q, atoms, ca;         /* queries, rows, atoms per row of prot: 37 or 5; the CA column (1 in both layouts)            */
  int32_t D;                         /* entries of the set                                                                          */
  int32_t top_k, rank_by, prune, details;
  int32_t n_buckets;                 /* launches of the score pass (0: nothing is scored)                                           */
  int32_t detail_cap;                /* details: rows of `alignment` per hit and the N_b of the detail launch; >= every listed entry */
  int64_t R;                         /* rows of db_ca                                                                               */
  double min_score;
  const float* prot;                 /* [Q,N_q,atoms,3] f32                                                                         */
  const float* mask;                 /* [Q,N_q] f32                                                                                 */
  const float* db_ca;                /* [R,3] f32: the CA atoms of all entries, packed                                              */
  const int64_t* db_offsets;         /* [D+1] i64, device: entry e is rows db_offsets[e] .. db_offsets[e + 1]                       */
  const int32_t* plan_entries;       /* [bucket_start[n_buckets]] i32, device                                                       */
  const int32_t* bucket_start;       /* [n_buckets + 1] i32, HOST memory, ascending from 0                                          */
  const int32_t* bucket_cap;         /* [n_buckets] i32, HOST memory, each 1 .. FDIPT_TMA_MAX_ROWS                                  */
  /* outputs per hit: [Q,top_k] */
  int32_t* hit;                      /* i32: entry index, -1 where fewer than top_k entries qualify                                 */
  double* tm_q;                      /* f64; NaN where hit is -1                                                                    */
  double* tm_t;
  int32_t* n_aligned;
  double* rmsd;
  int32_t* status;                   /* i32: FDIPT_TMA_* bits of the hit's pair; 0 where hit is -1                                  */
  /* outputs per query: [Q] */
  int32_t* n_scored;                 /* pairs a block scored or refused (D - n_pruned - n_skipped - entries no bucket lists)       */
  int32_t* n_pruned;
  int32_t* n_skipped;                /* entries beyond the row limit                                                                */
  double* pdb_tm;                    /* f64: the ranked score of hit 0; NaN without a hit                                           */
  /* outputs per pair: [Q,D] */
  double* scores_q;                  /* f64; NaN where not scored                                                                   */
  double* scores_t;
  int32_t* pair_n_aligned;
  double* pair_rmsd;
  int32_t* pair_status;              /* i32: FDIPT_TMA_* and FDIPT_SEARCH_* bits                                                    */
  /* outputs of the detail pass: [Q,top_k], NULL without details */
  double* detail_tm_q;               /* f64: the detail pass's own scores (equal to tm_q, tm_t bit for bit)                         */
  double* detail_tm_t;
  double* rotation;                  /* [Q,top_k,3,3] f64                                                                           */
  double* translation;               /* [Q,top_k,3] f64                                                                             */
  int32_t* alignment;                /* [Q,top_k,detail_cap] i32: the query row aligned with each entry row, or -1                  */
  int32_t* best_init;
  void* workspace;                   /* fdipt_structure_search_workspace bytes: the ranked scores of the lists, the floors, and the */
  size_t workspace_bytes;            /* detail pass's outputs nobody asked for                                                      */
} FdiptSearchArgs;
size_t fdipt_structure_search_workspace(int Q, int top_k, int details);
/* FDIPT_EINVAL: a null pointer, Q, N_q or D < 1, atoms not 37 or 5, ca outside 0 .. 4, top_k outside 1 .. FDIPT_SEARCH_MAX_K, a rank_by
 * that is none of the two, a plan that is not ascending or a cap outside 1 .. FDIPT_TMA_MAX_ROWS, details with detail_cap outside that
 * range.  FDIPT_ESIZE: N_q > FDIPT_TMA_MAX_ROWS, Q x D or Q x top_k x detail_cap >= 2^31, workspace too small. */
int fdipt_structure_search(const FdiptSearchArgs* args, fdipt_stream_t stream);
/* The same search with the initial alignments of every pair's search chosen, score and detail launches alike: inits is
 * FDIPT_TMA_INITS_DEFAULT (fdipt_structure_search itself) or FDIPT_TMA_INITS_ALL; anything else is FDIPT_EINVAL.  FdiptSearchArgs keeps
 * its layout: the mode is an argument of the entry, not a field.  The workspace of fdipt_structure_search_workspace serves both modes. */
int fdipt_structure_search_inits(const FdiptSearchArgs* args, int32_t inits, fdipt_stream_t stream);

/* ---------------------------------------------------------------- superposition-free accuracy (opt-in) */
/* lDDT (Mariani et al. 2013; openfold/utils/loss.py lddt :382, lddt_ca :438), dRMSD (compute_drmsd :1518) and backbone FAPE (compute_fape
 * :76 as backbone_loss :152 calls it: clamp 10, unit 10, eps 1e-4) of P ordered pairs (model structure a, reference structure b) in row
 * correspondence, float32 coordinates widened, all arithmetic float64 with contraction off, in two launches on one stream.  The
 * contract is DESIGN.md section 7.13.
 * A row exists where res_mask[a] != 0; a row that does not exist is skipped everywhere.  A score row (score_mask[a] != 0 and it exists)
 * has its scores reported and enters the pair's numbers; partners, points and frames are always all existing rows.  An atom takes part
 * where it exists in both structures: atom_mask != 0, or without a mask any non-zero coordinate.
 * Atom set (mode): CA = column 1 (column 0 of a CA trace, atoms = 1); BACKBONE = N, CA, C, O = columns 0, 1, 2, 4 of atom37 and of the
 * five-atom layout; ALL = the 37 columns of atom37.  A = 1, 4, 37 atoms per row.
 * lDDT: the atom pair (u, v) of rows (i, j) is scored where d_b = sqrt(1e-10 + |x_u - x_v|^2) of the reference < cutoff, both take part,
 * u != v, and i != j in the multi-atom sets unless same_residue (then it is the reference's lddt on the flattened atom list).  Per atom
 * u the integers c (scored pairs) and n_t (scored pairs with |d_b - d_a| < t; t = 0.5, 1, 2, 4); score = (1 / (1e-10 + c)) * (1e-10 +
 * 0.25 (n_0.5 + n_1 + n_2 + n_4)) per atom, per row (its atoms' integers summed) and per pair (the score rows' summed, int64).
 * dRMSD: over the CA atoms that take part of the score rows, n of them: sqrt(sum_{i != j} (d_a - d_b)^2 / (n (n - 1))), plain
 * distances, 0 for n <= 1 (compute_drmsd on these rows without its mask argument).
 * FAPE: frame i = from_3_points(C, CA, N, eps 1e-8) with the first and third column negated (data_transforms.atom37_to_frames, group
 * 0) of every existing row whose N, CA and C take part, for both structures; points = the CA atoms that take part of all existing
 * rows; e_ij = min(sqrt(|R_i^T (x_j - t_i) - G_i^T (y_j - u_i)|^2 + 1e-4), 10) / 10; fape = sum_i (sum_j e_ij / (1e-4 + n_frames)) /
 * (1e-4 + n_points); res_fape[i] = sum_j e_ij / (1e-4 + n_points); region_fape = the mean of res_fape over the score rows with a frame.
 * Every sum runs in a fixed order that depends on the pair's own rows only; no floating-point atomics. */
#define FDIPT_LDDT_CA 0
#define FDIPT_LDDT_BACKBONE 1
#define FDIPT_LDDT_ALL 2
#define FDIPT_LDDT_TILE 256          /* partner rows per LDS tile of the CA and BACKBONE sets                                       */
#define FDIPT_LDDT_TILE_ALL 64       /* ... of the ALL set                                                                          */
#define FDIPT_LDDT_NO_PARTNER 1      /* status: a score row has no scored pair (c = 0): its lDDT is the reference's eps / eps = 1   */
#define FDIPT_LDDT_NO_FRAME 2        /* status: no row has a frame (a CA trace among them): fape, res_fape, region_fape are 0       */
#define FDIPT_LDDT_SKIPPED 4         /* status: a structure index of the pair is out of range; every output of the pair is 0        */
typedef struct FdiptLddtArgs {
  int32_t S, N, atoms;               /* model structures, rows, atoms per row of prot: 37, 5 or 1 (a CA trace)                      */
  int32_t S_b, atoms_b;              /* of prot_b (ignored where prot_b is NULL)                                                    */
  int32_t P, mode, same_residue;     /* pairs; FDIPT_LDDT_CA / BACKBONE / ALL; 1: atom pairs inside a row are scored too            */
  double cutoff;                     /* inclusion radius on the reference's distances (15)                                          */
  const float* prot;                 /* [S,N,atoms,3] f32                                                                           */
  const float* prot_b;               /* [S_b,N,atoms_b,3] f32 or NULL: the reference structure of a pair comes from here, else from prot */
  const float* res_mask;             /* [S,N] f32                                                                                   */
  const float* score_mask;           /* [S,N] f32                                                                                   */
  const uint8_t* atom_mask_a;        /* [S,N,atoms] u8 or NULL                                                                      */
  const uint8_t* atom_mask_b;        /* [S_b,N,atoms_b] u8 ([S,N,atoms] without prot_b) or NULL                                     */
  const int32_t* pairs;              /* [P,2] i32: (model: index into prot, reference: index into prot_b or prot)                   */
  /* outputs */
  double* lddt;                      /* [P] f64                                                                                     */
  double* res_lddt;                  /* [P,N] f64; 0 at rows that are no score rows                                                 */
  int32_t* n_scored;                 /* [P,N] i32: c of the row                                                                     */
  int32_t* n_passed;                 /* [P,N,4] i32: n_0.5, n_1, n_2, n_4 of the row                                                */
  double* atom_lddt;                 /* [P,N,A] f64 or NULL: per atom of the score rows (an atom without a scored pair: eps / eps)  */
  double* drmsd;                     /* [P] f64                                                                                     */
  double* fape;                      /* [P] f64                                                                                     */
  double* res_fape;                  /* [P,N] f64; 0 where the row has no frame                                                     */
  double* region_fape;               /* [P] f64; 0 where no score row has a frame                                                   */
  int32_t* status;                   /* [P] i32: FDIPT_LDDT_* bits                                                                  */
  void* workspace;
  size_t workspace_bytes;
} FdiptLddtArgs;
size_t fdipt_sample_lddt_workspace(int P, int N);
/* FDIPT_EINVAL: a null pointer, S, N or P < 1, a layout or mode outside the above, ALL without atom37 in both structures, a cutoff that
 * is not positive.  FDIPT_ESIZE: workspace too small, more row tiles than a grid holds, N A A beyond an int32 row counter. */
int fdipt_sample_lddt(const FdiptLddtArgs* args, fdipt_stream_t stream);

/* ---------------------------------------------------------------- GDT-TS / GDT-HA (opt-in) */
/* The global distance test (openfold/utils/validation_metrics.py gdt, gdt_ts, gdt_ha) of P pairs (model, reference) in row
 * correspondence, in float64 with contraction off, in one launch of a block per pair.  The contract is DESIGN.md section 7.14.
 * x, y: the CA atoms of the rows where both structures' masks are set, in ascending row order, float32 widened; n their number;
 * L = norm_length of the pair where given and > 0, else n.  Cutoffs c = (0.5, 1, 2, 4, 8) Angstrom; under a transform T,
 * count_k(T) = #{i : |T x_i - y_i|^2 <= c_k^2}.  gdt_ts = (count_1 + count_2 + count_3 + count_4) / (4 L), gdt_ha = (count_0 + count_1 +
 * count_2 + count_3) / (4 L), the integers summed first, one division.
 * mode NONE: T the identity (the reference's gdt on the raw coordinates; n >= 1).  GLOBAL: the least-squares superposition of all n
 * rows (Horn, proper rotation), one T for every cutoff (superimpose, then gdt; n >= 3).  SEARCH (n >= 3): per cutoff the largest count
 * over every transform the search visits.  A work item is (refinement cutoff k, seed), numbered k * n_seeds + seed; the seeds are those
 * of the TM-score block above with every start.  A pass of an item: superpose the current set (first the seed's fragment), form the five
 * counts under the transform, select the rows with d^2 < cut^2, cut = c_k (+ 0.5 while fewer than 3 rows are inside and n > 3, up to
 * 10^4); the item ends where the set equals the set just superposed or after 21 passes.  Every pass offers its five counts; the winner
 * of cutoff j is the largest count_j, then the lowest item number, then the earliest pass.  Seed 0 starts from all rows: a searched count
 * is never below the GLOBAL one.  This search is the project's own; NO parity with the LGA program is claimed.
 * Every output of a pair depends on that pair's masked rows only. */
#define FDIPT_GDT_NONE 0
#define FDIPT_GDT_GLOBAL 1
#define FDIPT_GDT_SEARCH 2
#define FDIPT_GDT_CUTOFFS 5
#define FDIPT_GDT_TOO_SHORT 1        /* status: n < 1 (NONE) or n < 3; scores NaN                                                   */
#define FDIPT_GDT_SKIPPED 2          /* status: a structure index of the pair is out of range; scores NaN                           */
#define FDIPT_GDT_NOT_FINITE 4       /* status: a coordinate of a scored row is not finite, nothing is counted; scores NaN          */
typedef struct FdiptGdtArgs {
  int32_t S, N, atoms, ca;           /* structures, rows, atoms per row of prot: 37 or 5; the CA column (1 in both layouts)         */
  int32_t S_b, atoms_b;              /* of prot_b (ignored where prot_b is NULL)                                                    */
  int32_t P, mode;                   /* pairs; FDIPT_GDT_NONE / GLOBAL / SEARCH                                                     */
  const float* prot;                 /* [S,N,atoms,3] f32                                                                           */
  const float* mask;                 /* [S,N] f32                                                                                   */
  const float* prot_b;               /* [S_b,N,atoms_b,3] f32 or NULL: the second structure of a pair comes from here, else from prot */
  const float* mask_b;               /* [S_b,N] f32 (with prot_b)                                                                   */
  const int32_t* pairs;              /* [P,2] i32: (index into prot, index into prot_b or prot); x is the first, y the second       */
  const int32_t* norm_length;        /* [P] i32 or NULL: L of the pair where > 0                                                    */
  /* outputs: [P] */
  double* gdt_ts;                    /* f64; NaN with a status bit                                                                  */
  double* gdt_ha;                    /* f64; NaN with a status bit                                                                  */
  int32_t* counts;                   /* [P,5] i32: count_j under cutoff j's winning transform; 0 with a status bit                  */
  int32_t* n_scored;                 /* i32: n                                                                                      */
  double* rotation;                  /* [P,5,3,3] f64: R x + t ~ y per cutoff; the identity in NONE and with a status bit           */
  double* translation;               /* [P,5,3] f64                                                                                 */
  int32_t* best_item;                /* [P,5] i32: the winning item per cutoff; -1 outside SEARCH and with a status bit             */
  int32_t* best_pass;                /* [P,5] i32: its pass, from 0; -1 likewise                                                    */
  int32_t* passes;                   /* i32: superpositions over all items of the search (1 in GLOBAL, 0 in NONE)                   */
  int32_t* res_within;               /* [P,N] i32: bit j set where the row is scored and within c_j under cutoff j's transform      */
  int32_t* status;                   /* i32: FDIPT_GDT_* bits                                                                       */
  void* workspace;                   /* may be NULL: fdipt_sample_gdt_workspace is 0 (the search lives in LDS and registers)        */
  size_t workspace_bytes;
} FdiptGdtArgs;
size_t fdipt_sample_gdt_workspace(int S, int N, int P);
/* FDIPT_EINVAL: a null pointer, S, N or P < 1, atoms not 37 or 5, ca outside 0 .. 4, a mode outside the above.  FDIPT_ESIZE: N >
 * FDIPT_TM_MAX_ROWS. */
int fdipt_sample_gdt(const FdiptGdtArgs* args, fdipt_stream_t stream);

/* ---------------------------------------------------------------- accuracy through a row map (opt-in) */
/* The two accuracy entries above for structures whose rows do NOT correspond: a pair p is (model ia of prot [S,N_a,atoms,3], reference
 * ib of prot_b [S_b,N_b,atoms_b,3]) with a row map m = map[p,:], int32 [N_b]: m[j] is the model row that corresponds to reference row j,
 * or -1 - the layout of FdiptTmAlignArgs.alignment and of FdiptSearchArgs.alignment.  N_a and N_b are independent; every per-row output
 * has N_b rows: the reference owns the rows, as it owns the distances in lDDT.  The contract is DESIGN.md section 7.16.
 * In both entries args->N is N_b, args->prot_b is required, and what args says about the model ([S,N,...]: prot, res_mask, atom_mask_a,
 * mask) has N_a rows; FdiptLddtArgs.score_mask is not read.
 * Reference row j EXISTS where res_mask_b[ib,j] != 0 (GDT: mask_b[ib,j]).  It is COVERED where it exists, 0 <= m[j] < N_a and
 * res_mask[ia,m[j]] != 0 (GDT: mask[ia,m[j]]).  A model atom of a covered row is present by the rule of the un-mapped entry (atom_mask_a,
 * or any non-zero coordinate).  The map need not be monotone; it must be injective on its non-negative entries.
 * The gathered model G(p): row j is model row m[j] where covered, absent (no atom present) elsewhere.
 * lDDT, coverage FDIPT_MAP_IGNORE: an atom takes part where it exists in the reference and is present in G; every output is bit for bit
 * what fdipt_sample_lddt returns on G with absent atoms masked off, res_mask = the reference's existing rows and score_mask =
 * score_mask_b[ib].  FDIPT_MAP_PENALISE (OpenFold's lddt where only the true mask is known): the atom pair (u, v) is scored, and counted
 * in c, where both atoms exist IN THE REFERENCE and d_b < cutoff (and u != v, and the same-residue rule); it passes threshold t only if
 * both atoms are present in G and |d_b - d_a| < t.  An uncovered row therefore scores eps / (eps + c).  The integers equal those of
 * fdipt_sample_lddt on G with every absent atom placed at a far, distinct point and marked present: that construction is the test
 * oracle.  drmsd and the FAPE outputs are the same under both switches (coverage has no meaning for them).
 * GDT: x, y are the CA atoms of (model row m[j], reference row j) for ascending j over the covered rows; n their number; everything after
 * the load is fdipt_sample_gdt in its three modes, every output bit for bit that entry's on G; res_within is [P,N_b]; L = n without a
 * norm_length.  N_a and N_b are each limited to FDIPT_TM_MAX_ROWS.  A CA trace (atoms = 1, ca = 0) is accepted for either structure.
 * Status bits of the map, shared by both entries (outside the bits each entry uses itself): either zeroes the pair's outputs (lDDT) or
 * makes them NaN (GDT) exactly as that entry's SKIPPED does, and changes no bit of another pair.  n_covered and n_reference are 0 then. */
#define FDIPT_MAP_IGNORE 0
#define FDIPT_MAP_PENALISE 1
#define FDIPT_MAP_OUT_OF_RANGE 8     /* status: an entry of the pair's map is < -1 or >= N_a                                        */
#define FDIPT_MAP_DUPLICATE 16       /* status: two reference rows of the pair map to the same model row                            */
typedef struct FdiptRowMap {
  int32_t N_a, coverage;             /* rows of prot; FDIPT_MAP_IGNORE / FDIPT_MAP_PENALISE (lDDT, interface)                       */
  const int32_t* map;                /* [P,args->N] i32                                                                             */
  const float* res_mask_b;           /* [S_b,args->N] f32: the reference's existing rows (lDDT; GDT reads args->mask_b)             */
  const float* score_mask_b;         /* [S_b,args->N] f32: the score rows, in reference rows (lDDT)                                 */
  int32_t* n_covered;                /* [P] i32: covered rows                                                                       */
  int32_t* n_reference;              /* [P] i32: existing reference rows                                                            */
} FdiptRowMap;
/* fdipt_sample_lddt_workspace(P, N_b) plus the verdicts on the maps */
size_t fdipt_sample_lddt_mapped_workspace(int P, int N_b);
/* Three launches on one stream: the verdicts on the maps (and n_covered, n_reference), then fdipt_sample_lddt's two.  FDIPT_EINVAL: as
 * fdipt_sample_lddt, a null pointer in map, N_a < 1, a coverage outside the two, no prot_b.  FDIPT_ESIZE: as fdipt_sample_lddt. */
int fdipt_sample_lddt_mapped(const FdiptLddtArgs* args, const FdiptRowMap* row_map, fdipt_stream_t stream);
/* One launch.  FDIPT_EINVAL: as fdipt_sample_gdt (atoms 37, 5 or 1; ca below atoms), a null map, n_covered or n_reference, N_a < 1, no
 * prot_b.  FDIPT_ESIZE: N_a or N_b > FDIPT_TM_MAX_ROWS. */
int fdipt_sample_gdt_mapped(const FdiptGdtArgs* args, const FdiptRowMap* row_map, fdipt_stream_t stream);

/* ---------------------------------------------------------------- sequence alignment (opt-in) */
/* Global alignment with affine gaps (Gotoh, three states) of P pairs of sequences, a wave per pair: the correspondence
 * framedipt/protein/align.py:get_shared_residues_info takes from Bio.Align.PairwiseAligner (mode global, BLOSUM62, open -10, extend
 * -0.5), as a producer of the row map above.  The contract is DESIGN.md section 7.17.  Letters are aatype in restype order
 * ARNDCQEGHILKMFPSTWYV, 0 .. 19, and 20 = X.  All arithmetic is int32 in HALF units: table [21,21] holds twice the substitution score,
 * open_gap and extend_gap twice the penalties (<= 0); a gap of k positions costs open + (k - 1) extend, end gaps as inner gaps.  With i
 * over a (length la) and j over b (length lb), T the table, o and e the penalties:
 *   M[i,j] = max(M, X, Y)[i-1,j-1] + T[a_i,b_j]
 *   X[i,j] = max(M[i-1,j] + o, X[i-1,j] + e, Y[i-1,j] + o)      a_i against a gap
 *   Y[i,j] = max(M[i,j-1] + o, X[i,j-1] + o, Y[i,j-1] + e)      b_j against a gap
 * M[0,0] = 0, X[i,0] = o + (i - 1) e, Y[0,j] = o + (j - 1) e, every other state of row 0 and column 0 is unreachable.  score = max(M, X,
 * Y)[la,lb].  Tie rule: in each maximum the first of M, X, Y wins among equals; the path is the one those choices record, walked back
 * from [la,lb].  |table entries| and |penalties| are limited to 8192 half units: the int32 sums then cannot wrap.
 * Counts of the path: n_aligned (M steps), n_identical (M steps with a_i == b_j and neither X), n_gaps_a (Y steps: gap positions in a),
 * n_gaps_b (X steps), n_gap_runs (maximal runs of X steps and of Y steps; an X run next to a Y run counts twice).
 * traceback != 0: a direction byte per cell goes to a workspace slab of max_len_a x max_len_b bytes per persistent wave and one lane walks
 * the path back; alignment is written.  traceback == 0: no slab; the counts ride through the recurrence under the same tie rule, every
 * output but alignment (not touched, may be NULL) is the same number.  Waves take pairs w, w + W, ...; W follows from workspace_bytes and
 * no output depends on it. */
#define FDIPT_SEQ_MAX_ROWS 2048      /* max_len_a or max_len_b beyond: FDIPT_ESIZE                                                   */
#define FDIPT_SEQ_LETTERS 21
#define FDIPT_SEQ_MAX_HALF_UNITS 8192 /* |table entry|, |open_gap|, |extend_gap| beyond: FDIPT_EINVAL (penalties), the caller's check (table) */
#define FDIPT_SEQ_EMPTY 1            /* status: a length of 0; the outputs are zero and the map is -1                               */
#define FDIPT_SEQ_BAD_LETTER 2       /* status: a letter outside 0 .. 20 inside a length; scored as X                               */
#define FDIPT_SEQ_SKIPPED 4          /* status: a sequence index of the pair is out of range, or a device length is negative or beyond
                                        max_len / the padded width; the outputs are zero and the map is -1                          */
typedef struct FdiptSeqAlignArgs {
  int32_t S_a, N_a;                  /* sequences and padded width of seq_a                                                         */
  int32_t S_b, N_b;                  /* of seq_b (where seq_b is NULL: ignored, seq_a and len_a serve both sides)                   */
  int32_t P;                         /* pairs                                                                                       */
  int32_t max_len_a, max_len_b;      /* host-known: the largest length on each side; they size the LDS and the slabs                */
  int32_t open_gap, extend_gap;      /* half units, <= 0                                                                            */
  int32_t traceback;                 /* 0: score and counts only                                                                    */
  const int32_t* seq_a;              /* [S_a,N_a] i32: letters; beyond a sequence's length nothing is read                          */
  const int32_t* len_a;              /* [S_a] i32                                                                                   */
  const int32_t* seq_b;              /* [S_b,N_b] i32 or NULL                                                                       */
  const int32_t* len_b;              /* [S_b] i32 (with seq_b)                                                                      */
  const int32_t* pairs;              /* [P,2] i32: (index into seq_a, index into seq_b or seq_a)                                    */
  const int32_t* table;              /* [21,21] i32: twice the substitution score, row = letter of a                                */
  /* outputs: [P] i32 */
  int32_t* score;                    /* half units                                                                                  */
  int32_t* n_aligned;
  int32_t* n_identical;
  int32_t* n_gaps_a;
  int32_t* n_gaps_b;
  int32_t* n_gap_runs;
  int32_t* alignment;                /* [P,N_b] i32 (traceback): the row of a aligned with each row of b, or -1; monotone            */
  int32_t* status;                   /* FDIPT_SEQ_* bits                                                                            */
  void* workspace;                   /* traceback: the slabs; else may be NULL                                                      */
  size_t workspace_bytes;
} FdiptSeqAlignArgs;
/* traceback: W slabs of max_len_a x max_len_b bytes, W = the launch's persistent waves (at most P), lowered until the slabs fit
 * max_workspace_bytes, and at least one; else 0 */
size_t fdipt_seq_align_workspace_bytes(int P, int max_len_a, int max_len_b, int traceback, size_t max_workspace_bytes);
/* One launch.  FDIPT_EINVAL: a null pointer the mode reads or writes, S_a, N_a or P < 1 (S_b, N_b with seq_b), a max_len < 0 or beyond
 * its padded width, a penalty > 0 or < -FDIPT_SEQ_MAX_HALF_UNITS.  FDIPT_ESIZE: a max_len > FDIPT_SEQ_MAX_ROWS, traceback with a
 * workspace below one slab. */
int fdipt_seq_align(const FdiptSeqAlignArgs* args, fdipt_stream_t stream);

/* ---------------------------------------------------------------- sequence alignment: modes (opt-in) */
/* The alignment above with a mode: global, semi-global (chosen end gaps free) or local (Smith-Waterman with the same three states).
 * Units, table, penalties, states and the tie rule inside a cell are those above; the contract is DESIGN.md section 7.20.  A path is
 * a sequence of M / X / Y steps, a run a maximal stretch of one state; X is a letter of a against a gap, Y a letter of b.
 * SEMIGLOBAL, free_ends a set of FDIPT_SEQ_FREE_* bits: the global score, except that the first run costs 0 if it is X with A_LEFT or Y
 * with B_LEFT and the last run costs 0 if it is X with A_RIGHT or Y with B_RIGHT (only the first and the last run can be free).  The
 * cells [i,0] are corners (M = 0, X and Y unreachable) with A_LEFT, the cells [0,j] with B_LEFT; the end cell is chosen among [la,lb],
 * every [i,lb] with i < la (A_RIGHT) and every [la,j] with j < lb (B_RIGHT), each over its three states: score descending, then i + j
 * descending, then i descending, then the first of M, X, Y.  The charged path runs from the end cell back to the first corner it
 * reaches, or to [0,0]; a leading gap that is not free is walked and counted.  free_ends = 0 is GLOBAL.
 * LOCAL: M[i,j] = T[a_i,b_j] + max(0, max(M, X, Y)[i-1,j-1]), the fresh start taken where that maximum is <= 0; X and Y as above; no
 * boundary scores.  The end cell is the inner cell with the largest M: score descending, then i + j ascending, then i ascending; the
 * path runs back to its fresh start.  No cell with M > 0: the empty result (zeros, a map of -1, a span of zeros).
 * The charged path aligns a[begin_a:end_a] with b[begin_b:end_b] globally; the counts are those of the charged path (n_gaps_b = end_a -
 * begin_a - n_aligned, n_gaps_a = end_b - begin_b - n_aligned), alignment is -1 outside the span.  status: the bits above (a length of 0
 * stays FDIPT_SEQ_EMPTY alone), and FDIPT_SEQ_NO_ALIGNED on every other pair whose result has no aligned column, in every mode.
 * traceback == 0: the counts and the origin (12 + 12 bits per state) ride through the recurrence; every output but alignment is the
 * same number. */
#define FDIPT_SEQ_NO_ALIGNED 8       /* status: the result has no aligned column (an empty local result, free runs only, gaps only)  */
#define FDIPT_SEQ_MODE_GLOBAL 0
#define FDIPT_SEQ_MODE_SEMIGLOBAL 1
#define FDIPT_SEQ_MODE_LOCAL 2
#define FDIPT_SEQ_FREE_A_LEFT 1      /* free_ends: a leading run of letters of a against gaps costs nothing                           */
#define FDIPT_SEQ_FREE_A_RIGHT 2     /* a trailing run of letters of a                                                               */
#define FDIPT_SEQ_FREE_B_LEFT 4      /* a leading run of letters of b                                                                */
#define FDIPT_SEQ_FREE_B_RIGHT 8     /* a trailing run of letters of b                                                               */
typedef struct FdiptSeqAlignModeArgs {
  int32_t S_a, N_a;                  /* as FdiptSeqAlignArgs, field by field                                                        */
  int32_t S_b, N_b;
  int32_t P;
  int32_t max_len_a, max_len_b;
  int32_t open_gap, extend_gap;
  int32_t traceback;
  int32_t mode;                      /* FDIPT_SEQ_MODE_*                                                                            */
  int32_t free_ends;                 /* FDIPT_SEQ_FREE_* bits; 0 unless mode is FDIPT_SEQ_MODE_SEMIGLOBAL                           */
  const int32_t* seq_a;
  const int32_t* len_a;
  const int32_t* seq_b;
  const int32_t* len_b;
  const int32_t* pairs;
  const int32_t* table;
  /* outputs: [P] i32 */
  int32_t* score;
  int32_t* n_aligned;
  int32_t* n_identical;
  int32_t* n_gaps_a;                 /* charged Y steps                                                                             */
  int32_t* n_gaps_b;                 /* charged X steps                                                                             */
  int32_t* n_gap_runs;               /* charged runs                                                                                */
  int32_t* begin_a;                  /* the origin [begin_a, begin_b] and the end cell [end_a, end_b] of the charged path           */
  int32_t* end_a;
  int32_t* begin_b;
  int32_t* end_b;
  int32_t* alignment;                /* [P,N_b] i32 (traceback)                                                                     */
  int32_t* status;
  void* workspace;
  size_t workspace_bytes;
} FdiptSeqAlignModeArgs;
/* the slab rule of fdipt_seq_align_workspace_bytes */
size_t fdipt_seq_align_modes_workspace_bytes(int P, int max_len_a, int max_len_b, int traceback, size_t max_workspace_bytes);
/* One launch.  FDIPT_EINVAL: what fdipt_seq_align refuses, a null span output, an unknown mode, free_ends outside 0 .. 15, free_ends
 * != 0 with another mode than FDIPT_SEQ_MODE_SEMIGLOBAL.  FDIPT_ESIZE: as fdipt_seq_align. */
int fdipt_seq_align_modes(const FdiptSeqAlignModeArgs* args, fdipt_stream_t stream);

/* ---------------------------------------------------------------- interface accuracy (opt-in) */
/* Contacts across an interface, fnat, fnonnat, interface RMSD, ligand RMSD and DockQ (Basu & Wallner 2016: the formula, not the
 * program) of P pairs (model structure a, reference structure b) in row correspondence, each on the I interfaces of the call; float32
 * coordinates widened, all arithmetic float64 with contraction off, three launches on one stream.  The contract is DESIGN.md section
 * 7.18.
 * A row takes part where res_mask of the model AND of the reference is set.  sides[k,i] says what row i is in interface k: 0 neither,
 * FDIPT_IFACE_RECEPTOR, FDIPT_IFACE_LIGAND (anything else counts as 0).  An atom takes part where it exists in BOTH structures:
 * atom_mask != 0, or without a mask any non-zero coordinate.
 * Atom set (mode): CA = column 1 (column 0 of a CA trace, atoms = 1); CB = column 3 where it takes part, else column 1; BACKBONE = N,
 * CA, C, CB, O = columns 0 .. 4 of atom37 and of the five-atom layout; ALL = the 37 columns of atom37.
 * Residue pair (i receptor, j ligand) is a contact of a structure where some pair of atoms that take part has (dx dx + dy dy) + dz dz
 * <= contact_cutoff^2 in it; n_native counts the reference's contacts, n_model the model's, n_shared those of both.  A row of either
 * side is an interface row where, in the reference, some such atom pair across the sides is within interface_cutoff.  fnat = n_shared
 * / n_native (0 for n_native = 0), fnonnat = (n_model - n_shared) / n_model (0 for n_model = 0).
 * RMSD atoms: N, CA, C, O = columns 0, 1, 2, 4 where both layouts have them and mode is not CA, else CA alone; an atom is used where
 * it exists in both structures.  irmsd: the RMSD atoms of the interface rows after their own least-squares superposition (Horn, proper
 * rotation).  lrmsd: the RMSD atoms of the ligand rows under the superposition of the RMSD atoms of the receptor rows.  Both transforms
 * are R x + t ~ y, x the model.  dockq = (fnat + 1 / (1 + (irmsd / 1.5)^2) + 1 / (1 + (lrmsd / 8.5)^2)) / 3.
 * The integers are exact and order-free (integer atomics); every floating-point sum runs in a fixed order that depends on the pair's
 * own rows only.  Pruning (default) skips a residue pair of a structure only where |CA_i - CA_j| - reach_i - reach_j exceeds the
 * cutoff that structure is tested against by a relative 1e-6, reach the largest distance from the row's CA to one of its atoms that
 * take part: no output bit depends on it. */
#define FDIPT_IFACE_CA 0
#define FDIPT_IFACE_CB 1
#define FDIPT_IFACE_BACKBONE 2
#define FDIPT_IFACE_ALL 3
#define FDIPT_IFACE_RECEPTOR 1       /* values of sides                                                                             */
#define FDIPT_IFACE_LIGAND 2
#define FDIPT_IFACE_MAX_ROWS 2048    /* N beyond: FDIPT_ESIZE                                                                       */
#define FDIPT_IFACE_MAX_INTERFACES 64 /* I beyond: FDIPT_ESIZE                                                                      */
#define FDIPT_IFACE_ROWS 64          /* receptor rows a block of the contact pass serves                                            */
#define FDIPT_IFACE_TILE 256         /* ligand rows per LDS tile of the CA, CB and BACKBONE sets                                    */
#define FDIPT_IFACE_TILE_ALL 64      /* ... of the ALL set                                                                          */
#define FDIPT_IFACE_NO_PRUNE 1       /* flags: every residue pair across the sides is evaluated                                     */
#define FDIPT_IFACE_NO_NATIVE_CONTACT 1 /* status: n_native = 0: fnat is 0, irmsd and dockq NaN                                     */
#define FDIPT_IFACE_TOO_FEW_ATOMS 2  /* status: a superposition has fewer than 3 atoms: its RMSD and dockq are NaN, its transform 0 */
#define FDIPT_IFACE_DEGENERATE 4     /* status: the eigenvalue gap of a superposition is within rounding (1e-9 of the matrix)       */
#define FDIPT_IFACE_EMPTY_SIDE 8     /* status: no row takes part on one of the sides                                               */
#define FDIPT_IFACE_NOT_FINITE 16    /* status: a sum over RMSD atoms is not finite: that RMSD and dockq are NaN                    */
#define FDIPT_IFACE_SKIPPED 32       /* status: a structure index of the pair is out of range: integers and fractions 0, RMSDs and  */
                                     /* dockq NaN, transforms 0                                                                     */
typedef struct FdiptInterfaceArgs {
  int32_t S, N, atoms;               /* model structures, rows, atoms per row of prot: 37, 5 or 1 (a CA trace)                      */
  int32_t S_b, atoms_b;              /* of prot_b (ignored where prot_b is NULL)                                                    */
  int32_t P, I, mode, flags;         /* pairs, interfaces, FDIPT_IFACE_CA / CB / BACKBONE / ALL, FDIPT_IFACE_NO_PRUNE or 0          */
  double contact_cutoff;             /* > 0                                                                                         */
  double interface_cutoff;           /* > 0                                                                                         */
  const float* prot;                 /* [S,N,atoms,3] f32                                                                           */
  const float* prot_b;               /* [S_b,N,atoms_b,3] f32 or NULL: the reference of a pair comes from here, else from prot      */
  const float* res_mask;             /* [S,N] f32                                                                                   */
  const float* res_mask_b;           /* [S_b,N] f32 (with prot_b; without it res_mask serves both)                                  */
  const uint8_t* atom_mask_a;        /* [S,N,atoms] u8 or NULL                                                                      */
  const uint8_t* atom_mask_b;        /* [S_b,N,atoms_b] u8 ([S,N,atoms] without prot_b) or NULL                                     */
  const int32_t* pairs;              /* [P,2] i32: (model: index into prot, reference: index into prot_b or prot)                   */
  const int32_t* sides;              /* [I,N] i32                                                                                   */
  /* outputs */
  int32_t* n_native;                 /* [P,I] i32                                                                                   */
  int32_t* n_model;                  /* [P,I] i32                                                                                   */
  int32_t* n_shared;                 /* [P,I] i32                                                                                   */
  int32_t* n_interface_rows;         /* [P,I] i32                                                                                   */
  int32_t* res_native;               /* [P,I,N] i32: the reference's contacts the row is part of                                    */
  int32_t* res_model;                /* [P,I,N] i32                                                                                 */
  int32_t* res_shared;               /* [P,I,N] i32                                                                                 */
  int32_t* interface_rows;           /* [P,I,N] i32: 1 = an interface row                                                           */
  double* fnat;                      /* [P,I] f64                                                                                   */
  double* fnonnat;                   /* [P,I] f64                                                                                   */
  double* irmsd;                     /* [P,I] f64                                                                                   */
  double* lrmsd;                     /* [P,I] f64                                                                                   */
  double* dockq;                     /* [P,I] f64                                                                                   */
  double* interface_rotation;        /* [P,I,3,3] f64: the superposition of irmsd                                                   */
  double* interface_translation;     /* [P,I,3] f64                                                                                 */
  double* receptor_rotation;         /* [P,I,3,3] f64: the superposition of lrmsd                                                   */
  double* receptor_translation;      /* [P,I,3] f64                                                                                 */
  int32_t* status;                   /* [P,I] i32: FDIPT_IFACE_* bits                                                               */
  void* workspace;
  size_t workspace_bytes;
  int32_t* n_interface_covered;      /* [P,I] i32: fdipt_sample_interface_mapped only (below); fdipt_sample_interface does not read it */
} FdiptInterfaceArgs;
/* per pair and row: the atoms that take part, and the row's reach in both structures */
size_t fdipt_sample_interface_workspace(int P, int N);
/* FDIPT_EINVAL: a null pointer, S, N, P or I < 1, a layout or mode outside the above, ALL without atom37 in both structures, CB or
 * BACKBONE with a CA trace, a cutoff that is not positive, unknown flags.  FDIPT_ESIZE: N > FDIPT_IFACE_MAX_ROWS, I >
 * FDIPT_IFACE_MAX_INTERFACES, workspace too small, more blocks than a grid holds.  All before any launch. */
int fdipt_sample_interface(const FdiptInterfaceArgs* args, fdipt_stream_t stream);

/* ---------------------------------------------------------------- interface accuracy through a row map (opt-in) */
/* The entry above for a model whose rows do NOT correspond to the reference's: pair p is (model ia of prot [S,N_a,atoms,3], reference ib
 * of prot_b [S_b,N_b,atoms_b,3]) with the row map m = row_map->map[p,:] of "accuracy through a row map" above (m[j]: the model row of
 * reference row j, or -1; it need not be monotone - the model may store its chains in another order - and must be injective on its
 * entries >= 0).  The contract is DESIGN.md section 7.19.  As with the DockQ program's alignment step, no parity with that program is
 * claimed: the contract is this project's own.
 * args->N is N_b; args->prot_b is required; what args says about the model (prot, res_mask, atom_mask_a) has row_map->N_a rows; sides is
 * [I,N_b] - the reference owns the rows and the sides - and every per-row output is [P,I,N_b].  N_a and N_b are independent, each at
 * most FDIPT_IFACE_MAX_ROWS.  The reference's existing rows are read from args->res_mask_b ([S_b,N_b], required);
 * row_map->res_mask_b and row_map->score_mask_b are NOT read.
 * Reference row j EXISTS where res_mask_b[ib,j] != 0.  It is COVERED where it exists, 0 <= m[j] < N_a and res_mask[ia,m[j]] != 0.
 * The gathered model G(p): row j is model row m[j] where covered and is masked off by res_mask elsewhere.
 * Coverage FDIPT_MAP_IGNORE: a row takes part where it is covered, an atom where it exists in the reference row and in model row m[j];
 * every output is bit for bit fdipt_sample_interface's on G, and n_interface_covered = n_interface_rows.
 * Coverage FDIPT_MAP_PENALISE (a docking score when residues are missing): a row takes part where it EXISTS.  What is evaluated in the
 * reference alone - the native contacts, res_native, interface_rows, n_interface_rows - runs over every existing row: an uncovered row
 * with the atoms of the set that exist in the reference (CB set: CB where the reference has it, else CA), a covered row with the atoms
 * both structures have.  A contact of the model, and so a shared one, needs both rows covered: an uncovered row costs fnat every native
 * contact it is part of.  irmsd runs over the RMSD atoms of the interface rows that are covered - n_interface_covered [P,I] counts
 * them - and lrmsd over the covered ligand rows under the superposition of the covered receptor rows, both in ascending reference rows
 * (fd_block_sum's order).  dockq, fnonnat and the status bits follow the un-mapped rules on these numbers; FDIPT_IFACE_EMPTY_SIDE looks
 * at the rows that take part.  The counts equal fdipt_sample_interface's on G with every uncovered existing row given the reference row's
 * atom pattern at a far, distinct point (beyond both cutoffs from every atom and from each other, marked present): the test oracle.
 * Verdict on the pair's map: FDIPT_MAP_OUT_OF_RANGE and FDIPT_MAP_DUPLICATE (8, 16) are FDIPT_IFACE_EMPTY_SIDE and
 * FDIPT_IFACE_NOT_FINITE in this entry's status word, so the entry reports them under two values of its own (64, 128: defined behind the prototypes).  Either treats the
 * pair's outputs on every interface as FDIPT_IFACE_SKIPPED does (n_interface_covered 0) with n_covered = n_reference = 0, and changes
 * no bit of another pair; an entry of the map is range-checked at every read whatever the verdict was. */
/* fdipt_sample_interface_workspace(P, N_b) plus the model row of every reference row and the verdicts on the maps */
size_t fdipt_sample_interface_mapped_workspace(int P, int N_b);
/* Four launches on one stream: the verdicts on the maps (with n_covered, n_reference), then fdipt_sample_interface's three reading the
 * model through the map.  FDIPT_EINVAL: as fdipt_sample_interface, a null row_map, map, n_covered, n_reference, n_interface_covered or
 * args->res_mask_b, N_a < 1, a coverage outside the two, no prot_b.  FDIPT_ESIZE: as fdipt_sample_interface, N_a >
 * FDIPT_IFACE_MAX_ROWS.  All before any launch. */
int fdipt_sample_interface_mapped(const FdiptInterfaceArgs* args, const FdiptRowMap* row_map, fdipt_stream_t stream);
#define FDIPT_IFACE_MAP_OUT_OF_RANGE 64 /* status: an entry of the pair's map is < -1 or >= N_a (FDIPT_MAP_OUT_OF_RANGE of this entry) */
#define FDIPT_IFACE_MAP_DUPLICATE 128   /* status: two reference rows of the pair map to the same model row                           */

/* ---------------------------------------------------------------- inverse folding (opt-in) */
/* The vanilla full-backbone ProteinMPNN (ProteinMPNN/protein_mpnn_utils.py: ProteinFeatures, EncLayer, DecLayer, ProteinMPNN.forward
 * and .sample), inference only, float32 throughout; the contract is DESIGN.md section 7.10.  Letters are in the MODEL's alphabet
 * ACDEFGHIKLMNPQRSTVWYX (0 .. 20).  Two entries share the features and the encoder: fdipt_mpnn_score gives the teacher-forced
 * log-probabilities of forward(..., use_input_decoding_order=True) for M (sequence, decoding order) pairs per backbone,
 * fdipt_mpnn_design runs the autoregressive loop of sample for M sequences per backbone from caller-supplied uniforms.
 *
 * The weight image is ONE float32 array, every matrix stored TRANSPOSED ([in][out], so that a wave reads consecutive outputs), in this
 * order (reference parameter name -> floats); fdipt_mpnn_weights_floats is its length, 1 660 485 for every K:
 *   features.embeddings.linear.weight^T [66][16], .bias [16]
 *   features.edge_embedding.weight^T [416][128]; features.norm_edges.weight [128], .bias [128]
 *   W_e.weight^T [128][128], W_e.bias [128]; W_s.weight [21][128] (as stored: a row per letter)
 *   encoder_layers.l, l = 0 .. 2:  W1^T [384][128], b [128]; W2^T [128][128], b; W3^T [128][128], b; norm1 weight, bias [128];
 *       dense.W_in^T [128][512], b [512]; dense.W_out^T [512][128], b [128]; norm2 weight, bias;
 *       W11^T [384][128], b; W12^T [128][128], b; W13^T [128][128], b; norm3 weight, bias
 *   decoder_layers.l, l = 0 .. 2:  W1^T [512][128], b; W2^T, b; W3^T, b; norm1; dense.W_in^T, b; dense.W_out^T, b; norm2
 *   W_out.weight^T [128][21], W_out.bias [21]
 *
 * FdiptMpnnDims.ca_only = 1 is the CA-only model (CA_ProteinFeatures, ProteinMPNN(ca_only=True)): the same
 * model after features that read nothing but the CA trace.  The edge inputs are 167 columns (16 positional, 9 x 16 RBF over the
 * array-shifted traces, 7 orientation values), the image is the same table with features.edge_embedding.weight^T [167][128], so
 * fdipt_mpnn_weights_floats is 1 628 613 = 1 660 485 - 249 x 128; the five parameters the reference's forward never reads
 * (features.node_embedding, features.norm_nodes, W_v) are not in it.  prot may then also be the trace alone, atoms = 1: [B,N,3]; with
 * 37 or 5 atoms the kernel reads atom 1.  N < 3 is FDIPT_EINVAL (the reference raises there).  E_idx, the workspace and every other
 * argument are as for the vanilla model. */
#define FDIPT_MPNN_MAX_ROWS 2048     /* N beyond: FDIPT_ESIZE                                                                       */
#define FDIPT_MPNN_MAX_SEQ 64         /* M beyond: FDIPT_ESIZE                                                                       */
#define FDIPT_MPNN_MAX_NEIGHBORS 64   /* k_neighbors outside 1 .. 64: FDIPT_EINVAL                                                   */
#define FDIPT_MPNN_MASKED_NEIGHBOR 1  /* status: a row with res_mask set has a neighbour without; no parity with the reference there */
#define FDIPT_MPNN_NO_LETTER 2        /* status (design): the controls of a row left no letter with p > 0; it keeps its input letter  */
typedef struct FdiptMpnnDims {
  int32_t hidden, enc_layers, dec_layers, vocab; /* 128, 3, 3, 21: anything else is FDIPT_EINVAL                                    */
  int32_t k_neighbors;                /* K, the checkpoint's num_edges; a row takes K_eff = min(K, N) neighbours                     */
  int32_t ca_only;                    /* 0 = the vanilla model (a caller that never names it), 1 = the CA-only one; else FDIPT_EINVAL */
} FdiptMpnnDims;
/* floats of the weight image; FDIPT_EINVAL for dims the kernels are not built for */
int64_t fdipt_mpnn_weights_floats(const FdiptMpnnDims* dims);
typedef struct FdiptMpnnArgs {
  int32_t B, N, M, atoms;             /* backbones, rows, sequences per backbone, atoms per row of prot: 37 or 5 (N, CA, C, CB, O);  */
                                      /* with dims->ca_only also 1: the CA trace                                                     */
  const float* weights;               /* f32 [fdipt_mpnn_weights_floats]                                                             */
  const float* prot;                  /* [B,N,atoms,3] f32: N, CA, C at 0, 1, 2 and O at 4 in both layouts; CB is rebuilt            */
  const float* res_mask;              /* [B,N] f32                                                                                   */
  const float* chain_mask;            /* [B,N] f32: 1 = designed, 0 = fixed (design only; score ignores it)                          */
  const int32_t* residue_index;       /* [B,N] i32                                                                                   */
  const int32_t* chain_idx;           /* [B,N] i32                                                                                   */
  const int32_t* S;                   /* [B,M,N] i32: the sequence to score / the input letters fixed and masked rows keep           */
  const int32_t* decoding_order;      /* [B,M,N] i32: a permutation of 0 .. N-1 per sequence, first decoded row first                */
  const float* u;                     /* [B,M,N] f32 in [0,1), indexed by ROW (design only)                                          */
  const float* omit;                  /* [21] f32, 1 = never drawn (design only)                                                     */
  const float* bias;                  /* [21] f32 (design only)                                                                      */
  float temperature;                  /* > 0 (design only)                                                                           */
  /* outputs */
  int32_t* E_idx;                     /* [B,N,K_eff] i32: the neighbours of a row, nearest first, ties to the lower column           */
  float* log_probs;                   /* [B,M,N,21] f32 (score only); 0 in rows without res_mask                                     */
  int32_t* S_out;                     /* [B,M,N] i32 (design only)                                                                   */
  float* probs;                       /* [B,M,N,21] f32 (design only): chain_mask * res_mask * the row's sampling distribution       */
  int32_t* status;                    /* [B] i32: FDIPT_MPNN_* bits                                                                  */
  void* workspace;
  size_t workspace_bytes;
  /* optional inputs; NULL / 0 = absent, so a caller that zero-fills the struct and never names them gets the
   * entries as they were.  The per-row controls and the ties are read by fdipt_mpnn_design only, at the row being decoded (for a tied
   * group: at its LAST member, as tied_sample does). */
  const float* bias_by_res;           /* [B,N,21] f32: added to the logits as bias_by_res / temperature                              */
  const float* omit_mask;             /* [B,N,21] f32: p *= 1 - omit_mask, renormalised (the reference's omit_AA_mask)                */
  const float* pssm_coef;             /* [B,N] f32: needed by pssm_bias and pssm_log_odds_mask                                        */
  const float* pssm_bias;             /* [B,N,21] f32: p = (1 - pssm_multi coef) p + pssm_multi coef pssm_bias                        */
  const float* pssm_log_odds_mask;    /* [B,N,21] f32: p = p mask + 0.001 p, renormalised                                             */
  const int32_t* tie_group;           /* [B,N] i32: -1 = untied; consecutive steps of decoding_order whose rows carry the same id >= 0 */
                                      /* are ONE group: one letter from the weighted sum of the members' logits                      */
  const float* tied_beta;             /* [B,N] f32: a member's weight in its group's logits; needed by tie_group                      */
  float pssm_multi;                   /* the scalar of pssm_bias                                                                     */
  int32_t unconditional;              /* fdipt_mpnn_score only: != 0 = no neighbour counts as decoded (unconditional_probs); S and    */
                                      /* decoding_order are not read and may be NULL                                                 */
} FdiptMpnnArgs;
size_t fdipt_mpnn_workspace(const FdiptMpnnDims* dims, int B, int N, int M);
/* FDIPT_EINVAL: a null pointer the entry reads or writes, unsupported dims, B, N or M < 1, atoms not 37 or 5 (ca_only: or 1), N < 3
 * with ca_only, temperature <= 0
 * (design), pssm_bias or pssm_log_odds_mask without pssm_coef (design), tie_group without tied_beta (design).  FDIPT_ESIZE: N >
 * FDIPT_MPNN_MAX_ROWS, M > FDIPT_MPNN_MAX_SEQ, workspace too small.  All before any launch. */
int fdipt_mpnn_score(const FdiptMpnnDims* dims, const FdiptMpnnArgs* args, fdipt_stream_t stream);
int fdipt_mpnn_design(const FdiptMpnnDims* dims, const FdiptMpnnArgs* args, fdipt_stream_t stream);

/* ---------------------------------------------------------------- frame algebra (a8) ------- */
/* openfold/utils/rigid_utils.py free functions and Rigid/Rotation methods, n independent items, f32. */
int fdipt_quat_to_rot(int n, const float* quat, float* rot, fdipt_stream_t s);           /* :185 */
int fdipt_rot_to_quat(int n, const float* rot, float* quat, fdipt_stream_t s);           /* :208 (sign may differ) */
int fdipt_quat_multiply(int n, const float* q1, const float* q2, float* out, fdipt_stream_t s); /* :254 */
int fdipt_quat_multiply_by_vec(int n, const float* q, const float* v, float* out, fdipt_stream_t s); /* :266 */
int fdipt_invert_quat(int n, const float* q, float* out, fdipt_stream_t s);              /* :282 */
int fdipt_rigid_apply(int n, const float* t7, const float* pts, float* out, fdipt_stream_t s);        /* :1104 */
int fdipt_rigid_invert_apply(int n, const float* t7, const float* pts, float* out, fdipt_stream_t s); /* :1118 */
int fdipt_rigid_compose(int n, const float* a_t7, const float* b_t7, float* out_rot, float* out_trans, fdipt_stream_t s); /* :1065 */
int fdipt_rigid_invert(int n, const float* t7, float* out_rot, float* out_trans, fdipt_stream_t s);   /* :1132 */
int fdipt_rigid_compose_q_update(int n, const float* t7, const float* upd6, const float* mask, float* out_t7,
                                 fdipt_stream_t s);                                      /* :587,:1039 (fork: update_mask) */
int fdipt_quat_to_rotvec(int n, const float* q, float* rotvec, fdipt_stream_t s);        /* framedipt/data/transforms.py:53-69 */
int fdipt_rigid_from_3_points(int n, const float* p_neg_x_axis, const float* origin, const float* p_xy_plane, float eps,
                              float* rot /* [n,3,3]; the translation is `origin` */, fdipt_stream_t s);  /* :1233-1275 */
/* SO(3) exp / log of the geomstats fork (framedipt/diffusion/so3_utils.py): rot_mat_from_axis_angle_by_exp_map (:90-100),
 * rotation_vector_from_matrix (:120-190, with regularize :193-231), omega (:103-117); float64 buffers */
int fdipt_so3_exp_geomstats(int n, const double* rotvec, double* rot, fdipt_stream_t s);
int fdipt_so3_log_geomstats(int n, const double* rot, double* rotvec, fdipt_stream_t s);
int fdipt_so3_omega(int n, const double* rot, double eps, double* angle, fdipt_stream_t s);
/* SciPy Rotation conventions (float64): exp = from_rotvec().as_matrix(), log = from_matrix().as_rotvec() */
int fdipt_so3_exp(int n, const double* rotvec, double* rot, fdipt_stream_t s);
int fdipt_so3_log(int n, const double* rot, double* rotvec, fdipt_stream_t s);

/* ---------------------------------------------------------------- scores / backbone -------- */
/* SE3Diffuser.calc_rot_score (se3_diffuser.py:281-292 -> so3_diffuser.py:373-402,18-77,122-191): 1000-term IGSO(3)
 * series; quats_t = noisy x_t, quats_0 = prediction, sigma[B] as in FdiptForwardArgs. */
int fdipt_igso3_rot_score(int B, int N, const float* quats_t, const float* quats_0, const double* sigma,
                          const float* res_mask, double* score, fdipt_stream_t s);
/* ... with so3.use_cached_score = True: score_table [B, n_omega], omega_edges [n_omega - 1] as in FdiptForwardArgs. */
int fdipt_igso3_rot_score_cached(int B, int N, const float* quats_t, const float* quats_0, const double* score_table,
                                 const double* omega_edges, int n_omega, const float* res_mask, double* score, fdipt_stream_t s);
/* SE3Diffuser.calc_trans_score(use_torch=True, scale=True) (se3_diffuser.py:269-279 -> r3_diffuser.py:410-440). */
int fdipt_r3_trans_score(int B, int N, const float* trans_t, const float* trans_0, const float* t, float min_b,
                         float max_b, float coordinate_scaling, const float* res_mask, float* score, fdipt_stream_t s);
/* all_atom.compute_backbone (framedipt/protein/all_atom.py:147-176): frames given as tensor_7 (rot==NULL) or as
 * rot [n,3,3] + trans [n,3]; tables = default_frames[21,8,4,4] | ideal_pos[21,14,3] | atom_mask[21,14] (f32) then
 * group_idx[21,14] (i32) packed as in framedipt_amd/residue_tables.py. */
int fdipt_backbone_atoms(int n, const float* t7, const float* rot, const float* trans, const float* psi,
                         const int32_t* aatype, const void* tables, float* atom37, float* atom14, fdipt_stream_t s);

/* ---------------------------------------------------------------- building blocks ---------- */
/* Exposed for parity tests and for callers that assemble their own network. */
/* out[M,N] = epilogue(A[M,K] W[N,K]^T + bias): relu, +residual, *rowmask.  K % 8 == 0, lda/ldw in elements.
 * W is fp32 (precision F32) or the half-precision operand type (F16 / BF16, as produced by fdipt_model_prepare). */
int fdipt_linear(int precision, int M, int N, int K, const float* A, int lda, const void* W, int ldw, const float* bias,
                 const float* residual, int ldr, const float* rowmask, int relu, float* out, int ldo, fdipt_stream_t s);
int fdipt_layernorm(int M, int D, const float* x, const float* residual, const float* gamma, const float* beta,
                    const float* rowmask, float* out, fdipt_stream_t s);
/* self-test of the MFMA fragment maps used by every kernel: returns max |err| of a 64x64x64 product vs fp64 host math
 * through *max_err_host (host pointer). */
int fdipt_selftest_mfma(int precision, double* max_err_host);

/* HIP event helpers for bench.py (kernel timing on the stream the kernels are launched on). */
int fdipt_event_create(void** ev_host);
int fdipt_event_destroy(void* ev);
int fdipt_event_record(void* ev, fdipt_stream_t s);
int fdipt_event_elapsed_ms(void* start, void* stop, float* ms_host); /* synchronises on `stop` */

const char* fdipt_version(void);
/* Lengths N at which the half-precision forward switches kernel variants, ascending, into bounds_host[capacity] (host); returns their
 * number.  Two samples whose lengths (rounded up to 4) fall between the same bounds run the same kernels: padding inside a class does
 * not change a sample's bits (framedipt_amd/sharding.py: kernel_class). */
int fdipt_kernel_class_bounds(int32_t* bounds_host, int capacity);

#ifdef __cplusplus
}
#endif
#endif /* FDIPT_H */
