/*
 * uu3d_ops.h -- building-block operators of the training step's backward pass,
 * exported so that each one can be checked on its own against autograd of the CPU oracle.
 * They replace what TensorFlow's tape.gradient (train.py:477,498) dispatches for the layers of
 * common/net/vision_transformer.py and common/net/uplift_upsample_transformer.py:
 *   Dense / Conv1D kernel gradients (X^T dY), bias and positional-encoding gradients (column sums),
 *   LayerNormalization backward, softmax-attention forward/backward.
 * Same conventions as uu3d.h: device pointers, stream-ordered, int status, no host sync.
 */
#ifndef UU3D_OPS_H_
#define UU3D_OPS_H_

#include <stddef.h>
#include <stdint.h>

#include "uu3d.h" /* uu3d_model, UU3D_SCHEDULE_*: the operators of the spatial stack run on a handle */

#ifdef __cplusplus
extern "C" {
#endif

/* Preconditions common to the operators below: every violation returns UU3D_ERR_INVALID_ARGUMENT before any launch.  A leading
 * dimension (lda, ldb, ldc, ldx, ld, ldo: floats per row) is at least the row's width; the columns beyond the width are neither read nor
 * written.  Where rows move as 16-byte pieces the leading dimension is a multiple of 4 as stated per operator, and the base pointers are
 * 16-byte aligned (not checked).  Results are deterministic: two calls on the same inputs give the same bits. */
/* C[P][Q] = A[R][P]^T B[R][Q]  (dW = X^T dY).  R, P, Q >= 1; P, Q, lda, ldb multiples of 4, lda >= P, ldb >= Q; ldc >= Q, any value (C is
 * stored element by element).  scratch_dev holds the split-K slabs: uu3d_op_scratch_floats() floats give the plan of the training step, a
 * smaller scratch_floats cuts the number of slabs (P * round_up(Q, 4) floats each) down to none -- the product is then stored directly and
 * scratch_dev is not touched; it must not be NULL. */
int uu3d_op_gemm_tn(const float* a_dev, int32_t lda, const float* b_dev, int32_t ldb, int32_t R, int32_t P, int32_t Q,
                    float* c_dev, int32_t ldc, float* scratch_dev, size_t scratch_floats, void* stream);
/* The same product in the f16x3 arithmetic of the training step (gemm_tn_h3_kernel: f16 MFMA on hi / lo planes, fragments
 * read transposed from LDS) when P, Q >= 128; narrower results fall back to the exact-f32 kernel (the bits of uu3d_op_gemm_tn).  Same
 * preconditions and scratch rule. */
int uu3d_op_gemm_tn_h3(const float* a_dev, int32_t lda, const float* b_dev, int32_t ldb, int32_t R, int32_t P, int32_t Q,
                       float* c_dev, int32_t ldc, float* scratch_dev, size_t scratch_floats, void* stream);
/* C[M][N] = A[M][K] W[N][K]^T (dX = dY W^T with W in Keras (in,out) layout: N = in, K = out).
 * M >= 1, N % 64 == 0 and K % 32 == 0 (the training path keeps padded copies); ldw == K; lda >= K and a multiple of 4; ldc >= N, any value.
 * The split along K needs slices * M * N floats of scratch; with less (or scratch_dev NULL) the product runs unsplit. */
int uu3d_op_gemm_nt(const float* a_dev, int32_t lda, const float* w_dev, int32_t ldw, int32_t M, int32_t N, int32_t K,
                    float* c_dev, int32_t ldc, float* scratch_dev, size_t scratch_floats, void* stream);
/* out[(r % period)][c] (+)= sum_r X[r][c] over rows with (mask[r] != 0) == want (mask NULL: all rows). period 0 = 1.  R, C >= 1; R need
 * not be a multiple of period; ldx >= C, any value (rows are read as 16-byte pieces only when ldx and C are multiples of 4).  out is
 * max(period, 1) * C contiguous floats.  scratch_floats below max(period, 1) * C: UU3D_ERR_WORKSPACE, nothing is written. */
int uu3d_op_colsum(const float* x_dev, int32_t ldx, int32_t R, int32_t C, int32_t period, const uint8_t* mask_dev,
                   int32_t want, float* out_dev, int32_t accumulate, float* scratch_dev, size_t scratch_floats, void* stream);
/* (mean, 1/sqrt(var+eps)) per row.  M >= 1; 4 <= D <= 1024, D % 4 == 0; ld >= D and a multiple of 4. */
int uu3d_op_row_stats(const float* x_dev, int32_t ld, int32_t D, int32_t M, float eps, float* stats_dev, void* stream);
/* LayerNormalization backward: dx (written, or added to what dx_dev holds when accumulate != 0), dgamma, dbeta (written).  x, dy and dx
 * share the row stride ld.  M >= 1; 4 <= D <= 1024, D % 4 == 0; ld >= D and a multiple of 4.  scratch holds 2 D floats per workgroup: a
 * smaller scratch_floats gives fewer, longer workgroups with the same dx; below 2 D: UU3D_ERR_WORKSPACE, nothing is written. */
int uu3d_op_ln_bwd(const float* x_dev, const float* dy_dev, const float* stats_dev, const float* gamma_dev, int32_t ld,
                   int32_t D, int32_t M, float* dx_dev, int32_t accumulate, float* dgamma_dev, float* dbeta_dev,
                   float* scratch_dev, size_t scratch_floats, void* stream);
/* softmax attention over rows [q|k|v] (ld floats per row, head h at channels h*dh..), head dim 4 or 48.  B, L, H >= 1, D == H * head_dim,
 * ld >= 3 D, ldo >= D, ld and ldo multiples of 4.  Forward: out has row stride ldo.  Backward: dout has row stride ldo, dqkv the layout
 * and row stride ld of qkv.  key_mask (optional) is B * L bytes, 0 = masked key; a sequence with every key masked attends uniformly.
 * L <= 128 forward, L <= 96 backward (UU3D_ERR_UNSUPPORTED beyond: P and dS of a head live in LDS; 129 .. 416 tokens at head
 * dim 48: uu3d_op_attn_long_fwd / _bwd below) */
int uu3d_op_attn_fwd(const float* qkv_dev, int32_t ld, int32_t D, int32_t B, int32_t L, int32_t H, int32_t head_dim,
                     const uint8_t* key_mask_dev, float* out_dev, int32_t ldo, void* stream);
int uu3d_op_attn_bwd(const float* qkv_dev, const float* dout_dev, int32_t ld, int32_t D, int32_t B, int32_t L, int32_t H,
                     int32_t head_dim, const uint8_t* key_mask_dev, float* dqkv_dev, int32_t ldo, void* stream);
/* The training step's exact-f32 attention for 1 .. 416 tokens, head dim 48 (D == 48 H; UU3D_ERR_UNSUPPORTED otherwise), no attention
 * Dropout.  Forward: out (row stride ldo) and stats_dev, 2 B H L floats: per (sequence, head, query) row the softmax row max and row
 * sum, [B][H][L][2].  Backward: dQ, dK, dV into dqkv_dev in the layout and row stride ld of qkv, from out and dout (row stride ldo)
 * and the forward's stats.  Deterministic: every output element has one writer.  ld and ldo multiples of 4 and every pointer 16-byte
 * aligned (rows move as 16-byte pieces); UU3D_ERR_INVALID_ARGUMENT otherwise. */
int uu3d_op_attn_long_fwd(const float* qkv_dev, int32_t ld, int32_t D, int32_t B, int32_t L, int32_t H, const uint8_t* key_mask_dev,
                          float* out_dev, int32_t ldo, float* stats_dev, void* stream);
int uu3d_op_attn_long_bwd(const float* qkv_dev, const float* out_dev, const float* dout_dev, const float* stats_dev, int32_t ld, int32_t D,
                          int32_t B, int32_t L, int32_t H, const uint8_t* key_mask_dev, float* dqkv_dev, int32_t ldo, void* stream);
/* The forward of uu3d_op_attn_long_fwd without the statistics: the kernel an exact-f32 inference call (UU3D_SCHEDULE_EXACT_F32) takes for
 * its attention layers of 129 .. 416 tokens (attn_long_fwd_kernel<48, false>, launched through the helper the forward launches through).
 * Same shapes, same argument rules and the same bits in out as uu3d_op_attn_long_fwd: D == 48 H and 1 <= L <= 416
 * (UU3D_ERR_UNSUPPORTED otherwise); ld and ldo multiples of 4, both pointers 16-byte aligned (UU3D_ERR_INVALID_ARGUMENT otherwise, before
 * any launch).  Columns of out beyond D (ldo > D) are not written. */
int uu3d_op_attn_long_infer(const float* qkv_dev, int32_t ld, int32_t D, int32_t B, int32_t L, int32_t H, const uint8_t* key_mask_dev,
                            float* out_dev, int32_t ldo, void* stream);
size_t uu3d_op_scratch_floats(void);

/* The forward's row-panel path for a LayerNorm-fed Dense layer on its own (csrc/uu3d_gemm_panel.h; in the model:
 * kl.LayerNormalization + kl.Dense of vit.TransformerBlock / vit.MLP, vision_transformer.py:46-68,135-137,183,188):
 *   out[M][N] = LayerNorm(x[M][384]; gamma, beta, eps) W[384][N] + bias          (relu = 0: f32, row stride ldo)
 *   relu = 1: ReLU of that, written as two f16 planes hi[M][N] | lo[M][N] at out_dev (value = hi + lo / 2048)
 * W comes as the fragment-ordered f16 planes made by uu3d_op_panel_pack from the Keras (in, out) kernel on the HOST;
 * a_scratch_dev holds the fragment-ordered LayerNorm output (uu3d_op_panel_a_bytes(M)).  N % 32 == 0, N <= 1024 * 32 / 32. */
size_t uu3d_op_panel_operand_bytes(int32_t N);
size_t uu3d_op_panel_a_bytes(int32_t M);
int uu3d_op_panel_pack(const float* w_host, int32_t N, void* operand_dev, void* stream);
int uu3d_op_ln_dense_panel(const float* x_dev, int32_t ldx, int32_t M, const float* gamma_dev, const float* beta_dev, float eps,
                           const void* operand_dev, const float* bias_dev, int32_t N, int32_t relu, void* a_scratch_dev,
                           void* out_dev, int32_t ldo, void* stream);

/* ---- forward operators: every kernel the launch schedule of csrc/uu3d_forward.inc selects for a LayerNorm-fed Dense layer, each on its
 * own, launched through the forward's own launch helpers (csrc/uu3d_launch.h) -- tests/test_fwd_ops_gpu.py holds them to float64. ---- */
#define UU3D_EP_BIAS 0              /* out[M][N] f32 (row stride ldo) = v + bias */
#define UU3D_EP_BIAS_RELU_SPLIT 1   /* ReLU(v + bias) as f16 planes hi[M][N] | lo[M][N] at out_dev (value = hi + lo / 2048) */
#define UU3D_EP_BIAS_SPLIT_Q 2      /* v + bias, the first N / 3 columns (q of [q | k | v]) times qscale, as the same two planes; N % 3 == 0 */
#define UU3D_EP_BIAS_RESIDUAL 3     /* residual_dev[M][384] += v + bias in place (row stride 384); N == 384; out_dev is not used */
#define UU3D_EP_BIAS_RESIDUAL_LN 4  /* the same, then LayerNorm(ln2_gamma, ln2_beta, eps) of the finished rows written to ln_out_dev as A
                                     * fragments (uu3d_op_panel_a_bytes(M); rows past M of the last panel are not written): 8 waves, splits 1 */
/* uu3d_op_ln_dense_panel with the schedule spelled out.  waves: 4 (gemm_h3_panel_kernel) or 8 (gemm_h3_panel8_kernel: the contraction
 * split over wave pairs).  splits = S >= 1: column ranges per row tile, each workgroup takes (N / 32) / S chunks of 32 columns; splits 0
 * (4 waves only): the choice of uu3d_op_ln_dense_panel, which is this call with (4, 0) and the epilogue 0 or 1.
 * UU3D_ERR_INVALID_ARGUMENT before any launch, output untouched, for what no kernel is instantiated for: waves not 4 or 8; S not
 * dividing N / 32; more than 32 chunks per workgroup; 8 waves with (N / 32) / S not one of 4, 6, 8, 9, 12 (or splits 0); the residual
 * epilogues with N != 384; UU3D_EP_BIAS_RESIDUAL_LN with anything but (8 waves, S = 1).  Both kernels take any M >= 1: rows past M are read
 * clamped to row M - 1 and never stored, the 8-wave kernel included (its ragged last tile runs the predicated form).
 * With 4 waves the residual epilogue runs the forms with the chunk loop unrolled for S = 1, 2, 3 (what the forward launches) and the
 * runtime chunk loop for S = 4, 6, 12. */
int uu3d_op_ln_dense_panel_ex(const float* x_dev, int32_t ldx, int32_t M, const float* gamma_dev, const float* beta_dev, float eps,
                              const void* operand_dev, const float* bias_dev, int32_t N, int32_t waves, int32_t splits, int32_t epilogue,
                              float qscale, void* a_scratch_dev, void* out_dev, int32_t ldo, float* residual_dev,
                              const float* ln2_gamma_dev, const float* ln2_beta_dev, void* ln_out_dev, void* stream);
/* HOST: the inverse of the A-fragment order (panel_a_index, the order ln_split_frag and the Ln epilogue write): rows 0 .. M - 1 of a
 * fragment buffer copied back from the device, as the values of the two planes, hi_host[M][384] and lo_host[M][384] (value = hi + lo / 2048). */
int uu3d_op_panel_a_unpack(const void* frag_host, int32_t M, float* hi_host, float* lo_host);
/* HOST: its inverse: rows 0 .. M - 1 of the two planes, given as floats that halfs can hold, into frag_host (uu3d_op_panel_a_bytes(M)) through
 * panel_a_index; the elements of rows past M in the last 32-row panel are left as they are. */
int uu3d_op_panel_a_pack(const float* hi_host, const float* lo_host, int32_t M, void* frag_host);

/* vit.MLP of a temporal block in one launch (csrc/uu3d_mlp_fused.h; vision_transformer.py:46-68): the three partial sums
 *   mslab[s][M][384],  sum_s mslab[s] = relu(LayerNorm(x[M][384]) W1 + b1) W2        (W1 384 x 768, W2 768 x 384, Keras (in, out); no b2)
 * which the forward's next LayerNorm launch adds to the residual stream.  uu3d_op_mlp_pack (HOST arrays in, device operand out) packs W1
 * as the row-panel operand and W2 in the k order of fc1's accumulator registers, as uu3d_commit_weights does.  M >= 1. */
size_t uu3d_op_mlp_operand_bytes(void);
int uu3d_op_mlp_pack(const float* w1_host, const float* w2_host, void* operand_dev, void* stream);
int uu3d_op_mlp_fused(const float* x_dev, int32_t ldx, int32_t M, const float* gamma_dev, const float* beta_dev, float eps,
                      const void* operand_dev, const float* b1_dev, void* a_scratch_dev, float* mslab_dev, void* stream);

/* The forward's few-row path (csrc/uu3d_gemm_wt.h: gemm_h3_wt_kernel, LayerNorm in the loader, split-K over the workgroup's waves):
 *   out = epilogue(LayerNorm(x[M][K]) W[K][N] + bias),  epilogue UU3D_EP_BIAS, UU3D_EP_BIAS_RELU_SPLIT or UU3D_EP_BIAS_SPLIT_Q (as above).
 * 1 <= M <= 512 (the forward's few-row limit), K 384 or 768, N % 32 == 0, ldx >= K and a multiple of 4.  The operand is the pair of f16
 * planes hi[N][K] | lo[N][K] (lo scaled by 2048) the model keeps for every Dense kernel, made by uu3d_op_wt_pack from the Keras (in, out)
 * kernel on the HOST. */
size_t uu3d_op_wt_operand_bytes(int32_t N, int32_t K);
int uu3d_op_wt_pack(const float* w_host, int32_t K, int32_t N, void* operand_dev, void* stream);
int uu3d_op_ln_dense_wt(const float* x_dev, int32_t ldx, int32_t M, int32_t K, const float* gamma_dev, const float* beta_dev, float eps,
                        const void* operand_dev, const float* bias_dev, int32_t N, int32_t epilogue, float qscale, void* out_dev,
                        int32_t ldo, void* stream);

/* ---- the forward's temporal attention kernels, each on its own (csrc/uu3d_attn.h, csrc/uu3d_attn_h3.h), launched through the helper the
 * forward's Launcher::attn launches through (launch_attn_infer, csrc/uu3d_launch.h) -- tests/test_attn_infer_gpu.py holds them to float64.
 * B sequences of L tokens, H heads of 48 channels: D == 48 H.  key_mask_dev (optional): B * L bytes, 0 = masked key (its logit gets -1e9);
 * a sequence with every key masked attends uniformly: its context rows are the mean of v. ---- */
#define UU3D_ATTN_AUTO 0        /* the forward's rule (attn_choose) at precision f16x3 with no switch set */
#define UU3D_ATTN_F32_WG 1      /* attn_f32_kernel<ceil(L / 16), 48, SPLIT>: exact f32, one workgroup per (sequence, head); L <= 128 */
#define UU3D_ATTN_HEAD_WAVE 2   /* attn_head_wave_kernel<4 | 5, 48, SPLIT>: exact f32, one wave per (sequence, head); 49 <= L <= 80, H % 4 == 0 */
#define UU3D_ATTN_H3 3          /* attn_h3_kernel<48, MAXW, WPE, MASKED>: f16x3 products, online softmax over 32-key tiles; L <= 416 */
#define UU3D_ATTN_IN_F32 0      /* qkv_dev: [B L][3 D] floats, rows [q | k | v]; the kernel scales the logits by 1 / sqrt(48) itself */
#define UU3D_ATTN_IN_PLANES 1   /* qkv_dev: two f16 planes, hi [B L][3 D] halfs and lo directly behind it (value = hi + lo / 2048), 4 B L 3 D
                                 * bytes; q PRESCALED: already multiplied by log2(e) / sqrt(48), as the QKV projection's epilogue leaves it */
#define UU3D_ATTN_IN_QFRAG 2    /* qkv_dev: the same planes in the temporal chain's fragment order, uu3d_op_attn_qf_bytes(B L) bytes made by
                                 * uu3d_op_attn_qf_pack; q prescaled likewise.  The channels inside a 16-channel group arrive in lane order,
                                 * which q . k does not see and which v carries to the output: output channel 16 u + 8 g + j of a row holds
                                 * what lane 32 g, half j of v's piece (group u) held.  D == 384 */
#define UU3D_ATTN_OUT_F32 0     /* out_dev: [B L][D] floats */
#define UU3D_ATTN_OUT_PLANES 1  /* out_dev: hi [B L][D] halfs, lo directly behind it: 4 B L D bytes */
#define UU3D_ATTN_OUT_FRAG 2    /* out_dev: the row-panel GEMM's A-fragment order, uu3d_op_panel_a_bytes(B L) bytes, read back with
                                 * uu3d_op_panel_a_unpack; rows past B L of the last 32-row panel are not written.  D == 384 */
/* The exact-f32 kernels read UU3D_ATTN_IN_F32 and write any output form; attn_h3_kernel reads planes (either order) and writes planes
 * (either order).  Every device pointer 16-byte aligned.  Returned before any launch, the output untouched:
 *   UU3D_ERR_INVALID_ARGUMENT: a null qkv_dev / out_dev, misaligned pointers, B, L or H < 1, D != 48 H, an unknown kernel or layout;
 *     UU3D_ATTN_F32_WG / _HEAD_WAVE with plane input; UU3D_ATTN_H3 with UU3D_ATTN_IN_F32 or UU3D_ATTN_OUT_F32; UU3D_ATTN_HEAD_WAVE outside
 *     49 .. 80 tokens or with H % 4 != 0; UU3D_ATTN_IN_QFRAG or UU3D_ATTN_OUT_FRAG with D != 384 (the fragment strides are written for 72
 *     groups / 384 columns); UU3D_ATTN_AUTO with layouts the kernel its rule names cannot take (plane input up to 48 tokens in row-major
 *     order; f32 input with plane output above 48 tokens; plane input with f32 output);
 *   UU3D_ERR_UNSUPPORTED (as the forward answers at precision f16x3): the exact-f32 kernels above 128 tokens, attn_h3_kernel above 416.
 *   (A forward CALL at precision f32 takes the tiled exact-f32 kernel there, which is no kernel of this entry: uu3d_op_attn_long_infer.) */
int uu3d_op_attn_infer(const void* qkv_dev, int32_t in_layout, int32_t D, int32_t B, int32_t L, int32_t H, const uint8_t* key_mask_dev,
                       int32_t kernel, void* out_dev, int32_t out_layout, void* stream);
/* bytes of the fragment-ordered q | k | v buffer of `rows` tokens: whole 128-row tiles, as the temporal chain allocates it (0: rows < 1) */
size_t uu3d_op_attn_qf_bytes(int32_t rows);
/* HOST: hi_host / lo_host, f16 planes [rows][1152] of [q | k | v] rows (D = 384), into frag_host (uu3d_op_attn_qf_bytes(rows)) through the
 * producer's own index function (tchain_qf_index, csrc/uu3d_tchain16.h).  Elements of rows past `rows` in the last tile are left as they are. */
int uu3d_op_attn_qf_pack(const void* hi_host, const void* lo_host, int32_t rows, void* frag_host);
/* HOST: its inverse: rows 0 .. rows - 1 of frag_host (rows may reach into the tile rows past the live ones) as f16 planes [rows][1152]. */
int uu3d_op_attn_qf_unpack(const void* frag_host, int32_t rows, void* hi_host, void* lo_host);

/* ---- the forward's TILED GEMMs, each on its own (csrc/uu3d_gemm.h: gemm_f32_kernel, splitk_reduce_kernel; csrc/uu3d_gemm_h3.h: gemm_h3_kernel,
 * gemm_h3g_kernel), launched through the functions the forward's Launcher::gemm / gemm_g launch through (launch_fwd_gemm, launch_fwd_gemm_g,
 * csrc/uu3d_launch.h): tile shape, DEEP form and split are the forward's -- tests/test_fwd_tiled_gpu.py holds them to float64. ----
 * The operand: what uu3d_commit_weights keeps for a Dense / Conv1D kernel, made by the commit's own pack and split functions
 * (csrc/uu3d_pack.h) from the Keras (in, out) kernel w_host[K][N] on the HOST (a Conv1D (3, C, N) kernel flattened: k = j C + c):
 *   Bt[Np][Kp] f32, zero padded, Np = round_up(N, 128), Kp = round_up(K, 32) | its f16 hi plane | its lo * 2048 plane  = 8 Np Kp bytes.
 * uu3d_op_tiled_operand_bytes: 0 for N or K < 1.  uu3d_op_tiled_pack: UU3D_ERR_RANGE (nothing uploaded) for a value of magnitude >= 65504. */
size_t uu3d_op_tiled_operand_bytes(int32_t N, int32_t K);
int uu3d_op_tiled_pack(const float* w_host, int32_t K, int32_t N, void* operand_dev, void* stream);

#define UU3D_A_F32 0            /* ALoadPlain: a_dev = f32 rows [M][lda]; K % 4 == 0, lda >= K, lda % 4 == 0 */
#define UU3D_A_F32_LN 1         /* ALoadLayerNorm: the same rows, LayerNorm in the loader from ln_stats_dev ((mean, rstd) per row, made by
                                 * uu3d_op_row_stats(a_dev, lda, K, M, eps): the launch the forward makes in front of such a layer), ln_gamma_dev, ln_beta_dev */
#define UU3D_A_PLANES 2         /* GLoadPlain: a_dev / a_lo_dev = f16 planes [M][lda] (value = hi + lo / 2048); K % 32 == 0, lda >= K, lda % 8 == 0 */
#define UU3D_A_CONV3_F32 3      /* ALoadConv3: a_dev = f32 rows [B L_in][C]; output row (b, t), M = B L_out, contracts over k = j C + c with row
                                 * t stride + j - pad_left of sequence b, zero outside [0, L_in); K == 3 C, C % 4 == 0 */
#define UU3D_A_CONV3_PLANES 4   /* GLoadConv3: the same gather over f16 planes [B L_in][C]; C % 32 == 0.  The zero source is the operator's */
#define UU3D_EP_BIAS_RELU 5     /* out[M][N] f32 (row stride ldo) = max(v + bias, 0) */
#define UU3D_EP_CONV_RESIDUAL 6 /* EpConvResidual, inference form: out[M][N] = xin[b L_in + t stride + lo][.] + v + bias (+ pe_dev[t][.] when pe_dev != NULL),
                                 * lo = 1 when stride > 1 and pad_left == 0, else 0; every row stride N; (L_out - 1) stride + lo < L_in */
#define UU3D_EP_S2T 7           /* EpSpatialToTemporal, inference form: out[M][N] = (mask_dev == NULL || mask_dev[row] ? v + bias : token_dev[.]) + pe_dev[row % period][.] */
/* UU3D_EP_BIAS, _BIAS_RELU_SPLIT, _BIAS_SPLIT_Q as above (planes: hi[M][N] | lo[M][N] at out_dev).  UU3D_EP_BIAS_RESIDUAL here: out_dev[M][N] += v + bias in place
 * (row stride N, any N); out2_dev != NULL: out2_dev[M][N] = that sum + pe_dev[row % period][.] as well. */
typedef struct uu3d_tiled_dense_args {
    const void* a_dev; const void* a_lo_dev;                  /* the A source (a_lo_dev: plane sources only) */
    const float* ln_stats_dev; const float* ln_gamma_dev; const float* ln_beta_dev;
    const void* operand_dev; const float* bias_dev;           /* uu3d_op_tiled_pack's operand; bias[N] */
    void* out_dev; float* out2_dev;
    const float* xin_dev; const float* pe_dev; const float* token_dev; const uint8_t* mask_dev;
    float* slab_dev; size_t slab_floats;                      /* split-K partial sums and their capacity in floats; 0 forces the unsplit form */
    int32_t a_source, epilogue, precision, splitk_target;    /* UU3D_PREC_F16X3 | UU3D_PREC_F32; the workgroups a split aims for (the forward: 768, or UU3D_THR_SPLITK_TARGET) */
    int32_t M, N, K, lda, ldo;                                /* ldo: UU3D_EP_BIAS / _BIAS_RELU only (>= N) */
    int32_t conv_C, conv_L_in, conv_L_out, conv_stride, conv_pad_left;
    int32_t period; float qscale;
} uu3d_tiled_dense_args;
/* out = epilogue(A-op W + bias).  The (A source, epilogue, precision) combinations csrc/uu3d_forward.inc launches, and no other:
 *   UU3D_A_F32        x UU3D_EP_BIAS (head1, head2), _BIAS_RESIDUAL (proj_res, fc2_res), _S2T (s2t)              f16x3 (gemm_h3_kernel) and f32 (gemm_f32_kernel)
 *   UU3D_A_F32_LN     x UU3D_EP_BIAS (ln_qkv), _BIAS_RELU (ln_fc1)                                               f16x3 and f32
 *   UU3D_A_F32_LN     x UU3D_EP_BIAS_SPLIT_Q (ln_qkv), _BIAS_RELU_SPLIT (ln_fc1)                                 f16x3
 *   UU3D_A_PLANES     x UU3D_EP_BIAS_RESIDUAL (proj_res, fc2_res), _S2T (s2t)                                    f16x3 (gemm_h3g_kernel)
 *   UU3D_A_CONV3_F32  x UU3D_EP_CONV_RESIDUAL (s*.conv_res)                                                      f16x3 and f32
 *   UU3D_A_CONV3_PLANES x UU3D_EP_CONV_RESIDUAL (s*.conv_res)                                                    f16x3 (gemm_h3g_kernel)
 * Anything else, a null pointer the combination needs, a violated shape rule above, M, N or K < 1, M not a multiple of L_out, period < 1 where
 * pe_dev is read, slab_floats != 0 with slab_dev NULL, splitk_target < 1: UU3D_ERR_INVALID_ARGUMENT.  M round_up(max(N, lda), 4) >= 2^29 elements:
 * UU3D_ERR_UNSUPPORTED.  Both before any launch, every output untouched.  Every pointer 16-byte aligned (not checked).  Rows and columns beyond
 * M and N of every buffer are not written. */
int uu3d_op_tiled_dense(const uu3d_tiled_dense_args* args, void* stream);
/* HOST: {slices, k-tiles per slice} the launch of (M, N, K) takes under the forward's split rule (splitk_rule with its exception), for a test to
 * hold its own restatement of the rule against. */
int uu3d_op_tiled_split(int32_t M, int32_t N, int32_t K, int32_t splitk_target, size_t slab_floats, int32_t* slices, int32_t* k_tiles_per_slice);

/* ---- stage 1 of the forward, the SPATIAL STACK, each kernel form on its own (UpliftUpsampleTransformer.spatial_transformation up to, not
 * including, spatial_to_temporal_fc, u_u_t.py:313-330: keypoint embedding + spatial PE, spatial_depth pre-LN blocks of attention over the J
 * joints and an exact-erf GELU MLP, spatial_norm), launched through the helpers the forward's spatial_stage and generic_frame_features launch
 * through (launch_spatial_stack, launch_compact_frames, csrc/uu3d_forward.inc; generic_spatial_launch, csrc/uu3d_train_entry.inc): grid, block,
 * LDS bytes, SpatialParams and fragment arenas are the forward's -- tests/test_spatial_ops_gpu.py holds them to float64. ---- */
#define UU3D_SPATIAL_AUTO 0      /* spatial_stage's own choice for this handle and frame count: uu3d_op_spatial_choice(model, F, UU3D_SCHEDULE_LATENCY) */
#define UU3D_SPATIAL_F32 1       /* spatial_stack_mfma_kernel<17, 3> (csrc/uu3d_spatial.h): exact f32, one wave per 3 frames */
#define UU3D_SPATIAL_H3_TILES 2  /* spatial_stack_h3_kernel<17, 3, kSpatialMT> (csrc/uu3d_spatial_h3.h, inference form): f16x3, 3 frames per workgroup */
#define UU3D_SPATIAL_P16 3       /* spatial_stack_p16_kernel<17, 7, 1> (csrc/uu3d_spatial_p16.h): f16x3, 7 frames per workgroup */
#define UU3D_SPATIAL_OUT_F32 0   /* out_dev: S[F][J d_s] f32 */
#define UU3D_SPATIAL_OUT_PLANES 1/* out_dev: hi[F][J d_s] halfs, lo directly behind it (value = hi + lo / 2048), 4 F J d_s bytes; f16x3 kernels only */
/* S = the spatial stack of frames_dev[F][J][2] on a COMMITTED handle: the kernel reads the handle's own SpatialParams and weight fragments as
 * uu3d_commit_weights packed them (a handle with generic dims: its master parameter buffer).
 *   mask_dev == NULL: every frame is computed.  mask_dev != NULL (F bytes, any nonzero byte = compute): compact_frames_kernel first writes the
 *     list of the frames to compute into frame_list_dev (F + 1 ints, required then; see uu3d_op_compact_frames), as spatial_stage does; the rows
 *     of out_dev of the other frames are NOT written (both planes likewise).
 *   Handles with the compiled dims (J 17, d_s 32, h_s 64, 8 heads, d_t 384): any kernel; the f16x3 kernels need a handle of precision f16x3
 *     (a handle of precision f32 holds no f16 fragments).  UU3D_SPATIAL_AUTO on a handle of precision f32 is UU3D_SPATIAL_F32.
 *   Handles with generic dims: UU3D_SPATIAL_AUTO only, which launches spatial_generic_kernel (csrc/uu3d_spatial_generic.h, exact f32, one
 *     workgroup per frame, any J / d_s / heads / h_s that fits 160 KiB of LDS) exactly as uu3d_frame_features does, the repack of the operand
 *     packs included; no mask (that kernel has no frame list), no planes.
 * Returned before any launch, out_dev untouched:
 *   UU3D_ERR_INVALID_ARGUMENT: a null model, frames_dev or out_dev; F < 1 or F J > 2^30; a mask without frame_list_dev; an unknown kernel or
 *     layout; UU3D_SPATIAL_OUT_PLANES with UU3D_SPATIAL_F32 (or with AUTO where AUTO is that kernel) or on a generic handle; a forced kernel or a
 *     mask on a generic handle; an f16x3 kernel on a handle of precision f32;
 *   UU3D_ERR_NOT_READY: uu3d_commit_weights has not run since the last uu3d_set_weight;
 *   UU3D_ERR_UNSUPPORTED: a generic handle whose frame does not fit the LDS (include/uu3d.h, FRAMES FORM).
 * Rows of out_dev beyond F are not written.  A frame's result does not depend on F, on its index or on the other frames: the same bits.
 * frames_dev 8-byte aligned, out_dev 16-byte aligned (not checked).  The model's range word is not touched. */
int uu3d_op_spatial_stack(uu3d_model* model, const float* frames_dev, int32_t F, const uint8_t* mask_dev, int32_t* frame_list_dev,
                          int32_t kernel, int32_t out_layout, void* out_dev, void* stream);
/* compact_frames_kernel (csrc/uu3d_misc.h) on its own, the launch spatial_stage makes for a masked batch: list_dev[0 .. n - 1] = the indices i
 * of the nonzero bytes mask_dev[i], i < total, in rising order; list_dev[total] = n.  list_dev holds total + 1 ints; its entries n .. total - 1
 * are not written.  One workgroup; mask_dev needs no alignment (16-byte aligned runs of 16 bytes are read as one piece).  total >= 1 and both
 * pointers non-null, else UU3D_ERR_INVALID_ARGUMENT before any launch. */
int uu3d_op_compact_frames(const uint8_t* mask_dev, int32_t total, int32_t* list_dev /* total + 1 ints */, void* stream);
/* HOST: the decision of spatial_stage for a launch of F frames under `schedule` (UU3D_SCHEDULE_LATENCY or _THROUGHPUT, optionally with
 * UU3D_SCHEDULE_EXACT_F32), restated for a test to hold its own statement of the rule against: *kernel = UU3D_SPATIAL_F32, _H3_TILES or _P16,
 * *planes = 1 when the stack leaves S as the f16 planes the spatial-to-temporal GEMM reads.  The rule: an f16x3 kernel iff the call's precision
 * is f16x3 (the handle's, unless the exact-f32 bit is set), UU3D_SPATIAL is not f32, and either UU3D_SPATIAL=h3 or the launch is small enough
 * that the f16x3 rounds are no longer than the exact-f32 kernel's (spatial_h3_pays: ceil(F / 3) workgroups, 1536 per round of 68 us against
 * 1792 per round of 133 us); of the two, UU3D_SPATIAL=h3tiles takes _H3_TILES, anything else _P16; planes iff f16x3, UU3D_NO_PLANES is not 1
 * and J d_s % 32 == 0.  The switches are the handle's, read by uu3d_create.  The handle need not be committed.
 * UU3D_ERR_INVALID_ARGUMENT: a null pointer, F < 1, another schedule value, a handle with generic dims (it has one spatial kernel); the handle is
 * const here: uu3d_last_error is not written. */
int uu3d_op_spatial_choice(const uu3d_model* model, int32_t F, int32_t schedule, int32_t* kernel, int32_t* planes); /* HOST: what spatial_stage takes */

/* ---- the TEMPORAL CHAIN, one launch on its own (csrc/uu3d_tchain16.h: tchain16_kernel<FLAGS>, every row-local stage of a temporal block for the
 * 64 token rows a workgroup owns), launched through the helper the forward's Launcher::tchain launches through (launch_tchain, csrc/uu3d_launch.h):
 * grid, block, LDS bytes and the kernel's argument record are the forward's -- tests/test_tchain_ops_gpu.py holds every stage set to float64. ---- */
#define UU3D_TC_PROJ 1          /* x += attention output . Wp + bp */
#define UU3D_TC_MLP 2           /* x += fc2(relu(fc1(LayerNorm 2 (x)))) */
#define UU3D_TC_QKV 4           /* q | k | v = wqkv(LayerNorm 1 (x)) of the NEXT block, fragment order, q prescaled by log2(e) / sqrt(48) */
#define UU3D_TC_FC1_PLANES 8    /* relu(fc1(LayerNorm 2 (x))) of the first strided block as row-major f16 planes */
#define UU3D_TC_PE 16           /* x + pe[token % period] of the first strided block is what the final LayerNorm 1 reads */
/* Launch `launch` of the chain of a COMMITTED handle, on the handle's own weight stream and parameter table exactly as uu3d_commit_weights folded
 * (LayerNorm's affine part, q's scale) and packed them; uu3d_op_tchain_launches gives the stage set of every launch (launch 0: UU3D_TC_QKV;
 * 1 .. T: PROJ | MLP [| QKV [| PE]]; T + 1 with strided blocks: PROJ | FC1_PLANES).  M >= 1 token rows, any value: whole 64-row tiles run, rows
 * past M read row M - 1 (the attention output: the rows of the last written 16-row group) and store to a trash page inside the scratch.
 *   scratch_dev (uu3d_op_tchain_scratch_bytes(M)): the lane-linear residual tiles between two launches, slot 0 = the temporal stack's, slot 1 = the
 *     first strided block's (x + pe), each ceil(M / 64) tiles of 64 x 384 floats in the order of uu3d_op_tchain_xs_pack, then the trash page.
 *     A launch WITHOUT UU3D_TC_PROJ reads x_dev and stores the tile into slot 0; a launch WITH it reads its residual tile from the scratch (slot 1
 *     for PROJ | FC1_PLANES, else slot 0: whole tiles, the rows past M included); a launch with UU3D_TC_QKV stores the tile its LayerNorm 1 reads
 *     (slot 1 with UU3D_TC_PE, else slot 0), whole tiles.  So launch i + 1 runs on the scratch launch i left, with no host repack.
 *   attn_out_frag_dev (UU3D_TC_PROJ): the attention output as attn_h3_kernel leaves it for fragment-ordered q | k | v (UU3D_ATTN_IN_QFRAG,
 *     UU3D_ATTN_OUT_FRAG): A-fragment order (uu3d_op_panel_a_pack, uu3d_op_panel_a_bytes(M)), channel 16 u + 8 g + j of a row holding context
 *     channel 16 u + 8 (j >> 2) + 4 g + (j & 3) -- the projection's rows are packed in that order.  The rows past M of the last 32-row panel are read
 *     (dead lanes only): initialised memory.
 *   x_dev [M][384]: read by a launch without UU3D_TC_PROJ; written (rows < M) by a launch with UU3D_TC_MLP that has no UU3D_TC_QKV or has UU3D_TC_PE.
 *   xa_dev [M][384], h_dev (hi [M][768] halfs | lo [M][768] halfs): written (rows < M) by PROJ | FC1_PLANES: x + projection, and relu(fc1).
 *   q_dev (UU3D_TC_QKV): uu3d_op_attn_qf_bytes(M) bytes; the 64-row tiles that hold a live row are written whole.
 *   The positional encoding and its period of UU3D_TC_PE are the handle's: the first strided block's, num_frames rows; M need not be a multiple.
 * Pointers a launch's stage set does not use may be NULL.  Returned before any launch, every buffer untouched:
 *   UU3D_ERR_INVALID_ARGUMENT: a null model; M < 1 (or M 1152 4 >= 4e9, the forward's limit); launch < 0 or >= the number of launches; a null
 *     scratch_dev or a null pointer the stage set reads or writes;
 *   UU3D_ERR_NOT_READY: uu3d_commit_weights has not run since the last uu3d_set_weight;
 *   UU3D_ERR_UNSUPPORTED: the handle has no chain (precision f32, or d_t / h_t / heads other than 384 / 768 / 8, or no temporal block).
 * Every pointer 16-byte aligned (not checked).  A row's results do not depend on M, on its place in the tile or on the other rows: the same bits.
 * The model's range word is not touched. */
int uu3d_op_tchain(uu3d_model* model, int32_t launch, int32_t M, const void* attn_out_frag_dev, float* x_dev, float* xa_dev, void* q_dev,
                   void* h_dev, void* scratch_dev, void* stream);
size_t uu3d_op_tchain_scratch_bytes(int32_t M);      /* tchain16_scratch_bytes(ceil(M / 64)); 0 for M < 1 */
/* HOST: flags_out[i] = the stage set (UU3D_TC_*) of launch i for i < capacity; returns the number of launches (0: the handle has no chain or is
 * not committed), -1 for a null handle, capacity < 0 or a null flags_out with capacity > 0.  uu3d_last_error is not written. */
int uu3d_op_tchain_launches(const uu3d_model* model, int32_t* flags_out, int32_t capacity);
/* HOST: rows 0 .. rows - 1 of x_host[rows][384] to / from the lane-linear residual tiles of slot 0 or 1 of a scratch for M rows, through
 * tchain16_xs_index.  rows <= 64 ceil(M / 64): the tile rows past M can be given and read.  Other elements of the scratch are left as they are. */
int uu3d_op_tchain_xs_pack(const float* x_host, int32_t M, int32_t slot, int32_t rows, void* scratch_host);
int uu3d_op_tchain_xs_unpack(const void* scratch_host, int32_t M, int32_t slot, int32_t rows, float* x_host);

/* ---- TRAINING GEMMS: every loader and epilogue the training step (csrc/uu3d_train_forward.inc, csrc/uu3d_train_backward.inc) hands to its tiled
 * GEMMs, each on its own, launched through the step's own host dispatch (launch_gemm, launch_gemm_tn, launch_colsum, launch_ln_bwd_rows,
 * launch_ln_bwd_combine, csrc/uu3d_launch.h): kernel, DEEP form, slice count and combine are the step's -- tests/test_train_gemm_ops_gpu.py
 * holds them to float64. ----
 * The operand: one PackDesc of csrc/uu3d_train_kernels.h run through repack_kernel itself, from the Keras (in, out) kernel w_dev[K][N] on the DEVICE
 * into a block this call zeroes first, padded as csrc/uu3d_train_state.inc allocates it:
 *   kind 1 (forward)        Bt[round_up(N, 128)][round_up(K, 32)],        Bt[n][k] = W[k][n]
 *   kind 4 (backward)       WK[round_up(K, 64)][round_up(N, 32)],         WK[k][n] = W[k][n]            (dX = dY W^T reads rows of W)
 *   kind 5 (conv-transpose) WT[round_up(C, 128)][round_up(3 N, 32)],      WT[c][j N + n] = W[j C + c][n]   (K == 3 C)
 * The block is the f32 operand | its f16 hi plane | its lo * 2048 plane (written by the same pass), 8 bytes per padded element.
 * uu3d_op_train_operand_bytes: 0 for K or N < 1, K N >= 2^28, an unknown kind, kind 5 with K != 3 C (uu3d_op_train_pack refuses the same with
 * UU3D_ERR_INVALID_ARGUMENT).  uu3d_op_train_pack synchronises the stream. */
size_t uu3d_op_train_operand_bytes(int32_t kind, int32_t K, int32_t N, int32_t C);
int uu3d_op_train_pack(const float* w_dev, int32_t kind, int32_t K, int32_t N, int32_t C, void* operand_dev, void* stream);

#define UU3D_TA_PLAIN 0         /* ALoadPlain / TnLoadPlain: a_dev = f32 rows, row stride lda (a multiple of 4, >= the row's width) */
#define UU3D_TA_LN 1            /* ALoadLayerNorm / TnLoadLayerNorm: the same rows, LayerNorm in the loader from ln_stats_dev (uu3d_op_row_stats), ln_gamma_dev, ln_beta_dev */
#define UU3D_TA_GELU 2          /* ALoadGelu / TnLoadGelu: gelu(a_dev), exact erf */
#define UU3D_TA_CONV3 3         /* ALoadConv3 / TnLoadConv3: a_dev = f32 rows [B L_in][conv_C]; row (b, t) of B L_out rows contracts over k = j C + c with row
                                 * t stride + j - pad_left of sequence b, zero outside [0, L_in); the contraction length is 3 C, C % 4 == 0 */
#define UU3D_TA_CONVT 4         /* ALoadConvT: the transposed strided convolution as a gather; a_dev = f32 rows [B L_out][conv_C]; row (b, src) of M = B L_in rows
                                 * contracts over k = j C + n with row t = (src + pad_left - j) / stride of sequence b where that divides and t < L_out, else zero */
#define UU3D_TEP_STORE 0         /* EpStore: out[M][N] = v (row stride ldo) */
#define UU3D_TEP_BIAS 1          /* EpBias: v + bias */
#define UU3D_TEP_BIAS_RELU 2     /* EpBiasRelu: max(v + bias, 0) */
#define UU3D_TEP_BIAS_RES_GATE 3 /* EpBiasResGate: out = aux + (((v + bias) * dropout factor) / keep) * gate[row / rps]; aux_dev = the residual stream (row stride
                                  * ldo, as out); gate_dev NULL: no division, no gate; drop_rate 0: no Dropout, else the factor of oracle/dropout_oracle.py at
                                  * (drop_seed, drop_site, element row * ldo + col); out2_dev != NULL: out2 = out + pe_dev[row % period][.] (row stride ldo) */
#define UU3D_TEP_ADD 4           /* EpAdd: out += v */
#define UU3D_TEP_RELU_MASK 5     /* EpReluMask: out = aux > 0 ? v * scale : 0; aux_dev = H, the ReLU output (row stride ldo) */
#define UU3D_TEP_GELU_GRAD 6     /* EpGeluGrad: out = v * gelu'(aux); aux_dev = the GELU's input (row stride ldo) */
#define UU3D_TEP_CONV_RESIDUAL 7 /* EpConvResidual, training form: out = aux[b L_in + t stride + lo][.] + (((v + bias) * dropout factor) / keep) * gate[row / L_out]
                                  * (+ pe_dev[t][.] when pe_dev != NULL); lo = 1 when stride > 1 and pad_left == 0, else 0; (L_out - 1) stride + lo < L_in;
                                  * a gate needs rps == conv_L_out; every row stride ldo */
typedef struct uu3d_train_dense_args {
    const float* a_dev;
    const float* ln_stats_dev; const float* ln_gamma_dev; const float* ln_beta_dev;
    const void* operand_dev; const float* bias_dev;           /* uu3d_op_train_pack's block of kind operand_kind; bias[N] */
    float* out_dev; float* out2_dev;
    const float* aux_dev; const float* pe_dev; const float* gate_dev;
    float* slab_dev; size_t slab_floats;                      /* split-K partial sums and their capacity in floats; 0 (or NULL) forces the unsplit form */
    uint64_t drop_seed;
    int32_t a_source, epilogue, precision, operand_kind;     /* UU3D_PREC_F16X3 (the block's planes) | UU3D_PREC_F32 (Bh = Bl = NULL) */
    int32_t M, N, K, lda, ldo;                                /* the GEMM's dims: round_up(K, 32) is the block's row stride, N at most its rows */
    int32_t conv_C, conv_L_in, conv_L_out, conv_stride, conv_pad_left;
    int32_t rps, period; uint32_t drop_site;
    float keep, scale, drop_rate;
} uu3d_train_dense_args;
/* out = epilogue(A-op W) through launch_gemm (64 x 64 tiles; f16x3: gemm_h3_kernel, DEEP at up to UU3D_GEMM_DEEP_WGS workgroups; f32: gemm_f32_kernel;
 * split along K under splitk_rule(target 768) with EpSlab and splitk_reduce_kernel<epilogue>).  The (A source, epilogue, operand kind) combinations the
 * step launches, and no other, each at both precisions:
 *   UU3D_TA_GELU  x UU3D_TEP_BIAS_RES_GATE, kind 1      the unfused spatial fc2                                 uu3d_train_forward.inc: forward_spatial
 *   UU3D_TA_PLAIN x UU3D_TEP_BIAS_RES_GATE, kind 1      projections and fc2 (out2 / pe: the last temporal fc2)  block_forward, forward_spatial, forward_temporal
 *   UU3D_TA_LN    x UU3D_TEP_BIAS, _BIAS_RELU, kind 1   q | k | v and fc1 below 1024 rows                       block_forward
 *   UU3D_TA_CONV3 x UU3D_TEP_CONV_RESIDUAL, kind 1      the strided convolution                                 forward_temporal
 *   UU3D_TA_CONVT x UU3D_TEP_RELU_MASK, kind 5          d hidden of a strided block                             uu3d_train_backward.inc: the strided loop
 *   UU3D_TA_PLAIN x UU3D_TEP_GELU_GRAD, _RELU_MASK, kind 4   d hidden of a spatial / temporal block             block_backward
 *   UU3D_TA_PLAIN x UU3D_TEP_ADD, kind 4                head1's input gradient added to d t_out                 backward
 *   UU3D_TA_PLAIN x UU3D_TEP_STORE, kind 4              every other input-gradient GEMM                         attn_half, block_backward, backward
 * Anything else, a null pointer the combination needs, M or N < 1, K < 4 or K % 4 != 0, lda < K or lda % 4 != 0 (row sources), conv_C % 4 != 0 or
 * K != 3 conv_C, M not a multiple of L_out (CONV3) / L_in (CONVT), ldo < N, a gate with keep <= 0 or rps < 1, drop_rate outside [0, 1), out2 without
 * pe_dev or with period < 1, slab_floats != 0 with slab_dev NULL: UU3D_ERR_INVALID_ARGUMENT.  2^29 elements or more in a buffer: UU3D_ERR_UNSUPPORTED.
 * Both before any launch, every output untouched.  Every pointer 16-byte aligned (not checked).  Rows and columns beyond M and N are not written. */
int uu3d_op_train_dense(const uu3d_train_dense_args* args, void* stream);

#define UU3D_WEP_STORE 0        /* EpStore: out[P][Q], row stride ldo */
#define UU3D_WEP_STORE3 1       /* EpStore3: the three column blocks of Q / 3 columns to out_dev, out1_dev, out2_dev, each [P][Q / 3] contiguous */
typedef struct uu3d_train_wgrad_args {
    const float* a_dev;                                       /* [R][lda]; UU3D_TA_CONV3: [B L_in][conv_C] */
    const float* ln_stats_dev; const float* ln_gamma_dev; const float* ln_beta_dev;
    const float* b_dev;                                       /* [R][ldb] */
    float* out_dev; float* out1_dev; float* out2_dev;
    float* slab_dev; size_t slab_floats;                      /* a smaller capacity cuts the number of slabs (P round_up(Q, 4) floats each) down to none */
    int32_t a_source, epilogue, h3;                           /* h3 1: gemm_tn_h3_kernel when P, Q >= 128, else gemm_tn_kernel (exact f32) */
    int32_t R, P, Q, lda, ldb, ldo;
    int32_t conv_C, conv_L_in, conv_L_out, conv_stride, conv_pad_left;
} uu3d_train_wgrad_args;
/* C[P][Q] = A-op[R][P]^T B[R][Q] through launch_gemm_tn.  The combinations the step launches, and no other:
 *   UU3D_TA_LN x UU3D_WEP_STORE3 (d Wq | Wk | Wv, attn_half), UU3D_TA_LN x UU3D_WEP_STORE (d W1), UU3D_TA_GELU x UU3D_WEP_STORE (d W2 of a spatial
 *   block), UU3D_TA_CONV3 x UU3D_WEP_STORE (d of the strided convolution's kernel), UU3D_TA_PLAIN x UU3D_WEP_STORE (uu3d_op_gemm_tn / _h3).
 * R >= 1; P, Q >= 4 and multiples of 4; lda >= P, ldb >= Q, both multiples of 4; UU3D_WEP_STORE: ldo >= Q; UU3D_WEP_STORE3: Q % 3 == 0 and three outputs;
 * UU3D_TA_CONV3: P == 3 conv_C, conv_C % 4 == 0, R a multiple of L_out.  UU3D_ERR_INVALID_ARGUMENT otherwise, before any launch. */
int uu3d_op_train_wgrad(const uu3d_train_wgrad_args* args, void* stream);

/* launch_colsum into ReduceOut{out0, out1, out2, seg} (the q | k | v bias gradients of attn_half): out_s[c] (+)= sum_r X[r][s seg + c], s < 3, c < seg.
 * R, seg >= 1; ldx >= 3 seg.  scratch_floats below 3 seg: UU3D_ERR_WORKSPACE, nothing is written. */
int uu3d_op_colsum3(const float* x_dev, int32_t ldx, int32_t R, int32_t seg, float* out0_dev, float* out1_dev, float* out2_dev, int32_t accumulate,
                    float* scratch_dev, size_t scratch_floats, void* stream);
/* uu3d_op_ln_bwd as the step launches it (launch_ln_bwd_rows + launch_ln_bwd_combine): dx = d x, or res + d x when res_dev != NULL (res_dev may be
 * dx_dev: each element is read by the lane that writes it); gate_dev != NULL: gated_out_dev = (dx / keep) * gate[row / rps] as well (LnBwdGated: the
 * copy the next Dense-layer backward reads), row stride ld; gate_dev and gated_out_dev both or neither, keep > 0, rps >= 1.  dgamma, dbeta written.
 * Shapes and scratch as uu3d_op_ln_bwd. */
int uu3d_op_ln_bwd_ex(const float* x_dev, const float* dy_dev, const float* stats_dev, const float* gamma_dev, int32_t ld, int32_t D, int32_t M,
                      float* dx_dev, const float* res_dev, const float* gate_dev, float keep, int32_t rps, float* gated_out_dev, float* dgamma_dev,
                      float* dbeta_dev, float* scratch_dev, size_t scratch_floats, void* stream);
/* identity_bwd_kernel (the gradient of trim + MaxPool1D(1, stride) as a gather): dmid[b L_in + r][.] = dout[b L_out + (r - lo) / stride][.] where
 * r >= lo, stride divides r - lo and the quotient is below L_out, else 0.  Dense rows of D floats.  B, L_in, L_out, stride, D >= 1, lo >= 0. */
int uu3d_op_identity_bwd(const float* dout_dev, int32_t B, int32_t L_in, int32_t L_out, int32_t stride, int32_t lo, int32_t D, float* dmid_dev, void* stream);
/* scale_rows_kernel: out[r][.] = in[r][.], divided by keep and times gate[r / rps] when gate_dev != NULL, then 0 where row_mask_dev != NULL and
 * (row_mask_dev[r] != 0) != want.  Dense rows of D floats.  rows, D >= 1; want 0 or 1; a gate needs keep > 0 and rps >= 1. */
int uu3d_op_scale_rows(const float* in_dev, int32_t rows, int32_t D, const float* gate_dev, float keep, int32_t rps, const uint8_t* row_mask_dev,
                       int32_t want, float* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UU3D_OPS_H_ */
