/*
 * uu3d.h -- C ABI of the MI355X-native uplift/upsample 3D-HPE transformer forward path.
 *
 * This is the drop-in boundary of the hot path.  The reference has
 * no FFI of its own: the path sits behind a Keras model object,
 *
 *     model = build_uplift_upsample_transformer(config)
 *         (/root/reference/common/net/uplift_upsample_transformer_constructor.py:14-50)
 *     full, central = model([x, stride_mask], training=False)
 *         (/root/reference/common/net/uplift_upsample_transformer.py:388-421)
 *
 * so every entry point below cites the reference call it replaces.  The host-side mirror
 * of the Keras interface (uplift-upsample-3dhpe_amd/net/...) binds exactly these symbols
 * through ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions: plain C, no exceptions cross the ABI, every function returns a uu3d_status
 * (0 = ok).  Pointers named *_dev are device (HBM) pointers on the model's device; all
 * other pointers are host pointers.  `stream` is a hipStream_t passed as void* (NULL =
 * the null stream).  Calls are stream-ordered and perform no host synchronisation unless
 * stated.  The caller owns every buffer it passes in; the model owns its weights.
 */
#ifndef UU3D_H_
#define UU3D_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UU3D_MAX_STRIDED 8

typedef enum uu3d_status {
    UU3D_OK = 0,
    UU3D_ERR_INVALID_ARGUMENT = 1, /* NULL pointer, bad size, unknown weight name ...        */
    UU3D_ERR_UNSUPPORTED = 2,      /* config is schema-legal but outside the compiled / generic kernels */
    UU3D_ERR_SHAPE = 3,            /* tensor element count does not match the model           */
    UU3D_ERR_NOT_READY = 4,        /* forward before every weight was set and committed       */
    UU3D_ERR_WORKSPACE = 5,        /* workspace too small / misaligned                        */
    UU3D_ERR_HIP = 6,              /* a HIP runtime call failed (see uu3d_last_error)          */
    UU3D_ERR_NO_DEVICE = 7,        /* no usable gfx950 device                                 */
    UU3D_ERR_RANGE = 8             /* uu3d_range_status: a forward produced non-finite outputs -- activations left the f16 range of the
                                      f16x3 products (|x| >= 65504), or its inputs were not finite                                    */
} uu3d_status;

/* Arithmetic the GEMM-shaped work is carried out in. */
typedef enum uu3d_precision {
    UU3D_PREC_F32 = 0,     /* f32-input MFMA (v_mfma_f32_32x32x2_f32 / 16x16x4_f32), exact f32 */
    UU3D_PREC_F16X3 = 1    /* forward GEMMs as 3 f16 MFMA passes on hi/lo-split operands: f32-grade error,
                              f16-rate matrix pipe (csrc/uu3d_gemm_h3.h).  Attention, spatial stack, LayerNorm,
                              softmax and every epilogue stay f32.  The training step runs its forward, input-gradient
                              and weight-gradient GEMMs the same way (loss-scaled, see uu3d_train_forward_backward);
                              UU3D_TRAIN_F32=1 / UU3D_TN_F32=1 in the environment keep them on the exact-f32 kernels. */
} uu3d_precision;

/*
 * Architecture hyper-parameters: the keyword arguments the reference constructor derives
 * from the config (uplift_upsample_transformer_constructor.py:15-43) and hands to
 * UpliftUpsampleTransformer.__init__ (uplift_upsample_transformer.py:165-177).
 */
typedef struct uu3d_config {
    int32_t num_frames;          /* SEQUENCE_LENGTH (token count N)                     */
    int32_t num_keypoints;       /* NUM_KEYPOINTS (J)                                   */
    int32_t d_spatial;           /* SPATIAL_EMBED_DIM                                   */
    int32_t d_temporal;          /* TEMPORAL_EMBED_DIM                                  */
    int32_t h_spatial;           /* int(d_spatial  * MLP_RATIO)                         */
    int32_t h_temporal;          /* int(d_temporal * MLP_RATIO)                         */
    int32_t spatial_depth;       /* SPATIAL_TRANSFORMER_BLOCKS                          */
    int32_t temporal_depth;      /* TEMPORAL_TRANSFORMER_BLOCKS                         */
    int32_t num_strided;         /* len(STRIDES)                                        */
    int32_t strides[UU3D_MAX_STRIDED];
    int32_t pad_left[UU3D_MAX_STRIDED];   /* PADDINGS[i][0] ([1,1] when PADDINGS is null) */
    int32_t pad_right[UU3D_MAX_STRIDED];  /* PADDINGS[i][1]                               */
    int32_t num_heads;           /* NUM_HEADS                                           */
    int32_t qkv_bias;            /* QKV_BIAS                                            */
    int32_t has_strided_input;   /* constructor.py:16-21                                */
    int32_t first_strided_token_attention_layer; /* FIRST_STRIDED_TOKEN_ATTENTION_LAYER */
    int32_t full_output;         /* not USE_REFINE                                      */
    int32_t precision;           /* uu3d_precision                                      */
    int32_t output_bn;           /* OUTPUT_BN: BatchNormalization(momentum 0.1, eps 1e-5) in front of both heads
                                    (uplift_upsample_transformer.py:275-285).  uu3d_forward: moving statistics, folded into
                                    the head operands at commit time; the training step: batch statistics (see there)   */
    int32_t learnable_masked_token; /* TOKEN_MASK_RATE > 0 and LEARNABLE_MASKED_TOKEN: the model owns one more weight,
                                    "learnable_masked_token_layer/learnable_masked_token" (d_temporal,), the value random token
                                    masking writes in training mode (uplift_upsample_transformer.py:38-50,219-220,337); unused
                                    at inference                                                                        */
} uu3d_config;

typedef struct uu3d_model uu3d_model;

/* Library / build information: "uu3d <version> gfx950 ...". Never NULL. */
const char* uu3d_version(void);
const char* uu3d_status_string(int status);
/* Human-readable detail of the last failure on this model (or of the last failed
 * uu3d_create when model == NULL).  Never NULL. */
const char* uu3d_last_error(const uu3d_model* model);

/*
 * Replaces: build_uplift_upsample_transformer(config) -> model
 * (uplift_upsample_transformer_constructor.py:14-50).  Creates the model on HIP device
 * `device` with all weight storage allocated but unset.
 * The specialised kernels are compiled for J = 17, SPATIAL_EMBED_DIM 32, TEMPORAL_EMBED_DIM 384, NUM_HEADS 8, MLP_RATIO 2 (every
 * shipped config).  Other dims the constructor accepts (:26-32) give a handle whose forward (uu3d_forward_ex) and training step run on
 * generic, untuned kernels: embed dims and MLP widths multiples of 4, head dims in {2, 4, 8, 12, 16, 24, 32, 48, 64}, <= 128 keypoints, <= 128 frames, >= 1 temporal and strided
 * block, the full-sequence head.  The generic attention keeps a head in LDS: the FORWARD holds 2 L (d_h + 4) floats (fits every legal shape), the training
 * step's BACKWARD 4 L (d_h + 4) + 2 L (L + 1) floats <= 160 KiB -- i.e. up to 128 frames only for head dims <= 8 (and 48, which has an MFMA backward;
 * 96 with ATTENTION_DROP_RATE > 0), 127 at 12, 124 at 16, 117 at 24, 111 at 32, 90 at 64; uu3d_train_forward_backward refuses longer sequences up front.  Outside that: UU3D_ERR_UNSUPPORTED.
 * Training-step token limits (every handle): attention layers of head dim 48 without ATTENTION_DROP_RATE train up to 416 tokens -- up to 128
 * on the register-resident kernels, 129 .. 416 on the tiled exact-f32 pair of csrc/uu3d_attn_long.h (row statistics saved by the forward, P
 * recomputed by the backward, deterministic); other head dims up to 128 (and the LDS bound above); ATTENTION_DROP_RATE > 0 up to 96.
 * Training-step structures (compiled dims): temporal_depth == 0 (no full-sequence head; strided block 1 takes the key mask when the model has
 * strided input), num_strided == 0 (head2 reads the central token x[:, N // 2] of the temporal stack's output) and both at once train
 * like the shipped structure.  Refused with UU3D_ERR_UNSUPPORTED: full_output == 0 with temporal blocks (USE_REFINE), and generic-dims
 * handles without a temporal or a strided block (uu3d_create refuses those already).
 */
int uu3d_create(const uu3d_config* config, int device, uu3d_model** out_model);
void uu3d_destroy(uu3d_model* model);

/*
 * Weight inventory in the reference's creation order, Keras layouts
 * (Dense kernel (in,out), Conv1D kernel (k,in,out)); names follow the Keras layer names
 * given at uplift_upsample_transformer.py:198-285, e.g.
 * "temporal_block_1/attn/wq/kernel".  Replaces model.weights / get_weights / set_weights
 * (train.py:400,503) and the by-name h5 loader's target (common/utils/weight_io.py:172-235).
 */
int uu3d_num_weights(const uu3d_model* model);
int uu3d_weight_info(const uu3d_model* model, int index, const char** out_name,
                     int32_t* out_ndim, int64_t out_dims[4]);
/* Copy `numel` host floats into the named weight.  Stages on the host; nothing reaches
 * the device until uu3d_commit_weights. */
int uu3d_set_weight(uu3d_model* model, const char* name, const float* host_data, int64_t numel);
int uu3d_get_weight(const uu3d_model* model, const char* name, float* host_out, int64_t numel);
/* Repack every weight into the device layouts the kernels read ([N][K]-transposed,
 * padded GEMM operands, fused QKV) and upload.  Fails with UU3D_ERR_NOT_READY (and names
 * the first missing tensor in uu3d_last_error) if any weight was never set.
 * Synchronises `stream` before returning. */
int uu3d_commit_weights(uu3d_model* model, void* stream);

/* Bytes of device scratch uu3d_forward needs for `batch` sequences (256-byte aligned). */
size_t uu3d_workspace_bytes(const uu3d_model* model, int32_t batch);

/*
 * Replaces: model([x, stride_mask], training=False) -> (full_output, central_output)
 * (uplift_upsample_transformer.py:388-421; called at eval.py:70, train.py:520).
 *   kp2d_dev        (B, N, J, 2) f32.  The CALLER zeroes masked frames (eval.py:67).
 *   stride_mask_dev (B, N) uint8, 1 = real 2D input present; must be NULL iff the model
 *                   has no strided input.
 *   full_out_dev    (B, N, J, 3) f32, or NULL to skip head1 (must be NULL-able only when
 *                   full_output == 0 / temporal_depth == 0, where the reference returns None).
 *   central_out_dev (B, J, 3) f32.
 */
int uu3d_forward(uu3d_model* model, const float* kp2d_dev, const uint8_t* stride_mask_dev,
                 int32_t batch, float* full_out_dev, float* central_out_dev,
                 void* workspace_dev, size_t workspace_bytes, void* stream);
/* The same forward with return_attention=True (uplift_upsample_transformer.py:365,418-419: `att_list`, the softmax weights every temporal
 * block's MHA returns, vision_transformer.py:117-130): attn_out_dev_ptrs is a HOST array of temporal_depth device pointers, each
 * (B, num_heads, N, N) f32 (or NULL to skip that block); NULL = uu3d_forward.  The maps are recomputed from the block's q | k by a
 * separate kernel -- the attention kernels of the hot path never materialise them.  Sequences of up to ~800 tokens (K of one head in LDS). */
int uu3d_forward_attention(uu3d_model* model, const float* kp2d_dev, const uint8_t* stride_mask_dev, int32_t batch,
                           float* full_out_dev, float* central_out_dev, float* const* attn_out_dev_ptrs,
                           void* workspace, size_t workspace_bytes, void* stream);


/*
 * Replaces: metrics.mpjpe(pred, gt, root_index, normalize=False)
 * (common/dataset/metrics.py:13-37) on device, float64 like the reference's numpy call:
 * root-align pred and gt, per-joint L2 distance; -1 where gt valid flag <= 0.
 *   pred_dev (B, J, 3) f32; gt_dev (B, J, 4) f32 (x, y, z, valid); out_dev (B, J) f64.
 * This (B_local, J) block is the payload of the multi-GPU all-gather.
 */
int uu3d_mpjpe(const float* pred_dev, const float* gt_dev, int32_t batch, int32_t num_keypoints,
               int32_t root_index, double* out_dev, void* stream);

/*
 * The evaluation report on the device.  Replaces evaluation._frame_metrics (metrics.mpjpe, metrics.nmpjpe(alignment="root"),
 * metrics.pmpjpe, all normalize=False; common/dataset/metrics.py:13-201), interpolate_between_keyframes
 * (common/dataset/action_wise_eval.py:77-100) and the sums behind h36_action_wise_eval / frame_wise_eval (:17-74), in float64.
 * Stream-ordered, no host synchronisation.
 *
 *   pred_dev (num_rows, J, 3), gt_dev (num_poses, J, gt_channels): float32 (inputs_f64 = 0: the product path; run_eval and
 *     run_train never pass anything else), widened exactly.  inputs_f64 = 1 reads both as float64: a verification aid, there so that
 *     poses which exist in float64 only (the reference's own metric fixtures) can be held to the 1e-9 m bounds without rounding the
 *     inputs first; it runs the same kernel source with another load type.  gt_channels 3: every joint valid; 4: (x, y, z, valid), a joint with valid <= 0 gives -1.  J <= 32.
 *   left_dev / right_dev (num_poses) int32, weight_dev (num_poses) float64: pose i is
 *     pred[left[i]] * (1 - weight[i]) + pred[right[i]] * weight[i], formed in float64 and never written to memory
 *     (evaluation.keyframe_plan builds the three arrays).  weight_dev NULL: pose i is pred[left[i]]; left_dev NULL as well: row i.
 *     A row index outside [0, num_rows) makes the pose NaN: it drops out of every sum.
 *   errors_out_dev (num_poses, J, 3) float64 or NULL: (mpjpe, nmpjpe, pmpjpe) per joint in metres.
 *   sums_out_dev (num_actions + 1, 3, 2) float64 or NULL: per action and metric the sum of the errors >= 0 and their count; the last
 *     row is over all poses.  actions_dev (num_poses) int32 (NULL with num_actions = 0); an action outside [0, num_actions) counts in
 *     the last row only.  num_actions <= 63.  Partial sums per workgroup in a fixed order and one ordered combine: no floating-point
 *     atomics, two calls give the same bits.  Needs scratch of uu3d_error_sums_scratch_bytes(num_poses, num_actions) bytes.
 *   select_dev (num_poses) uint8 or NULL: poses with 0 are not evaluated (their rows are not read, their errors are -1, they are in
 *     no sum) -- the KEYFRAMES report.
 * At least one of errors_out_dev / sums_out_dev.  The sums of the fused call and of uu3d_error_sums on its error array agree bit for bit
 * only while a tile holds 64 poses (J = 17 in float32 does); larger poses are tiled smaller and summed in another order.
 */
int uu3d_pose_errors(const void* pred_dev, int64_t num_rows, const int32_t* left_dev, const int32_t* right_dev,
                     const double* weight_dev, const void* gt_dev, int64_t num_poses, int32_t num_keypoints, int32_t gt_channels,
                     int32_t root_index, int32_t inputs_f64, double* errors_out_dev, const int32_t* actions_dev,
                     int32_t num_actions, const uint8_t* select_dev, double* sums_out_dev, void* scratch, size_t scratch_bytes,
                     void* stream);

/* The sums table of uu3d_pose_errors from an error array (num_poses, J, 3) float64 that is already in memory (any number of joints). */
int uu3d_error_sums(const double* errors_dev, int64_t num_poses, int32_t num_keypoints, const int32_t* actions_dev,
                    int32_t num_actions, const uint8_t* select_dev, double* sums_out_dev, void* scratch, size_t scratch_bytes,
                    void* stream);

/* Scratch bytes of the two calls above (0 for arguments they would refuse). */
size_t uu3d_error_sums_scratch_bytes(int64_t num_poses, int32_t num_actions);

/*
 * "Next" row 3 of the scope table: the window / stride-mask generator as a gather over a RESIDENT pose table.
 * Replaces the per-sample slicing, padding, stride mask and flip of H36mSequenceGenerator
 * (common/dataset/uplifiting_dataset.py:322-407) plus the harness's `x * stride_mask` (eval.py:67, train.py:474).
 *   poses_dev (F, J, C) f32: all videos back to back (C = 2 for 2D keypoints, 3 for 3D ground truth);
 *   video_start_dev (V) i64 first row of each video, video_len_dev (V) i32;
 *   windows_dev (B) uu3d_window: video, centre frame, sampling stride, ABSOLUTE mask stride, mask shift (centre frame
 *   for globally aligned masks, rand_shift * stride in training, 0 otherwise), flip flag;
 *   flip_order_dev (J) i32 or NULL (AUGM_FLIP_KEYPOINT_ORDER); pad_edge: 1 = "copy" padding, 0 = zeros.
 *   out_dev (B, N, J, C); stride_mask_dev (B, N) u8 (1 = real input); pad_mask_dev (B, N) u8 or NULL (1 = frame exists).
 */
typedef struct uu3d_window { int32_t video, center, stride, mask_stride, mask_shift, flip; } uu3d_window;
int uu3d_gather_windows(const float* poses_dev, const int64_t* video_start_dev, const int32_t* video_len_dev,
                        const uu3d_window* windows_dev, const int32_t* flip_order_dev,
                        int32_t batch, int32_t num_frames, int32_t num_keypoints, int32_t channels,
                        int32_t pad_edge, int32_t zero_masked,
                        float* out_dev, uint8_t* stride_mask_dev, uint8_t* pad_mask_dev, void* stream);

/*
 * YOUR OWN 2D TRACKS (predict.predict_tracks): the front and the back of the chain pose table -> uu3d_gather_windows -> forward, for keypoint
 * tracks that come from the caller's detector instead of a dataset.  One launch per call for all tracks, every output element written by one
 * thread (no atomics: bitwise repeatable), 16-byte stores; stream-ordered, all buffers are the caller's.
 *
 *   uu3d_normalize_tracks: pixel coordinates -> the model's normalised screen coordinates in the pose table table_dev (rows, J, 2) f32,
 *   16-byte aligned: x / w * 2 - 1, y / w * 2 - h / w (common/dataset/camera.py:15-20) in numpy's float32 / float64 operation order, so
 *   the result equals h36m.normalize_screen_coordinates on float32 input bit for bit.  row_track_dev (rows) i32: the track of every table
 *   row; resolution_dev (num_tracks, 2) f64 = (w, h) per track, or NULL: coordinates are taken as they are.
 *     key_stride == 0: src_dev holds the rows of the table (src_rows == rows; src_dev == table_dev converts in place);
 *     key_stride > 0 (keyframes only): src_dev (src_rows, J, 2), 8-byte aligned and not the table, holds frames 0, key_stride, 2 key_stride, ...
 *     of every track back to back; track t starts at row track_start_dev[t] of the table and at row src_start_dev[t] of src_dev (i64 each).
 *     The same launch scatters the keyframes to their table rows and writes zeros to every other row.
 *   A track id or source row out of range yields NaN rows, never a read out of bounds.
 *
 *   uu3d_assemble_tracks: the central predictions of the forwarded windows as the pipeline leaves them -- plain_dev (num_windows, J, 3) and,
 *   with flip test-time augmentation, flipped_dev (num_windows, J, 3) of the mirrored windows with flip_order_dev (J) i32 (both NULL: no flip)
 *   -- to the dense out_dev (num_frames, J, 3) f32, 16-byte aligned: un-flip (x negated, joints permuted) and average in float32 as
 *   eval.py:163-166, then per frame f the plan (left_dev, right_dev (num_frames) i32 rows of the prediction arrays, weight_dev f64) of
 *   evaluation.keyframe_plan: pred[left] where left == right, else pred[left] * (1 - weight) + pred[right] * weight in float64 with every
 *   operation rounded, stored as float32 -- evaluation.interpolate_between_keyframes on float32 predictions bit for bit.  root_index >= 0:
 *   that joint of the frame is subtracted in float32 afterwards (it comes out exactly 0); -1: absolute predictions.  A plan row outside
 *   [0, num_windows) yields NaN.
 *
 *   uu3d_assemble_tracks_cubic (predict_tracks(interpolation="cubic")): the same launch with a C1 cubic between the predicted frames in
 *   place of the line -- the plan of evaluation.keyframe_plan_cubic: before_dev / after_dev (num_frames) i32 name the predicted frame in front
 *   of left and the one behind right, in the same track, or -1 where there is none (and wherever left == right).  pred[left] where
 *   left == right: the bits of uu3d_assemble_tracks.  Else, with P0..P3 = pred[before], pred[left], pred[right], pred[after] and t = weight,
 *   all in float64 with every operation rounded and no fused multiply-add, in this order:
 *     m1 = (P2 - P0) * 0.5 (before == -1: P2 - P1);  m2 = (P3 - P1) * 0.5 (after == -1: P2 - P1);  t2 = t * t;  t3 = t2 * t;
 *     h01 = 3.0 * t2 - 2.0 * t3;  h00 = 1.0 - h01;  h11 = t3 - t2;  h10 = (h11 - t2) + t;
 *     value = ((h00 * P1 + h01 * P2) + h10 * m1) + h11 * m2, stored as float32
 *   -- the Hermite segment with Catmull-Rom tangents over equally spaced predicted frames; evaluation.interpolate_cubic_host bit for bit.
 *   The un-flip, the average and root_index are those of uu3d_assemble_tracks.  left or right outside [0, num_windows), or before / after
 *   outside [-1, num_windows) where left != right, yields NaN, never a read out of bounds.  Argument checks as uu3d_assemble_tracks.
 */
int uu3d_normalize_tracks(const float* src_dev, int64_t src_rows, float* table_dev, int64_t rows, int32_t num_keypoints,
                          const int32_t* row_track_dev, int32_t num_tracks, const double* resolution_dev,
                          const int64_t* track_start_dev, const int64_t* src_start_dev, int32_t key_stride, void* stream);
int uu3d_assemble_tracks(const float* plain_dev, const float* flipped_dev, int64_t num_windows, const int32_t* flip_order_dev,
                         const int32_t* left_dev, const int32_t* right_dev, const double* weight_dev, int64_t num_frames,
                         int32_t num_keypoints, int32_t root_index, float* out_dev, void* stream);
int uu3d_assemble_tracks_cubic(const float* plain_dev, const float* flipped_dev, int64_t num_windows, const int32_t* flip_order_dev,
                               const int32_t* before_dev, const int32_t* left_dev, const int32_t* right_dev, const int32_t* after_dev,
                               const double* weight_dev, int64_t num_frames, int32_t num_keypoints, int32_t root_index, float* out_dev,
                               void* stream);

/*
 * World -> camera coordinates -> 2D projection with the Human3.6M camera model, one camera per window: replaces
 * tf_world_to_cam_and_2d (common/dataset/uplifiting_dataset.py:669-761), the on-the-fly AMASS projection of training.
 *   world_dev (B, N, J, 3) f32; cams_dev (B, 18) f32 = quaternion wxyz | translation | 11 intrinsics (res, focal,
 *   centre, 3 radial, 2 tangential coefficients at [7..18) as the reference stores them);
 *   cam3d_dev (B, N, J, 3) or NULL; kp2d_dev (B, N, J, 2) or NULL.
 */
int uu3d_world_to_cam_2d(const float* world_dev, const float* cams_dev, int32_t batch, int32_t num_frames, int32_t num_keypoints,
                         float* cam3d_dev, float* kp2d_dev, void* stream);

/*
 * The schedule of a forward: what its launch shapes are chosen for.  Below 1024 token rows (B * N) the results are bit-identical either
 * way (the same products per element, computed by other workgroups); from 1024 rows on the throughput schedule takes the temporal chain
 * (csrc/uu3d_tchain16.h, rounds 5-6: one launch per temporal block for every row-local stage, residual stream and relu(fc1) on chip -- other summation orders and LayerNorm's affine part
 * folded into the next layer's weights: within 3e-5 of the latency schedule (measured 4e-6), same 1e-4 bar against the oracle; deterministic run
 * to run; return_attention keeps the round-4 launches.  UU3D_TCHAIN=0 in the environment of uu3d_create: never; UU3D_TCHAIN_MIN_TILES=n: from n
 * row tiles of 128 tokens on).
 *   UU3D_SCHEDULE_LATENCY: one batch at a time -- every launch spreads over as many CUs as pays for ITS duration;
 *   UU3D_SCHEDULE_THROUGHPUT: several independent batches in flight on different streams (pipeline.ForwardPipeline) -- the chip is
 *     shared between forwards, so a launch is shaped for the fewest CU-microseconds instead: the attention projection runs as 71
 *     workgroups x 12 column chunks instead of 213 x 4 (27 instead of 16 us alone, +2.4 % sequences/s with four batches in flight;
 *     DESIGN.md section 5).
 * uu3d_forward_ex takes it as an ARGUMENT of the call (round 4): it is a property of the enqueued / captured forward, not of the
 * model, so a model(...) call on one thread and a pipeline on another never see each other's choice.  attention_out as in
 * uu3d_forward_attention (NULL: none).  uu3d_forward / uu3d_forward_attention = uu3d_forward_ex with the model's DEFAULT schedule,
 * which uu3d_set_schedule changes (UU3D_SCHEDULE_LATENCY unless set; kept for callers that cannot pass the argument).
 */
#define UU3D_SCHEDULE_LATENCY 0
#define UU3D_SCHEDULE_THROUGHPUT 1
/*
 * RANGE CONTRACT of precision f16x3 (round 5).  The reference computes in float32 end to end; the f16x3 products split
 * every operand into two f16 planes, so an ACTIVATION of magnitude >= 65504 (LayerNorm outputs, q | k | v, attention context, ReLU(fc1),
 * the residual stream in front of the full-sequence head, the spatial stack's operands) becomes Inf in its hi plane and the sequence it
 * belongs to comes out NaN.  (Weights are checked when they are committed: uu3d_commit_weights fails with UU3D_ERR_RANGE.)  Keras-default
 * and trained weights keep activations at O(10); nothing in the format guarantees it.  Therefore:
 *   - every f16x3 forward ends with a check of its outputs (one small launch): non-finite values set a STICKY device word of the model;
 *   - uu3d_range_status(model, stream, &flag) synchronises `stream`, returns the word (flag 0 / 1; may be NULL) and clears it; its return
 *     value is UU3D_ERR_RANGE when the word was set, UU3D_OK otherwise -- the forward itself stays asynchronous and keeps returning
 *     launch errors only;
 *   - OR-ing UU3D_SCHEDULE_EXACT_F32 into `schedule` runs THIS call on the exact-f32 kernels whatever the handle's precision (f32-input
 *     MFMA: the whole float32 range; every sequence length a compiled-dims handle takes, up to 416 tokens -- above 128 the attention is
 *     the training step's tiled exact-f32 forward without its statistics, csrc/uu3d_attn_long.h): the fallback for a batch that
 *     overflowed.  Handles with generic dims have no such path (UU3D_ERR_UNSUPPORTED).  The per-CALL bit reaches 416 tokens; the
 *     handle-wide uu3d_create(precision = f32) is still refused above 128.
 * The Python model(...) does all three: it checks after the call and repeats an overflowed batch in exact f32 (or raises Uu3dRangeError
 * where that path does not exist: generic dims); pipelines check once, at ForwardPipeline.check_range() / the end of run_eval, or run
 * every forward under the bit (ForwardPipeline(exact_f32=True), predict_windows(exact_f32=True)): nothing to check then.
 */
#define UU3D_SCHEDULE_EXACT_F32 0x100
int uu3d_range_status(uu3d_model* model, void* stream, int32_t* out_flag);
int uu3d_forward_ex(uu3d_model* model, const float* kp2d_dev, const uint8_t* stride_mask_dev, int32_t batch, float* full_out_dev,
                    float* central_out_dev, float* const* attention_out, void* workspace_dev, size_t workspace_bytes,
                    int32_t schedule, void* stream);
int uu3d_set_schedule(uu3d_model* model, int32_t schedule);

/*
 * FRAMES FORM of the forward (evaluation over overlapping windows; live tracks).  The spatial stack and spatial_to_temporal_fc work on
 * one frame at a time: a frame's d_t features do not depend on the window it sits in, only the token blend and the temporal PE that
 * follow do.  So features are computed once per frame and every window reads them from a table.
 *
 * Handles with generic dims (anything but J = 17, d_s = 32, d_t = 384, 8 heads, MLP ratio 2) have the form under ONE rule: the spatial
 * stack of a frame runs in one workgroup (csrc/uu3d_spatial_generic.h), so the frame has to fit a workgroup's 160 KiB of LDS --
 *     4 * (2 J d_s + J (max(3 d_s, h_s) + 1) + hg J (J | 1)) <= 163840 bytes,   hg = clamp(2048 / (J (J | 1)), 1, heads)  (integer division)
 * (the residual stream, a LayerNorm / attention-output buffer, q | k | v or the hidden layer, the logits of hg heads).  Every J <= 32 with
 * d_s <= 128 and MLP ratio <= 4 fits; J = 128 with d_s = 128 does not.  A handle whose frame does not fit HAS NO FRAMES FORM:
 * uu3d_frame_features_bytes returns 0, and uu3d_frame_features, uu3d_forward_frames_ex and every uu3d_stream_* entry return
 * UU3D_ERR_UNSUPPORTED before anything is launched, with the needed and the available bytes in uu3d_last_error.  Its window forward
 * (uu3d_forward_ex) is unaffected.  There is no second path.  On a generic handle uu3d_frame_features is that kernel (exact f32, weights
 * read from the handle's master buffer) followed by spatial_to_temporal_fc as the generic GEMM; uu3d_forward_frames_ex is the generic
 * forward from its temporal stack on, under the same rules (workspace uu3d_workspace_bytes(batch)); UU3D_SCHEDULE_EXACT_F32 stays refused.
 * CAPTURED GRAPHS AND TRAINING on a generic handle: the operand packs of the generic GEMMs (spatial_to_temporal_fc, the temporal and strided
 * blocks, the heads) are shared with the training step, and the test "are the packs the handle's, else repack" runs on the HOST when a call
 * is enqueued -- so it is part of a capture, not of its replays.  A training step on the same handle (uu3d_train_forward_backward with a
 * Trainer's own parameter buffer) repacks from that buffer; a graph captured before it (a pipeline's, a live session's tick) then replays on
 * the Trainer's packs without an error.  Direct calls are safe (they repack).  After training on a handle, capture again: build a new
 * pipeline / StreamSession.  (As for the window form of a generic handle in a captured pipeline.)
 *
 *   uu3d_frame_features(model, frames_dev (F, J, 2) f32, F, features_dev (F, d_t) f32, workspace, bytes, schedule, stream)
 *       the spatial stack and spatial_to_temporal_fc with its bias on F frames -- no blend, no PE.  The kernel choice of the forward
 *       (f16x3 / exact-f32 spatial kernel by frame count, f16 operand planes of the s2t GEMM); UU3D_SCHEDULE_EXACT_F32 in `schedule` runs
 *       the exact-f32 kernels.  In f16x3 non-finite features set the model's sticky range word (RANGE CONTRACT above).
 *       The workspace (256-byte aligned) holds uu3d_frame_features_bytes(model, F) bytes.
 *   uu3d_gather_window_frames(video_start_dev, video_len_dev, windows_dev (B) uu3d_window, B, N, pad_edge, zero_masked, frame_base, zero_row,
 *                             rows_dev (B, N) int32, stride_mask_dev (B, N), pad_mask_dev (B, N) or NULL, stream)
 *       the windows of uu3d_gather_windows with exactly its frame and mask rules (one device helper states them for both kernels), but
 *       a feature-table row per token instead of coordinates: -1 where zero_masked is set and the stride mask drops the token (the forward
 *       writes the masked token), zero_row where zero padding reads no frame (the caller stores the features of an all-zero frame there),
 *       else video_start[video] + source frame (the edge frame for copy padding), + frame_base for a flipped window (the flipped half of
 *       the table: features of frames flipped like the window).  video_start may be shifted so that a table covers part of a pose table.
 *   uu3d_forward_frames_ex(model, features_dev (R, d_t) f32, R, rows_dev (B, N) int32, stride_mask_dev, B, full_out, central_out,
 *                          attention_out, workspace, bytes, schedule, stream)
 *       the forward of uu3d_forward_ex from its stage 3 on (temporal chain under the throughput schedule, attention_out, the range check,
 *       UU3D_SCHEDULE_EXACT_F32 -- one shared body), its input x = (masked ? token : features[rows]) + temporal PE written by one kernel.
 *       features_dev 16-byte aligned; a real token whose row is outside [0, R) comes out NaN and trips the range check.  Workspace:
 *       uu3d_workspace_bytes(batch).  Capturable into a hipGraph like uu3d_forward_ex.
 * Results agree with uu3d_forward_ex on the same windows to ~3e-5 (the s2t GEMM sums in another split-K order at another row count).
 */
size_t uu3d_frame_features_bytes(const uu3d_model* model, int32_t frames);
int uu3d_frame_features(uu3d_model* model, const float* frames_dev, int32_t frames, float* features_dev, void* workspace_dev,
                        size_t workspace_bytes, int32_t schedule, void* stream);
int uu3d_gather_window_frames(const int64_t* video_start_dev, const int32_t* video_len_dev, const uu3d_window* windows_dev,
                              int32_t batch, int32_t num_frames, int32_t pad_edge, int32_t zero_masked, int64_t frame_base, int64_t zero_row,
                              int32_t* rows_dev, uint8_t* stride_mask_dev, uint8_t* pad_mask_dev, void* stream);
int uu3d_forward_frames_ex(uu3d_model* model, const float* features_dev, int64_t num_rows, const int32_t* rows_dev,
                           const uint8_t* stride_mask_dev, int32_t batch, float* full_out_dev, float* central_out_dev,
                           float* const* attention_out, void* workspace_dev, size_t workspace_bytes, int32_t schedule, void* stream);

/*
 * LIVE TRACKS (stream.StreamSession; every handle that has the FRAMES FORM above -- a generic handle whose frame does not fit the LDS
 * returns UU3D_ERR_UNSUPPORTED; the root, bone and association stages keep their own limit of 64 joints).  `slots` tracks grow by
 * one frame of 2D keypoints per tick; after the push that made frame t the newest of a slot, the pose of frame c = t - lookahead comes out
 * when c >= 0 and c % pred_stride == 0 (the windows eval.needed_windows keeps), computed from the window uu3d_gather_window_frames writes
 * for a video of t + 1 frames centred on c with a globally aligned stride mask: frames that do not exist yet are padded as the end of a
 * video is.  Per tick, on one stream, in this order:
 *
 *   uu3d_stream_stage(model, cfg, kp_dev (slots, J, 2) f32, resolution_dev (slots, 2) f64 (w, h) or NULL, active_dev (slots) u8,
 *                     flip_order_dev (J) i32 (NULL without flip), frames_out_dev (halves * slots, J, 2) f32, stream)
 *       the pushed frames in normalised screen coordinates (the bits of uu3d_normalize_tracks: one device helper) and, with flip, behind
 *       them their mirrored copies (x negated, joints permuted); halves = flip ? 2 : 1.  An inactive slot's frames are zeros.
 *   uu3d_frame_features on frames_out_dev (halves * slots frames) -> features_dev (halves * slots, d_t)
 *   uu3d_stream_commit(model, cfg, state_dev, features_dev, active_dev, rows_dev (halves * slots, N) i32, stride_mask_dev (halves * slots, N)
 *                      u8, fresh_dev (slots) u8, stream)
 *       one launch, one workgroup per slot.  An active slot's frame counter advances (new frame index f = the old count); the features are
 *       stored as the slot's edge row when f % seq_stride == 0 and in ring place (f / mask_stride) % ring_capacity when f % mask_stride == 0.
 *       Then the window of this tick as rows of the state block's feature table: -1 for a token the stride mask drops (the zero row for a
 *       model without strided input), the zero row where zero padding reads no frame, the ring place of a keyframe, the edge row for copy
 *       padding behind the newest frame (that frame is a multiple of seq_stride, not necessarily of mask_stride), the flipped half of the
 *       table for the mirrored windows.  fresh = 1 where a pose comes out at this tick; any other slot gets an all-masked window (finite,
 *       discarded).  The frame and mask rules are the device helper uu3d_gather_windows and uu3d_gather_window_frames share.
 *   uu3d_forward_frames_ex with features_dev = state_dev + table_offset, num_rows = table_rows, batch = halves * slots
 *   uu3d_stream_emit(model, cfg, state_dev, central_dev (halves * slots, J, 3), flip_order_dev, fresh_dev, out_dev (slots, J, 3) f32, stream)
 *       un-flip and average in float32 as uu3d_assemble_tracks (one device helper), root_index >= 0: that joint subtracted.  A fresh slot's
 *       pose goes to out_dev and to the held poses of the state block; any other slot's out_dev row is its held pose.
 *
 *   uu3d_stream_reset(model, cfg, state_dev, slot_mask_dev (slots) u8 or NULL = every slot, stream): those slots start a new track
 *   (zero frames, held pose 0).
 *
 * The state block (256-byte aligned, uu3d_stream_state_bytes; all zeros = every slot empty, except that the caller stores the features of
 * an all-zero frame in the table's row zero_row) is laid out by uu3d_stream_state_layout: frame counters (slots) i32 at frames_offset, held
 * poses (slots, J, 3) f32 at held_offset, the feature table (table_rows, d_t) f32 at table_offset = per half and slot ring_capacity ring
 * rows and one edge row, then the zero row.  ring_capacity = (lookahead + (N / 2) * seq_stride) / mask_stride + 1 covers every keyframe a
 * window reaches, so no ring place a window reads has been overwritten.  0 <= lookahead <= (N / 2) * seq_stride; mask_stride a multiple of
 * seq_stride.  No atomics, one writer per output element, 16-byte stores where rows allow; every launch has the same arguments at every
 * tick (the counters live on the device), so the five steps replay from ONE captured hipGraph, a linear chain.
 */
typedef struct uu3d_stream_config {
    int32_t slots, seq_stride, mask_stride, pred_stride, lookahead, flip, pad_edge /* 1 = "copy" padding */, root_index /* < 0: absolute */;
} uu3d_stream_config;
typedef struct uu3d_stream_layout { int64_t ring_capacity, table_rows, zero_row, frames_offset, held_offset, table_offset, bytes; } uu3d_stream_layout;
size_t uu3d_stream_state_bytes(const uu3d_model* model, const uu3d_stream_config* cfg);
int uu3d_stream_state_layout(const uu3d_model* model, const uu3d_stream_config* cfg, uu3d_stream_layout* out);
int uu3d_stream_stage(uu3d_model* model, const uu3d_stream_config* cfg, const float* kp_dev, const double* resolution_dev,
                      const uint8_t* active_dev, const int32_t* flip_order_dev, float* frames_out_dev, void* stream);
int uu3d_stream_commit(uu3d_model* model, const uu3d_stream_config* cfg, void* state_dev, const float* features_dev,
                       const uint8_t* active_dev, int32_t* rows_dev, uint8_t* stride_mask_dev, uint8_t* fresh_dev, void* stream);
int uu3d_stream_emit(uu3d_model* model, const uu3d_stream_config* cfg, void* state_dev, const float* central_dev,
                     const int32_t* flip_order_dev, const uint8_t* fresh_dev, float* out_dev, void* stream);
int uu3d_stream_reset(uu3d_model* model, const uu3d_stream_config* cfg, void* state_dev, const uint8_t* slot_mask_dev, void* stream);

/*
 * MISSED DETECTIONS (predict.predict_tracks(valid=...), stream.StreamSession(missed_detections=True)): a frame of a track is VALID or
 * MISSING (the detector found nobody: occlusion, blur, the person left the image).  A missing frame is never an observation: its token
 * is the learned strided-input token, hidden as a key in the first temporal block(s), exactly like a frame the stride mask drops.
 * THE RULE, stated once on the device (window_token_real next to window_frame, csrc/uu3d_misc.h) and shared by every kernel below: token n
 * of a window reads source frame src (its own frame, or under copy padding the nearest sampled in-range frame); with a validity table
 * (one byte per frame, 0 = missing) its stride-mask bit becomes
 *     sm' = sm && (!have || valid[video_start + src])
 * Zero padding (!have: no frame is read) is untouched; a copy-padded token whose source frame is missing is masked; a flipped window uses
 * the entry of its plain twin.  Everything downstream follows from the bit as before (zero_masked, rows = -1, the key mask).  Missing
 * frames are written to the pose table as ZEROS, so their features are finite and nothing non-finite can reach the network or the range
 * word.  Needs a model with strided input (the masked token); the stream calls return UU3D_ERR_UNSUPPORTED otherwise.
 * Every function above is its _valid form with the validity pointers NULL: one kernel source, a NULL check.  No atomics, one writer per
 * output element.
 *
 *   uu3d_normalize_tracks_valid = uu3d_normalize_tracks + valid_in_dev (src_rows) u8 or NULL, valid_out_dev (rows) u8.  A source frame is
 *       valid iff valid_in (when given) is non-zero AND all 2 J of its coordinates are finite; valid_out[row] holds that flag and the
 *       table row of a missing frame is all zeros.  key_stride > 0: rows that are not given keep valid_out = 1 and zeros (they behave as
 *       before; the copy-padding exception of keyframes_only is unchanged).  Two launches on the stream: the flags (one wave per frame,
 *       reading src only), then uu3d_normalize_tracks' own kernel reading them -- so the in-place form (src == table) stays legal.
 *   uu3d_gather_windows_valid / uu3d_gather_window_frames_valid = the two gathers + frame_valid_dev (F) u8 indexed like the pose table
 *       (video_start[video] + frame; with shifted video starts pass the pointer shifted back), NULL = the old function.  pad_mask is
 *       unchanged: it says whether a frame exists, not whether it is valid.
 *   uu3d_stream_stage_valid = uu3d_stream_stage + valid_in_dev (slots) u8 or NULL, valid_out_dev (slots) u8:
 *       valid_out[slot] = active && valid_in && all coordinates finite; a missing slot's staged frames, both halves, are zeros.
 *   uu3d_stream_commit_valid = uu3d_stream_commit + valid_dev (slots) u8 (the stage's valid_out) and valid_state_dev: a caller-allocated
 *       block of uu3d_stream_valid_bytes(model, cfg) bytes = (slots, ring_capacity + 1) u8, one byte per ring place and one for the edge
 *       row, the same for both halves, filed where the features are filed.  All zeros is a legal initial state (a window never reads a
 *       place its counter has not reached), so uu3d_stream_reset needs no change.  A missing frame still advances the slot's counter --
 *       time passes; that is the difference from active = 0.  The window of the tick applies the rule with the byte of the ring place or
 *       edge row it points to; fresh is unchanged.  A tick stays a linear chain of five launches with unchanging arguments.
 */
int uu3d_normalize_tracks_valid(const float* src_dev, int64_t src_rows, float* table_dev, int64_t rows, int32_t num_keypoints,
                                const int32_t* row_track_dev, int32_t num_tracks, const double* resolution_dev,
                                const int64_t* track_start_dev, const int64_t* src_start_dev, int32_t key_stride,
                                const uint8_t* valid_in_dev, uint8_t* valid_out_dev, void* stream);
int uu3d_gather_windows_valid(const float* poses_dev, const int64_t* video_start_dev, const int32_t* video_len_dev,
                              const uu3d_window* windows_dev, const int32_t* flip_order_dev,
                              int32_t batch, int32_t num_frames, int32_t num_keypoints, int32_t channels,
                              int32_t pad_edge, int32_t zero_masked, const uint8_t* frame_valid_dev,
                              float* out_dev, uint8_t* stride_mask_dev, uint8_t* pad_mask_dev, void* stream);
int uu3d_gather_window_frames_valid(const int64_t* video_start_dev, const int32_t* video_len_dev, const uu3d_window* windows_dev,
                                    int32_t batch, int32_t num_frames, int32_t pad_edge, int32_t zero_masked, int64_t frame_base,
                                    int64_t zero_row, const uint8_t* frame_valid_dev, int32_t* rows_dev, uint8_t* stride_mask_dev,
                                    uint8_t* pad_mask_dev, void* stream);
size_t uu3d_stream_valid_bytes(const uu3d_model* model, const uu3d_stream_config* cfg);
int uu3d_stream_stage_valid(uu3d_model* model, const uu3d_stream_config* cfg, const float* kp_dev, const double* resolution_dev,
                            const uint8_t* active_dev, const int32_t* flip_order_dev, const uint8_t* valid_in_dev,
                            uint8_t* valid_out_dev, float* frames_out_dev, void* stream);
int uu3d_stream_commit_valid(uu3d_model* model, const uu3d_stream_config* cfg, void* state_dev, const float* features_dev,
                             const uint8_t* active_dev, const uint8_t* valid_dev, void* valid_state_dev, int32_t* rows_dev,
                             uint8_t* stride_mask_dev, uint8_t* fresh_dev, void* stream);

/*
 * PER-JOINT MISSED DETECTIONS (predict.predict_tracks(valid=..., repair_joints=G)): a detector rarely loses a whole frame; it loses a wrist
 * or an ankle for a few frames.  uu3d_repair_joints fills such joints on the device, in front of uu3d_normalize_tracks_valid or
 * uu3d_resample_tracks, which take its output as their src_dev and its frame flags as their valid_in_dev.
 * src_dev (rows, J, 2) f32, 8-byte aligned: the frames as given (raw coordinates; source frames, or the given keyframes), all tracks back to
 * back; track t is rows [track_start_dev[t], track_start_dev[t + 1]), track_start_dev (num_tracks + 1) i64.  Nothing crosses a track boundary.
 * THE RULE.  Joint j of frame t is OBSERVED, a(t, j), iff its byte of joint_flags_dev (rows, J) u8 is non-zero (NULL: no flags given) AND
 * both of its coordinates are finite.  max_gap = G >= 1 is the longest run of consecutive unobserved frames of one joint that is filled.
 * For an unobserved (t, j) let l be the largest t' < t with a(t', j) and r the smallest t' > t with a(t', j), inside the track:
 *     l and r exist and r - l - 1 <= G:  per coordinate (float)((double)src[l] * (1.0 - w) + (double)src[r] * w), w = (double)(t - l) /
 *         (double)(r - l): two products and one sum in float64, each rounded, no fused multiply-add, rounded once to float32 -- the
 *         expression of uu3d_resample_tracks, so a numpy restatement (predict.repair_joints_host) gives the same bits;
 *     only r exists (before the joint's first observation) and r - t <= G:  the bits of src[r, j];
 *     only l exists (behind its last observation) and t - l <= G:  the bits of src[l, j];
 *     otherwise the joint is UNREPAIRABLE.
 * A frame is a real observation iff at least one of its joints is observed and every other one was filled.  A frame without an observed
 * joint is never filled and a frame with an unrepairable joint is missing too: both stay MISSING in the sense of MISSED DETECTIONS above.
 * Outputs, each element with one writer, no atomics, bitwise repeatable:
 *     out_dev (rows, J, 2) f32, 16-byte aligned, never src_dev (UU3D_ERR_INVALID_ARGUMENT): observed joints keep their bits, filled joints
 *         hold the value above, everything else is zeros -- nothing non-finite leaves the call.  src_dev is only read.
 *     frame_valid_dev (rows) u8: 1 = a real observation.        joint_state_dev (rows, J) u8, 2-byte aligned: 1 observed, 2 filled, 0 neither.
 * l and r come from two segmented scans along the frames of every track and joint, so the cost does not depend on G.  They pass through
 * scratch_dev, 4-byte aligned, of at least uu3d_repair_joints_scratch_bytes bytes = two (rows, J) i32 planes; 0 for arguments out of range:
 * rows < 2^31, num_tracks * J < 2^31.  A row that track_start_dev does not cover gets NaN and state 0 for its unobserved joints, never a read
 * out of bounds.  Three launches on the stream, no host synchronisation.
 */
size_t uu3d_repair_joints_scratch_bytes(int64_t rows, int32_t num_keypoints);
int uu3d_repair_joints(const float* src_dev, int64_t rows, int32_t num_keypoints, const uint8_t* joint_flags_dev,
                       const int64_t* track_start_dev, int32_t num_tracks, int32_t max_gap, float* out_dev, uint8_t* frame_valid_dev,
                       uint8_t* joint_state_dev, void* scratch_dev, size_t scratch_bytes, void* stream);

/*
 * ANY SKELETON (predict.predict_tracks(keypoints=M), stream.StreamSession(keypoints=M)): no detector emits the model's own joint layout
 * (the shipped configs: Human3.6M's 17 joints).  uu3d_map_keypoints turns the joints a detector does emit -- `inputs` of them, K_in -- into
 * the J = num_keypoints joints of the handle, on the device, in front of EVERYTHING else that looks at a track: uu3d_repair_joints,
 * uu3d_normalize_tracks(_valid), uu3d_resample_tracks, the stage of a live tick.  It runs on the raw coordinates as given, pixels or
 * normalised: the map is affine (every joint's weights sum to 1), so it commutes, mathematically, with the screen normalisation.
 * THE RULE.  Per model joint j an ordered list of 1 <= n_j <= 8 distinct sources src[j][k] with float64 weights w[j][k], finite, non-zero,
 * summing to 1 within 1e-12 (negative weights allowed).  For every frame and model joint, per coordinate,
 *     out[j] = (float)(w[j][0] * (double)in[src[j][0]] + w[j][1] * (double)in[src[j][1]] + ...)
 * in float64, summed left to right in the listed order, every product and sum rounded, no fused multiply-add, rounded once to float32 -- the
 * discipline of uu3d_resample_tracks' expression, so a numpy restatement (predict.map_keypoints_host) gives the same bits.  A NaN result is
 * stored as the quiet NaN 0x7fc00000 (which NaN an invalid sum makes is not the same on every processor).  A joint with one source of
 * weight 1.0 has that source's bits; only listed sources are read, so an unlisted NaN never reaches a joint.
 * FLAGS.  flags_in_dev (frames, inputs) u8 and flags_out_dev (frames, J) u8, both or neither (UU3D_ERR_INVALID_ARGUMENT).  Neither: the
 * expression alone; a NaN source gives a NaN joint.  Both: a source is OBSERVED when its byte is non-zero and both of its coordinates are
 * finite; a model joint is observed iff every one of its sources is; flags_out holds that (1 / 0) and an unobserved joint's coordinates
 * are written as zeros -- what uu3d_repair_joints and uu3d_stream_repair_stage take as joint_flags_dev.
 *
 *   uu3d_keypoint_map_bytes(inputs, joints): the size of the device-resident table, 0 for arguments out of range.  Fixed stride 8, three
 *       planes back to back: w (joints, 8) f64 at 0, src (joints, 8) i32 at 64 joints (-1 for an unused entry), n (joints) i32 at 96 joints.
 *   uu3d_keypoint_map_pack(inputs, joints, counts (joints) i32, sources (joints, 8) i32, weights (joints, 8) f64, out_host, out_bytes): HOST
 *       memory in, HOST memory out (8-byte aligned): checks the rule's terms and that every listed source lies in [0, inputs)
 *       (UU3D_ERR_INVALID_ARGUMENT otherwise; entries k >= counts[j] are ignored) and writes the table.  The caller packs once, uploads
 *       once and keeps the block; no call does host work per frame.  The kernel does NOT re-check the table.
 *   uu3d_map_keypoints(model, map_dev, inputs, src_dev (frames, inputs, 2) f32, flags_in_dev or NULL, frames, out_dev (frames, J, 2) f32,
 *       flags_out_dev or NULL, stream): one launch, one lane per (frame, model joint), one 8-byte store of the coordinate pair; every
 *       element has one writer, no atomics: bitwise repeatable.  map_dev, src_dev and out_dev 8-byte aligned; src_dev is only read and is
 *       never out_dev.  frames == 0 is a no-op that returns UU3D_OK.  inputs < 1: UU3D_ERR_INVALID_ARGUMENT.  The arguments are the same
 *       at every tick of a live session, so the launch is the first step of its captured graph.
 */
size_t uu3d_keypoint_map_bytes(int32_t inputs, int32_t joints);
int uu3d_keypoint_map_pack(int32_t inputs, int32_t joints, const int32_t* counts, const int32_t* sources, const double* weights,
                           void* out_host, size_t out_bytes);
int uu3d_map_keypoints(uu3d_model* model, const void* map_dev, int32_t inputs, const float* src_dev, const uint8_t* flags_in_dev,
                       int64_t frames, float* out_dev, uint8_t* flags_out_dev, void* stream);

/*
 * PER-FRAME DETECTIONS (predict.associate_detections / predict_detections, stream.StreamSession(detections=D)): a multi-person detector
 * emits a list of people per frame, in arbitrary order, with people entering, leaving and being missed.  These calls turn the lists into
 * tracks (whole videos) and into the slots of a live session (one frame per tick) on the device, by ONE rule; predict.associate_host is
 * the same rule in numpy and gives the same results bit for bit.  The rule is greedy and has no motion model and no Hungarian step: it is
 * the simplest rule that can be stated exactly.  Capacities: slots S, detections D and joints K each <= 64 (UU3D_ERR_UNSUPPORTED beyond).
 * THE RULE.  State per slot: alive, track_id (-1: free), age (consecutive frames without a match), a reference pose ref (K, 2) f32 with
 * ref_seen (K): the last observed position of each joint since the slot's birth.  Global: next_id, dropped.  Per frame: dets (D, K, 2)
 * f32, count, optional flags (D) or (D, K) u8.  A joint of a detection is OBSERVED when its flag is non-zero and both coordinates are
 * finite; detection d is a CANDIDATE when d < count (count is clamped into [0, D]), its frame flag is set and it has >= min_common observed
 * joints.  Unobserved joints never enter any arithmetic.
 *   1. cost(alive slot s, candidate d): C = joints with ref_seen[s] that are observed in d; |C| < min_common: not allowed.  d2 = the sum
 *      over C in ascending j of dx * dx + dy * dy, dx = (double)det.x - (double)ref.x, accumulated left to right in float64, every product
 *      and sum rounded, no fused multiply-add.  scale2 = w * w + h * h of the bounding box of the slot's seen reference joints, in
 *      float64; scale2 == 0: not allowed.  cost = d2 / ((double)|C| * scale2), one IEEE division; allowed iff cost <= max_dist * max_dist.
 *   2. greedy: repeatedly the allowed pair of smallest cost among unmatched slots and unmatched candidates, ties to the smaller s, then
 *      the smaller d, until no allowed pair is left.
 *   3. a matched slot: age = 0; ref takes the bits of every joint observed in d and ref_seen = 1 there; d is its frame of this tick.
 *   4. an unmatched alive slot: age += 1; age > max_age: it dies (alive = 0, track_id = -1); else its frame of this tick is MISSING.
 *   5. unmatched candidates in ascending d take the lowest free slot each (one that died in step 4 included): BORN -- track_id =
 *      next_id++, age = 0, ref / ref_seen from the detection, which is its first frame.  No free slot: dropped += 1, assignment -1.
 *   6. per frame: assignment (D) i32 (slot or -1), track_ids (S) i32 (-1: free), born (S) u8, alive (S) u8.
 * Causal: frame t's result depends on frames <= t only.
 *
 *   uu3d_associate_state_bytes(slots, keypoints): the size of the state block (256-byte aligned), 0 for arguments out of range.
 *   uu3d_associate_reset(params, state_dev, slot_mask_dev (S) u8 or NULL, stream): the chosen slots become free (their tracks end); NULL =
 *       every slot, and next_id = dropped = 0.  A fresh block must be reset once (a free slot's track_id is -1, not 0).
 *   uu3d_associate_detections(params, dets_dev (frames, D, K, 2) f32, counts_dev (frames) i32 or NULL = D, flags_dev or NULL, flag_joints
 *       (0: flags are (frames, D); else (frames, D, K)), video_start_dev (num_videos + 1) i64, num_videos, frames, state_dev (num_videos
 *       blocks), assignment_dev (frames, D) i32, track_of_dev (frames, D) i32 = the track id of each detection or -1, track_ids_dev
 *       (frames, S) i32 / born_dev (frames, S) u8 / alive_dev (frames, S) u8 or NULL each, counters_dev (num_videos, 2) i32 = (next_id,
 *       dropped), stream): one workgroup per video runs its frames in order from a fresh state and leaves its final state in block v of
 *       state_dev.  One launch.
 *   uu3d_stream_associate(params, state_dev, dets_dev (D, K, 2), count_dev (1) i32, flags_dev or NULL, flag_joints, kp_out_dev (S, K, 2)
 *       f32, flags_out_dev, flags_out_joints, active_out_dev (S) u8, born_out_dev (S) u8, assignment_dev (D) i32, track_ids_dev (S) i32,
 *       dropped_dev (1) i32, stream): ONE frame, one workgroup -- the first launch of a live tick, in front of uu3d_stream_reset with
 *       born_out_dev as its slot mask.  kp_out = the slot's detection, zeros for a slot without one; flags_out (S, K) (flags_out_joints
 *       != 0): 1 iff the joint is observed; (S) otherwise: 1 iff the slot has a detection and every joint flag of it is set (an unmatched
 *       alive slot's frame is MISSING); active_out = alive.  Same arguments at every tick: it replays from the tick's captured graph.
 * Every output element has one writer, no atomics, dets_dev is only read (8-byte aligned; never kp_out_dev): bitwise repeatable.
 */
typedef struct uu3d_associate_params {
    int32_t slots, detections, keypoints;  /* S, D, K: each in [1, 64] */
    int32_t max_age, min_common, reserved; /* >= 0, >= 1, 0 */
    double max_dist;                       /* >= 0; compared squared */
} uu3d_associate_params;
size_t uu3d_associate_state_bytes(int32_t slots, int32_t keypoints);
int uu3d_associate_reset(const uu3d_associate_params* params, void* state_dev, const uint8_t* slot_mask_dev, void* stream);
int uu3d_associate_detections(const uu3d_associate_params* params, const float* dets_dev, const int32_t* counts_dev, const uint8_t* flags_dev,
                              int32_t flag_joints, const int64_t* video_start_dev, int32_t num_videos, int64_t frames, void* state_dev,
                              int32_t* assignment_dev, int32_t* track_of_dev, int32_t* track_ids_dev, uint8_t* born_dev, uint8_t* alive_dev,
                              int32_t* counters_dev, void* stream);
int uu3d_stream_associate(const uu3d_associate_params* params, void* state_dev, const float* dets_dev, const int32_t* count_dev,
                          const uint8_t* flags_dev, int32_t flag_joints, float* kp_out_dev, uint8_t* flags_out_dev, int32_t flags_out_joints,
                          uint8_t* active_out_dev, uint8_t* born_out_dev, int32_t* assignment_dev, int32_t* track_ids_dev, int32_t* dropped_dev,
                          void* stream);

/*
 * ABSOLUTE ROOT POSITION (predict.solve_roots, predict.predict_tracks(camera=...), predict.predict_detections(camera=...)): every pose these
 * calls return is root-relative; eight people of one video all sit on the origin.  The 2D keypoints that were uplifted, together with the
 * camera's intrinsics, determine where each skeleton must stand so that it projects onto them: a linear least-squares problem with three
 * unknowns per frame.  predict.solve_roots_host and predict.root_trajectory_host are the same rule in numpy, bit for bit.  No accuracy is
 * claimed: the model's scale error goes 1:1 into the depth.
 * THE RULE, in float64, every product and sum rounded, no fused multiply-add, sums over the used joints in ascending joint order.
 * Camera (fx, fy, cx, cy), no distortion, in the units of the 2D coordinates as given; non-finite, fx <= 0 or fy <= 0: the caller refuses
 * it (a frame of such a camera is not solved).  Joint j of a frame is USED iff its byte of joint_flags_dev (frames, J) u8 is non-zero (NULL:
 * no flags) and both of its 2D coordinates are finite -- the raw coordinates in the model's layout, behind uu3d_map_keypoints and in
 * front of uu3d_repair_joints, the normalisation and the resampling: a filled joint is an interpolation, not a measurement, and a frame
 * the network never saw still fixes its own root from the joints that were seen.  With the frame's pose (X, Y, Z) widened from float32:
 *     a = (u - cx) / fx    b = (v - cy) / fy    p = a * Z - X    q = b * Z - Y
 *     n = the used joints; Sa += a; Sb += b; Sq += (a * a + b * b); Sp += p; Sk += q; Sr += (a * p + b * q)
 *     den = Sq - (Sa * Sa + Sb * Sb) / n        num = (Sa * Sp + Sb * Sk) / n - Sr
 *     Tz = num / den        Tx = (Sp + Sa * Tz) / n        Ty = (Sk + Sb * Tz) / n
 * (the normal equations of Tx - a Tz = p, Ty - b Tz = q).  The frame is SOLVED iff n >= min_joints (>= 2), den > 0, Tx, Ty and Tz are
 * finite, Tz > 0 and Z + Tz > 0 for every used joint; the root of a frame that is not solved is zeros.
 * TRAJECTORY.  The root motion of a track is the piecewise-linear function through its solved given frames, read at the positions of the
 * returned frames.  The host hands over each position as an exact rational in given-frame units (predict.root_plan): base_dev (out_frames)
 * i64 = the global row of the given frame at or before it, wnum_dev / wden_dev (out_frames) i64 = the fraction behind that frame, 0 <= wnum <
 * wden, every (frames of the track) * wden below 2^53.  With L = the nearest solved frame of the track at or before base and R = the
 * nearest one behind base:
 *     wnum == 0 and L == base:  the bits of that frame's root, rounded once to float32                                    root_state 1
 *     L and R exist:  (float)(root[L] * (1.0 - w) + root[R] * w), w = (double)((base - L) * wden + wnum) / (double)((R - L) * wden)    2
 *     only one of them exists (before the first solved frame, behind the last one):  its root, held                               2
 *     the track has no solved frame:  zeros                                                                                       0
 *
 *   uu3d_solve_roots(poses_dev (frames, J, 3) f32, kp2d_dev (frames, J, 2) f32 8-byte aligned, joint_flags_dev or NULL, frames, J,
 *       row_track_dev (frames) i32 or NULL = camera 0 for every frame, num_tracks, cameras_dev (num_tracks, 4) f64, min_joints, roots_dev
 *       (frames, 3) f64, solved_dev (frames) u8, stream): one launch, one lane per frame.  J > 64: UU3D_ERR_UNSUPPORTED.  frames == 0 is a
 *       no-op that returns UU3D_OK.  A track id out of range: not solved, nothing is read out of bounds.
 *   uu3d_root_trajectory_scratch_bytes(frames): two (frames) i32 planes; 0 for arguments out of range (frames < 2^31).
 *   uu3d_root_trajectory(roots_dev, solved_dev, frames, track_start_dev (num_tracks + 1) i64: track t is given frames [track_start[t],
 *       track_start[t + 1]), num_tracks, base_dev, wnum_dev, wden_dev, out_frames, out_roots_dev (out_frames, 3) f32, root_state_dev
 *       (out_frames) u8, scratch_dev 4-byte aligned, scratch_bytes, stream): two segmented scans along the given frames of every track (one
 *       workgroup per track, the scheme of uu3d_repair_joints: the cost does not depend on the length of a gap), then one lane per returned
 *       frame.  Two launches.  A plan entry or a scan entry out of range gives NaN and state 0, never a read out of bounds.
 * Every output element has one writer, no atomics, the caller's memory is only read, nothing copies to the host or waits: bitwise repeatable.
 */
int uu3d_solve_roots(const float* poses_dev, const float* kp2d_dev, const uint8_t* joint_flags_dev, int64_t frames, int32_t num_keypoints,
                     const int32_t* row_track_dev, int32_t num_tracks, const double* cameras_dev, int32_t min_joints, double* roots_dev,
                     uint8_t* solved_dev, void* stream);
size_t uu3d_root_trajectory_scratch_bytes(int64_t frames);
int uu3d_root_trajectory(const double* roots_dev, const uint8_t* solved_dev, int64_t frames, const int64_t* track_start_dev, int32_t num_tracks,
                         const int64_t* base_dev, const int64_t* wnum_dev, const int64_t* wden_dev, int64_t out_frames, float* out_roots_dev,
                         uint8_t* root_state_dev, void* scratch_dev, size_t scratch_bytes, void* stream);

/*
 * LENS DISTORTION (predict.undistort_points, predict.predict_tracks(camera=Camera(..., distortion=...)), predict.predict_detections,
 * stream.StreamSession): the calls above read a camera as an ideal pinhole.  A real lens puts a keypoint near the image border tens of
 * pixels from where a pinhole would; this call takes the raw pixels a detector saw back to the pixels a pinhole with the same intrinsics
 * would have seen, on the device, in front of everything else that looks at a track (uu3d_map_keypoints included: an affine joint map does
 * not commute with distortion).  predict.undistort_points_host is the same rule in numpy, bit for bit.  No accuracy is claimed.
 * THE RULE, in float64, every operation rounded once, no fused multiply-add, one final rounding to float32.  A camera is ten doubles: fx,
 * fy, cx, cy, then k1, k2, p1, p2, k3 in OpenCV's Brown-Conrady order, then tol in pixels.  For a raw point (u, v) widened from float32:
 *     x0 = (u - cx) / fx    y0 = (v - cy) / fy    x = x0    y = y0
 *     exactly 20 times, no early exit (the fixed-point iteration of OpenCV's undistortPoints):
 *         r2 = x * x + y * y                                   ic = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
 *         dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)      dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
 *         x = (x0 - dx) * ic                                   y = (y0 - dy) * ic
 *     then r2, dx, dy once more from the final (x, y), rad = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2, xd = x * rad + dx, yd = y * rad + dy.
 * The point is ACCEPTED iff u, v, x and y are finite, |xd - x0| * fx <= tol and |yd - y0| * fy <= tol, and the result, (fx * x + cx,
 * fy * y + cy) rounded once to float32, is finite.  Any other point -- a non-finite input, an observation outside the region where the
 * model can be inverted (with strong barrel distortion that region does not cover the plane), a camera with a non-finite intrinsic or
 * fx <= 0 or fy <= 0 -- is (NaN, NaN), the quiet NaN 0x7fc00000: a lost joint for the finite tests of everything behind.
 *
 *   uu3d_undistort_points(in_dev (rows, points_per_row, 2) f32, out_dev the same shape, never in_dev, both 8-byte aligned, rows,
 *       points_per_row, row_track_dev (rows) i32 or NULL = camera 0 for every row, num_tracks, cameras_dev (num_tracks, 10) f64, stream):
 *       one launch, one lane per point, one 8-byte load and one 8-byte store.  rows == 0 is a no-op that returns UU3D_OK.  A track id out
 *       of range writes NaN, nothing is read out of bounds.  The same arguments at every tick: it replays from a live tick's captured
 *       graph, where it is the first launch (in_dev the staged push, out_dev a buffer of the session).
 * Every output element has one writer, no atomics, in_dev is only read, nothing copies to the host or waits: bitwise repeatable.
 */
int uu3d_undistort_points(const float* in_dev, float* out_dev, int64_t rows, int32_t points_per_row, const int32_t* row_track_dev,
                          int32_t num_tracks, const double* cameras_dev, void* stream);

/*
 * WORLD SPACE (predict.camera_to_world, predict.predict_tracks(camera=Camera(..., orientation=, translation=)), predict.predict_detections,
 * stream.StreamSession): the scene the calls above return -- root-relative poses and a root per frame -- stands in the camera's own space,
 * where "up" is a slanted direction for every camera that is tilted or rolled.  This call takes it to world axes with the extrinsics a
 * calibration hands over beside the intrinsics: behind the root solve (which stays in camera space), in front of the One-Euro filters
 * (which then steady the floor's axes, not the camera's) and of the joint rotations.  predict.camera_to_world_host is the same rule in
 * numpy, bit for bit.  The convention is h36m.camera_to_world's: X_world = qrot(q, X_cam) + t, q the camera's orientation, t its position.
 * THE RULE, in float64 on the float32 inputs, every operation rounded once, no fused multiply-add, one final rounding to float32.  A
 * camera is seven doubles: the UNIT quaternion q = (w, x, y, z) (normalised once on the host, in float64), then t.  For a point
 * v = (a, b, c):
 *     uv  = (y * c - z * b,        z * a - x * c,        x * b - y * a)
 *     uuv = (y * uv2 - z * uv1,    z * uv0 - x * uv2,    x * uv1 - y * uv0)
 *     r_i = v_i + 2.0 * (w * uv_i + uuv_i)
 * A JOINT of a pose becomes (float) r_i: poses are rotated only, they stay relative to their root, and the exact zeros of the root joint
 * stay +0.0 (poses that are not root-relative are rotated only as well; poses + roots[:, None] is the world scene in both cases).  A ROOT
 * whose root_state is not 0 becomes (float) (r_i + t_i); a root with state 0 stays zeros.  NaN in, NaN out.  root_state is only read.
 *
 *   uu3d_camera_to_world(poses_dev (rows, J, 3) f32 and poses_out_dev the same shape -- both NULL: roots only --, roots_dev (rows, 3) f32,
 *       root_state_dev (rows) u8 and roots_out_dev (rows, 3) f32 -- all three NULL: poses only --, rows, J, row_track_dev (rows) i32 or
 *       NULL = camera 0 for every row, num_tracks, extrinsics_dev (num_tracks, 7) f64, stream): one launch of 256-thread blocks, one lane
 *       per (row, point), the points of a row being its J joints and, as point J, its root; one 12-byte load and one 12-byte store per
 *       lane.  An output pointer MAY equal its input pointer: a lane reads its own element before it writes it.  rows == 0 is a no-op that
 *       returns UU3D_OK.  A track id out of range writes NaN, nothing is read out of bounds.  The same arguments at every tick: it replays
 *       from a live tick's captured graph, directly behind uu3d_stream_root (out of place, stateless, all slots: a slot that is not fresh
 *       gets its previous bits again from the held camera-space buffers), and from the drain graph behind uu3d_stream_root_drain.
 * Every output element has one writer, no LDS, no atomics, nothing copies to the host or waits: bitwise repeatable.
 */
int uu3d_camera_to_world(const float* poses_dev, float* poses_out_dev, const float* roots_dev, const uint8_t* root_state_dev,
                         float* roots_out_dev, int64_t rows, int32_t J, const int32_t* row_track_dev, int32_t num_tracks,
                         const double* extrinsics_dev, void* stream);

/*
 * SEVERAL VIEWS (predict.fuse_views, predict.solve_view_roots, predict.predict_views): V calibrated cameras, 1 <= V <= 8, see the same
 * person at the same, time-synchronised frames.  WORLD SPACE has put every view's root-relative pose into one frame; the two calls here
 * join them to one pose per frame and solve ONE world root per frame from all views' 2D keypoints at once, which takes the depth
 * ambiguity of ABSOLUTE ROOT POSITION away: with a second view the model's scale error no longer goes into the depth.
 * predict.fuse_views_host and predict.solve_view_roots_host are the same rules in numpy, bit for bit.  No accuracy is claimed.
 * All buffers are view-major: poses_dev (V, rows, J, 3) f32 in world axes, kp2d_dev (V, rows, J, 2) f32 -- the raw, undistorted
 * coordinates in the model's layout, as ABSOLUTE ROOT POSITION reads them --, joint_flags_dev (V, rows, J) u8 or NULL.  Joint j of view v
 * at frame f is USED iff its flag is non-zero (NULL: every joint) and both of its coordinates are finite.  View v SEES frame f iff at
 * least min_joints (>= 2) of its joints are used there.  In float64 on the float32 inputs, every operation rounded once, no fused
 * multiply-add, one final rounding to float32 (the poses) or none (the roots).
 * FUSION.  Per frame, joint and channel: s = 0.0; for v ascending over the seeing views s = s + (double) pose_v; the fused value is
 * (float)(s / (double) n), n the number of seeing views, and view_count = n.  No view sees the frame: the same mean over ALL V views and
 * view_count = 0 (the network has upsampled over the gap in every view).  The root joint's zeros stay +0.0; NaN in, NaN out.
 * ROOT.  The unknown is the world root T.  A camera is sixteen doubles: fx, fy, cx, cy, then the camera's axes in world coordinates r1,
 * r2, r3 (the unit quaternion of WORLD SPACE applied to e_1, e_2, e_3 on the host), then its position t.  Over the seeing views in
 * ascending order and their used joints in ascending order, with P the frame's fused pose widened from float32:
 *     a = (u - cx) / fx    b = (v - cy) / fy    n = r1 - a * r3    m = r2 - b * r3    d = t - P_j
 *     e = (n0 * d0 + n1 * d1) + n2 * d2        g = (m0 * d0 + m1 * d1) + m2 * d2
 *     A_ik += (n_i * n_k + m_i * m_k) for ik = 00, 01, 02, 11, 12, 22        B_i += (n_i * e + m_i * g)
 * (the normal equations of n . (T + P_j - t) = 0, m . (T + P_j - t) = 0), solved by cofactors:
 *     c00 = A11 * A22 - A12 * A12    c01 = A02 * A12 - A01 * A22    c02 = A01 * A12 - A02 * A11
 *     c11 = A00 * A22 - A02 * A02    c12 = A01 * A02 - A00 * A12    c22 = A00 * A11 - A01 * A01
 *     det = (A00 * c00 + A01 * c01) + A02 * c02
 *     x0 = (c00 * B0 + c01 * B1) + c02 * B2    x1 = (c01 * B0 + c11 * B1) + c12 * B2    x2 = (c02 * B0 + c12 * B1) + c22 * B2
 *     T_i = x_i / det
 * The frame is SOLVED iff at least one view sees it, det is finite and > 0, det > 2^-40 * ((A00 * A11) * A22), T is finite and every used
 * joint of every seeing view lies in front of its camera: with w = (T + P_j) - t, (r3_0 * w0 + r3_1 * w1) + r3_2 * w2 > 0.  The root of
 * a frame that is not solved is zeros.  (The rank guard: one view whose used joints share one pixel gives a matrix of rank 2, whose det
 * is zero in exact arithmetic and rounding noise of either sign here, about 2^-52 of Hadamard's bound A00 * A11 * A22.)  uu3d_root_trajectory joins the solved frames of a person as it joins those of a track.
 *
 *   uu3d_fuse_views(poses_dev, kp2d_dev 8-byte aligned, joint_flags_dev or NULL, views, rows, J, min_joints, fused_dev (rows, J, 3) f32,
 *       never poses_dev, view_count_dev (rows) u8, sees_dev (views, rows) u8, stream): one launch of 256-thread blocks, one lane per (frame,
 *       joint), one 12-byte store per lane; the lane of joint 0 also writes the frame's view_count and sees bytes.
 *   uu3d_solve_view_roots(fused_dev (rows, J, 3) f32, kp2d_dev, joint_flags_dev or NULL, views, rows, J, cameras_dev (views, 16) f64,
 *       min_joints, roots_dev (rows, 3) f64, solved_dev (rows) u8, stream): one launch, one lane per frame, the shape of uu3d_solve_roots.
 *       A camera with a non-finite intrinsic, fx <= 0 or fy <= 0: the frames it sees are not solved.  The cameras belong to the views,
 *       not to the rows, so there is no per-row index that could leave their range.
 * Both: views > 8 or J > 64: UU3D_ERR_UNSUPPORTED.  rows == 0 is a no-op that returns UU3D_OK.  Every output element has one writer, no
 * LDS, no atomics, the inputs are only read, nothing copies to the host or waits: bitwise repeatable.
 */
int uu3d_fuse_views(const float* poses_dev, const float* kp2d_dev, const uint8_t* joint_flags_dev, int32_t views, int64_t rows,
                    int32_t num_keypoints, int32_t min_joints, float* fused_dev, uint8_t* view_count_dev, uint8_t* sees_dev, void* stream);
int uu3d_solve_view_roots(const float* fused_dev, const float* kp2d_dev, const uint8_t* joint_flags_dev, int32_t views, int64_t rows,
                          int32_t num_keypoints, const double* cameras_dev, int32_t min_joints, double* roots_dev, uint8_t* solved_dev,
                          void* stream);

/*
 * WHO IS WHO (predict.view_pair_sums, predict.group_views, predict.gather_view_tracks, predict.match_views,
 * predict.predict_views(match=...)): SEVERAL VIEWS wants the same index to be the same person in every camera, but every camera's tracker
 * numbers people in the order it meets them.  The three calls here find the correspondence from the geometry alone and lay the tracks
 * out per person.  predict.view_pair_sums_host, predict.group_views_host and predict.gather_view_tracks_host are the same rules in
 * numpy, bit for bit.  Greedy, view by view, dependent on the order of the views: no matching accuracy is claimed.
 * M tracks in all, 1 <= M <= 64, view-major: view_of_host (M) i32 in HOST memory, ascending, every entry in 0 .. views - 1 (a view may be
 * empty); all tracks on one clock with one length T.  kp_dev (M, T, J, 2) f32: the detector's own joints, undistorted -- the same joint
 * index in two views is all the rule needs --, joint_flags_dev (M, T, J) u8 or NULL; a joint is USED as in SEVERAL VIEWS.  cameras_dev
 * (views, 16) f64: the rows of SEVERAL VIEWS.  In float64 on the float32 inputs, every operation rounded once, no fused multiply-add.
 * PAIR SUMS.  For tracks p < q of different views v, w: o = t_w - t_v, oo = (o0 * o0 + o1 * o1) + o2 * o2; oo not finite or not > 0
 * (coincident cameras cannot be matched by geometry): no terms.  Else per frame f and joint j used in both tracks, per track
 *     a = (u - cx) / fx    b = (v - cy) / fy    d_i = (r1_i * a + r2_i * b) + r3_i            (the pixel's ray in world axes)
 * and with dp, dq the two rays
 *     c = dp x dq (c0 = dp1 * dq2 - dp2 * dq1, ...)    cc = (c0 * c0 + c1 * c1) + c2 * c2    pp, qq: the same expression of dp, dq
 *     oc = (o0 * c0 + o1 * c1) + o2 * c2               e = (oc * oc) / cc                    (the squared distance of the two LINES)
 * The term counts iff cc > 2^-20 * (pp * qq) -- rays closer than about 1e-3 rad carry no distance information -- and e is finite.  The
 * rays are lines, not half-lines: an intersection behind a camera is not rejected.  Order: per frame s_f = 0.0, s_f = s_f + e over the
 * counted joints ascending, n_f their number; lane l of 256 sums s_f for f = l, l + 256, ... ascending from 0.0; then for stride = 128,
 * 64, ..., 1: x[l] = x[l] + x[l + stride] for l < stride; sums[p][q] = sums[q][p] = x[0], terms[p][q] = terms[q][p] = the sum of n_f.
 * Same-view pairs, the diagonal and pairs without terms hold 0.0 and 0.
 * GROUPING.  Persons start as the tracks of the first non-empty view, in track order, ids from 0.  For each later view w ascending: for
 * person k (members m_1 < m_2 < ..., at most one per view) and track b of view w, S = 0.0, S = S + sums[m][b] over the members with
 * terms[m][b] > 0 ascending, n = the sum of those terms; the pair is allowed iff n >= min_terms and S / (double) n <= max_dist * max_dist.
 * Repeatedly the allowed pair of smallest S / n among the persons without a track in view w and the unmatched tracks of view w is
 * taken; ties go to the smaller k, then the smaller b.  Only persons that existed before the step compete; the tracks of view w left
 * over then become new persons in ascending track order.
 *
 *   uu3d_view_pair_sums(kp_dev 8-byte aligned, joint_flags_dev or NULL, view_of_host, tracks, frames, J, views, cameras_dev,
 *       sums_dev (M, M) f64, terms_dev (M, M) i32, stream): one launch, one workgroup of 256 lanes per unordered pair p <= q, which writes
 *       both mirrored elements; the fixed tree runs through LDS.  frames * J must stay below 2^31.
 *   uu3d_group_views(sums_dev, terms_dev, view_of_host, tracks, views, max_dist >= 0, min_terms >= 1, person_dev (M) i32,
 *       n_persons_dev (1) i32, table_dev (views, M) i32, stream): one launch of one wave.  table[v][k] = the track of person k in view v
 *       or -1; columns >= n_persons are -1.
 *   uu3d_gather_view_tracks(src_dev (views * persons) i32, poses_dev (M * T, J, 3) f32, kp2d_dev (M * T, J, 2) f32 8-byte aligned,
 *       joint_flags_dev (M * T, J) u8 or NULL, views, persons, frames, J, tracks, out_poses_dev (views, persons * T, J, 3) f32,
 *       out_kp2d_dev (views, persons * T, J, 2) f32, out_flags_dev (views, persons * T, J) u8, stream): one launch, one lane per (view,
 *       person row, joint); src[v * persons + k] = the track whose rows become person k's block of view v, or -1 (as is anything outside
 *       0 .. M - 1): zero poses, NaN keypoints and flags 0, so that view does not SEE the frame.  A NULL joint_flags_dev reads as ones.
 * All: views > 8, tracks or persons > 64 or J > 64: UU3D_ERR_UNSUPPORTED; bad counts, NULLs, misalignment or a view_of_host that does not
 * ascend: UU3D_ERR_INVALID_ARGUMENT -- every guard before any device call.  Every output element has one writer, no atomics, the inputs
 * are only read, nothing copies to the host or waits: bitwise repeatable.
 */
int uu3d_view_pair_sums(const float* kp_dev, const uint8_t* joint_flags_dev, const int32_t* view_of_host, int32_t tracks, int64_t frames,
                        int32_t num_keypoints, int32_t views, const double* cameras_dev, double* sums_dev, int32_t* terms_dev, void* stream);
int uu3d_group_views(const double* sums_dev, const int32_t* terms_dev, const int32_t* view_of_host, int32_t tracks, int32_t views,
                     double max_dist, int32_t min_terms, int32_t* person_dev, int32_t* n_persons_dev, int32_t* table_dev, void* stream);
int uu3d_gather_view_tracks(const int32_t* src_dev, const float* poses_dev, const float* kp2d_dev, const uint8_t* joint_flags_dev,
                            int32_t views, int32_t persons, int64_t frames, int32_t num_keypoints, int32_t tracks, float* out_poses_dev,
                            float* out_kp2d_dev, uint8_t* out_flags_dev, void* stream);

/*
 * ONE CLOCK (predict.view_lag_sums, predict.view_offsets, predict.align_views, predict.crop_views, predict.predict_views(align=...)):
 * SEVERAL VIEWS and WHO IS WHO take frame f of every view for the same instant, but cameras started by hand are seconds apart.  The two
 * calls here find every camera's clock offset, in whole frames, from the geometry alone: the squared distance between the lines of PAIR
 * SUMS is smallest when the two frames belong together.  predict.view_lag_sums_host and predict.view_offsets_host are the same rules in
 * numpy, bit for bit.  In float64 on the float32 inputs, every operation rounded once, no fused multiply-add.  Alignment is against the
 * reference view only: a camera that shares no person with it cannot be aligned, and there is no chaining through a third camera.
 * Offsets are whole frames of one common rate (up to half a frame remains; no sub-frame refinement, no per-camera frame rates).  Periodic
 * or standing motion is ambiguous: ties go to the smallest shift, and no claim is made for such scenes.  No accuracy is claimed.
 * TRACKS AND CLOCKS.  M tracks in all, 1 <= M <= 64, view-major, view_of_host (M) i32 ascending as in WHO IS WHO.  Every track starts at
 * frame 0 of its camera's clock and has its own length frames[m] >= 1: track m is rows first_row_host[m] .. first_row_host[m + 1] - 1 of
 * kp_dev (rows, J, 2) f32 -- the detector's own joints, undistorted --, first_row_host (M + 1) i64 in HOST memory, strictly ascending,
 * rows = first_row_host[M]; joint_flags_dev (rows, J) u8 or NULL; a joint is USED as in SEVERAL VIEWS.  View v's frame f was taken at
 * common time f + o_v.  The reference view r is the first non-empty view and o_r = 0; its tracks are 0 .. N_r - 1.
 * LAG SUMS.  For every track p of the reference view, every track q of a later view w and every lag l in -L .. L (l stands for
 * o_w - o_r): frame f of p pairs with frame g = f - l of q.  Per paired frame and per joint used in both, the term is e exactly as PAIR
 * SUMS defines it: the rays, c, cc, oc, the 2^-20 parallel test, the finite test, and no terms for coincident cameras.  The order is that
 * of PAIR SUMS over p's frames: s_f = 0.0, s_f = s_f + e over the counted joints ascending, n_f their number; a frame f without a
 * partner (g < 0 or g >= q's length) has s_f = 0.0 and n_f = 0; lane i of 256 sums s_f for f = i, i + 256, ... ascending from 0.0; then
 * for stride = 128, 64, ..., 1: x[i] = x[i] + x[i + stride] for i < stride.  sums[p][q][l + L] = x[0], terms[p][q][l + L] = the sum of
 * n_f: sums (N_r, M, 2L + 1) f64, terms (N_r, M, 2L + 1) i32.  The columns q of the reference view hold 0.0 and 0.  For two tracks of
 * equal length the slice at l = 0 is uu3d_view_pair_sums' sums[p][q] and terms[p][q], bit for bit.
 * OFFSETS.  For each later non-empty view w and each lag: S = 0.0, n = 0 (a 64-bit integer); for each reference track p ascending, the
 * candidates are the tracks q of w with terms[p][q][l + L] >= min_terms -- with same_index != 0 only the track with p's index inside its
 * view --; among them the one of smallest sums / (double) terms is taken, ties to the smaller q, and S = S + sums, n = n + terms.  The lag
 * is ALLOWED iff some p had a candidate; its score is S / (double) n.  The view takes the allowed lag of smallest score, ties to the
 * smaller |l|, then to the smaller l: offset[w] = l, state[w] = 1, score[w].  A view without an allowed lag: offset 0, state 0, score
 * 0.0.  The reference view and empty views: offset 0, state 1, score 0.0.
 *
 *   uu3d_view_lag_scratch_bytes(rows, J): the rays of every row's joints, three f64 each, then a byte per joint; 0 for arguments out of
 *       range.
 *   uu3d_view_lag_sums(kp_dev 8-byte aligned, joint_flags_dev or NULL, view_of_host, first_row_host, tracks, J, views, cameras_dev
 *       (views, 16) f64 as in SEVERAL VIEWS, max_lag = L, scratch_dev 8-byte aligned of uu3d_view_lag_scratch_bytes(rows, J) bytes,
 *       sums_dev, terms_dev, stream): two launches.  The first writes every joint's ray and whether it is used into scratch_dev, one lane
 *       per (row, joint), so that the divisions and the rotation are not repeated 2L + 1 times; the second runs one workgroup of 256
 *       lanes per (p, q, lag), the fixed tree through LDS.  The per-joint expression is one device function shared with
 *       uu3d_view_pair_sums.
 *   uu3d_view_offsets(sums_dev, terms_dev, view_of_host, tracks, views, max_lag, min_terms >= 1, same_index, offset_dev (views) i32,
 *       state_dev (views) i32, score_dev (views) f64, stream): one launch of one wave, the lags over the lanes, the minimum by a butterfly
 *       of exact comparisons.
 * Both: views > 8, tracks > 64, J > 64 or max_lag > 512: UU3D_ERR_UNSUPPORTED; max_lag < 1, min_terms < 1, bad counts, NULLs,
 * misalignment, a view_of_host that does not ascend, a first_row_host that does not ascend strictly, a track with frames * J >= 2^31 or
 * same_index with unequal non-empty view sizes: UU3D_ERR_INVALID_ARGUMENT -- every guard before any device call.  Every output element
 * has one writer, no atomics, the inputs are only read, nothing copies to the host or waits: bitwise repeatable.
 */
size_t uu3d_view_lag_scratch_bytes(int64_t rows, int32_t num_keypoints);
int uu3d_view_lag_sums(const float* kp_dev, const uint8_t* joint_flags_dev, const int32_t* view_of_host, const int64_t* first_row_host,
                       int32_t tracks, int32_t num_keypoints, int32_t views, const double* cameras_dev, int32_t max_lag, void* scratch_dev,
                       double* sums_dev, int32_t* terms_dev, void* stream);
int uu3d_view_offsets(const double* sums_dev, const int32_t* terms_dev, const int32_t* view_of_host, int32_t tracks, int32_t views,
                      int32_t max_lag, int32_t min_terms, int32_t same_index, int32_t* offset_dev, int32_t* state_dev, double* score_dev,
                      void* stream);

/*
 * WHERE RAYS MEET (predict.triangulate_joints, predict.place_joints, predict.predict_views(triangulate=...)): the fused pose of SEVERAL
 * VIEWS is a mean of V monocular lifts, and only the root is solved from the rays of all cameras; the network's scale and depth errors,
 * which all views share, stay in the pose.  Where two or more cameras see the same joint, its world position is fixed by geometry alone.
 * The two calls here place such joints there and leave every other joint -- one camera saw it, the frame's root joint cannot be
 * triangulated, only one camera saw the person -- to the fused lift: a hybrid pose, behind which bones, the root solve, the trajectory,
 * the filters and the rotations run unchanged.  predict.triangulate_joints_host and predict.place_joints_host are the same rules in
 * numpy, bit for bit.  In float64 on the float32 inputs, every operation rounded once, no fused multiply-add.  The camera rows
 * cameras_dev (views, 16) f64, USED and SEES are those of SEVERAL VIEWS; sees_dev (views, rows) u8 is the output of uu3d_fuse_views.
 * TRIANGULATION.  Per frame f and joint j the candidate set C holds the views v with sees[v][f] set and joint j USED in v.  A round:
 *   |C| < min_views: the joint is not triangulated.
 *   PASS 1, over v in C ascending, with q_v = 1.0:
 *     a = (u - cx) / fx;  b = (v - cy) / fy;  n_i = (r1_i - a r3_i) q_v;  m_i = (r2_i - b r3_i) q_v
 *     e = (n0 t0 + n1 t1) + n2 t2;  g = (m0 t0 + m1 t1) + m2 t2
 *     A_ik += (n_i n_k + m_i m_k) for ik = 00, 01, 02, 11, 12, 22;  B_i += (n_i e + m_i g)
 *   -- the normal equations of n . (X - t) = 0 and m . (X - t) = 0: the joint lies on the line of its pixel --, solved by the cofactor
 *   statements of SEVERAL VIEWS, term for term: c00 .. c22, det, x_i, X_i = x_i / det.  The solve is ACCEPTED iff det is finite and > 0,
 *   det > 2^-20 * ((A00 A11) A22) -- the 2^-20 of PAIR SUMS with its meaning: rays closer than about 1e-3 rad carry no distance
 *   information (two coincident cameras give rounding noise; cameras on a ring 0.037 or more with three views, 0.49 with two) -- and X
 *   is finite.  With w = X - t, z_v = (r3_0 w0 + r3_1 w1) + r3_2 w2; a z_v that is not > 0 or a solve that is not accepted: the joint is
 *   not triangulated (no view is dropped for it).
 *   PASS 2: the same statements with q_v = 1.0 / z_v, which turns the depth-weighted algebraic error into one in normalised image units;
 *   the same guards, z_v recomputed from the new X.
 *   RESIDUAL, per view of C: xc = (r1_0 w0 + r1_1 w1) + r1_2 w2, yc likewise with r2; du = |(fx (xc / z_v) + cx) - u|, dv likewise;
 *   rho_v = max(du, dv), +infinity when either is NaN.
 *   Every rho_v <= max_residual: the joint is triangulated, X and count = |C|.  Otherwise the view of the largest rho_v leaves C (ties:
 *   the larger view index) and another round runs.
 * A joint that is not triangulated gets X = zeros and count = 0.  At most views - min_views + 1 rounds, exactly two passes per round, no
 * early exit (the spirit of Camera.ITERATIONS).
 * PLACEMENT.  With r the root joint, for every frame f and joint j: count[f][r] > 0 and count[f][j] > 0: the pose is (float)(X_j - X_r)
 * per channel, +0.0 for j == r, and joint_views[f][j] = count[f][j].  Otherwise the joint keeps the fused pose's bits (NaN included) and
 * joint_views[f][j] = 0.
 * LIMITS.  With exactly two views an error along the epipolar line cannot be seen; with three views and an outlier the honest view can
 * be the one dropped, and the remaining two agree on a wrong point.  The lines are lines, apart from the z > 0 test.  A kept lifted joint
 * stays relative to the root, not to its triangulated parent, so bones across the seam can stretch (bones= runs behind the stage and
 * fixes lengths).  A frame without a triangulated root joint stays lifted as a whole.  max_residual is in pixels of the tracks as given;
 * the defaults of predict.Triangulate are conveniences, not tuned values.  No accuracy is claimed.
 *
 *   uu3d_triangulate_joints(kp2d_dev (views, rows, J, 2) f32, 8-byte aligned, joint_flags_dev (views, rows, J) u8 or NULL, sees_dev,
 *       views, rows, J, cameras_dev, min_views, max_residual, points_dev (rows, J, 3) f64, count_dev (rows, J) u8, stream): one launch, one
 *       lane per (frame, joint) in blocks of 256.  The views are walked through a bitmask; a view's weight is recomputed from pass 1's X.
 *   uu3d_place_joints(fused_dev (rows, J, 3) f32, points_dev, count_dev, rows, J, root, placed_dev (rows, J, 3) f32 -- not fused_dev --,
 *       joint_views_dev (rows, J) u8, stream): one launch, one lane per (frame, joint), one 12-byte store and one byte.
 * views > 8 or J > 64: UU3D_ERR_UNSUPPORTED; views < 1, J < 1, rows < 0, root outside 0 .. J - 1, min_views outside 2 .. 8, max_residual
 * not finite or not > 0, NULLs, misalignment: UU3D_ERR_INVALID_ARGUMENT -- every guard before any device call; rows == 0 is UU3D_OK and
 * launches nothing.  Every output element has one writer, no LDS, no atomics, the inputs are only read, nothing copies to the host or
 * waits: bitwise repeatable.
 */
int uu3d_triangulate_joints(const float* kp2d_dev, const uint8_t* joint_flags_dev, const uint8_t* sees_dev, int32_t views, int64_t rows,
                            int32_t num_keypoints, const double* cameras_dev, int32_t min_views, double max_residual, double* points_dev,
                            uint8_t* count_dev, void* stream);
int uu3d_place_joints(const float* fused_dev, const double* points_dev, const uint8_t* count_dev, int64_t rows, int32_t num_keypoints,
                      int32_t root, float* placed_dev, uint8_t* joint_views_dev, void* stream);

/*
 * WHERE THE CAMERAS STAND (predict.calibrate_views, predict.view_moment_sums, predict.view_position_sums, predict.solve_view_pose,
 * predict.predict_views(calibrate=...)): SEVERAL VIEWS takes every camera's extrinsics as given, and who puts two phones and a webcam on
 * tripods has none.  Every view's lift is the same skeleton in that camera's own axes, so the rotation between two cameras is the rotation
 * between their lifts; every view's rays and the lifts' metric size then fix where the second camera stands.  The calls here find the pose
 * of views 1 .. views - 1 in the space of view 0: a unit quaternion q_v and a position c_v with X_0 = qrot(q_v, X_v) + c_v, the convention
 * of WORLD SPACE.  predict.view_moment_sums_host, predict.view_position_sums_host and predict.solve_view_pose_host are the same rules in
 * numpy, bit for bit.  In float64 on the float32 inputs, every operation rounded once, no fused multiply-add, correctly rounded square root
 * and division; the order of every sum is part of the rule.  The buffers are view-major: poses_dev (views, rows, J, 3) f32 -- the lifts,
 * root-relative, in each camera's OWN axes --, kp2d_dev (views, rows, J, 2) f32, joint_flags_dev (views, rows, J) u8 or NULL; USED is the
 * test of SEVERAL VIEWS.
 * SEES.  View v sees row r iff at least min_joints of its joints are USED there -- the rule of uu3d_fuse_views, counted here because the
 * fusion runs later.  Row r is a TERM of view v >= 1 iff view 0 and view v both see it.
 * THE ORDER OF SUMMATION, for both sums: the rows are cut into chunks of 4096; within chunk k lane l of 256 adds the values of the terms
 * among rows 4096 k + l, + 256, ... ascending to 0.0; then for stride = 128, 64, ..., 1: x[l] = x[l] + x[l + stride] for l < stride (the
 * tree of PAIR SUMS), one value after the other; x[0] is the chunk's partial, partial_dev (views, chunks, 10) f64, the tenth value the
 * number of terms.  The solve adds a view's chunks ascending to 0.0.  View 0's partials are zeros.
 * 1. ROTATION (uu3d_view_moment_sums).  A term's values: s_ik = 0.0; s_ik = s_ik + p_v[j][i] * p_0[j][k] over ALL J joints ascending, p the
 *   lift of the row (an unobserved joint's lift is still read); ik = 00, 01, 02, 10, ..., 22.  Their sum is M_v.
 * 2. QUATERNION (uu3d_solve_view_pose, stage 0; one wave, a view per lane).  Horn's symmetric matrix
 *     N00 = (M00 + M11) + M22;  N01 = M12 - M21;  N02 = M20 - M02;  N03 = M01 - M10;  N11 = (M00 - M11) - M22;  N12 = M01 + M10
 *     N13 = M20 + M02;  N22 = (M11 - M00) - M22;  N23 = M12 + M21;  N33 = (M22 - M00) - M11
 *   goes through 10 sweeps of cyclic Jacobi, no early exit, the pairs (p, q) in the order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); E starts as
 *   the identity.  A rotation:
 *     th = (Nqq - Npp) / (2.0 Npq);  tt = (th >= 0.0 ? 1.0 : -1.0) / (|th| + sqrt(th th + 1.0));  t = Npq == 0.0 ? 0.0 : tt
 *     c = 1.0 / sqrt(t t + 1.0);  s = t c;  Npp = Npp - t Npq;  Nqq = Nqq + t Npq;  Npq = 0.0
 *     for the two other indices r ascending: (Nrp, Nrq) = (c Nrp - s Nrq, s Nrp + c Nrq);  for i = 0 .. 3: (Eip, Eiq) likewise
 *   -- the smaller-root tangent; a zero off-diagonal rotates nothing.  The eigenvalues are the diagonal; the column e of the largest is
 *   taken, ties to the smaller index; len = sqrt(((e0 e0 + e1 e1) + e2 e2) + e3 e3), q = e / len, negated as a whole when q0 < 0.0.  The
 *   view is REFUSED (state 0, the identity quaternion) when its terms are fewer than min_terms, an eigenvalue or q is not finite, or
 *   top - next > 2^-20 |top| does not hold for the two largest eigenvalues: the lifts then do not fix a rotation (all zeros, one point).
 * 3. POSITION (uu3d_view_position_sums; behind stage 0, whose quaternions it reads from device memory).  Per term, per view u in {0, v}, over
 *   u's USED joints ascending, the root-solve rows of SEVERAL VIEWS:
 *     a = (u - cx) / fx;  b = (v - cy) / fy;  n_i = r1_i - a r3_i;  m_i = r2_i - b r3_i;  e = (n0 P0 + n1 P1) + n2 P2;  g likewise with m
 *     A_ik += (n_i n_k + m_i m_k) for ik = 00, 01, 02, 11, 12, 22;  B_i += (n_i e + m_i g)
 *   View 0: r1, r2, r3 = e_1, e_2, e_3 and P = its own lift.  View v: r_i = qrot(q_v, e_i) and P = qrot(q_v, lift), qrot the statements of
 *   WORLD SPACE before their final rounding.  With the row's unknown root T: A0 T = -B0 and Av (T - c) = -Bv.  T is eliminated:
 *     A = A0 + Av, its cofactors c00 .. c22 and det by the statements of SEVERAL VIEWS; det not finite, not > 0 or not above
 *     2^-40 ((A00 A11) A22): the row is not a term.  K_ik = c_ik / det
 *     W_ik = (Av_i0 K_0k + Av_i1 K_1k) + Av_i2 K_2k, all nine
 *     S_ik = Av_ik - ((W_i0 Av_0k + W_i1 Av_1k) + W_i2 Av_2k) for ik = 00, 01, 02, 11, 12, 22
 *     h = B0 + Bv;  g_i = Bv_i - ((W_i0 h0 + W_i1 h1) + W_i2 h2)
 *   A view whose state is not 1, and a view whose or view 0's fx, fy, cx, cy are not finite with fx, fy > 0, has no terms.
 * 4. SOLVE (uu3d_solve_view_pose, stage 1: a second launch of the same kernel).  S c = g by the same cofactors, c_i = x_i / det; det not
 *   finite, not > 0, not above 2^-40 ((S00 S11) S22), or c not finite: state 0, position zeros, the quaternion stays.
 * pose_dev (views, 8) f64: q (4), c (3), the state as 1.0 / 0.0.  Row 0 is the identity, zeros and 1.  terms_dev (views) i32: the terms
 * of the stage's sums.
 * LIMITS.  The rig's scale is the model's: lifts scaled by s put every camera s times too far away, and nothing here rescales.  Every
 * view is calibrated against view 0 only; nothing is chained through a third camera.  Every term has unit weight in an algebraic error:
 * near and far frames count alike.  A person who only stands still fixes the position poorly.  The view-dependent depth errors of real
 * lifts are not modelled.  No accuracy is claimed.
 *
 *   uu3d_view_calibrate_chunks(rows): (rows + 4095) / 4096, 0 for rows outside 1 .. 2^31 - 1.
 *   uu3d_view_moment_sums(poses_dev, kp2d_dev, joint_flags_dev or NULL, views, rows, J, min_joints, partial_dev, stream): one launch, one
 *       workgroup per (chunk, view).
 *   uu3d_view_position_sums(..., J, intrinsics_dev (views, 4) f64, min_joints, pose_dev of stage 0, partial_dev, stream): likewise.
 *   uu3d_solve_view_pose(partial_dev, views, chunks, stage, min_terms, pose_in_dev (stage 1; not pose_out_dev), pose_out_dev, terms_dev,
 *       stream): one launch of one wave.
 * views > 8 or J > 64: UU3D_ERR_UNSUPPORTED; views < 1, J < 1, rows or chunks < 1, rows >= 2^31, min_joints < 2, min_terms < 1, another
 * stage, NULLs, misalignment: UU3D_ERR_INVALID_ARGUMENT -- every guard before any device call.  Every output element has one writer, no
 * atomics, the inputs are only read, nothing copies to the host or waits: bitwise repeatable.
 */
int64_t uu3d_view_calibrate_chunks(int64_t rows);
int uu3d_view_moment_sums(const float* poses_dev, const float* kp2d_dev, const uint8_t* joint_flags_dev, int32_t views, int64_t rows,
                          int32_t num_keypoints, int32_t min_joints, double* partial_dev, void* stream);
int uu3d_view_position_sums(const float* poses_dev, const float* kp2d_dev, const uint8_t* joint_flags_dev, int32_t views, int64_t rows,
                            int32_t num_keypoints, const double* intrinsics_dev, int32_t min_joints, const double* pose_dev, double* partial_dev,
                            void* stream);
int uu3d_solve_view_pose(const double* partial_dev, int32_t views, int64_t chunks, int32_t stage, int32_t min_terms, const double* pose_in_dev,
                         double* pose_out_dev, int32_t* terms_dev, void* stream);

/*
 * WHO IS WHO WITHOUT A WORLD (predict.lift_pair_sums, predict.match_lifts, predict.predict_views(match=MatchLifts(...))): WHO IS WHO
 * compares pixel rays in world axes, and cameras that WHERE THE CAMERAS STAND has yet to place share no world.  Matching does not need
 * rays: every view's lift is the same skeleton in that camera's own axes, so two tracks of different views are the same person iff their
 * lifts agree up to ONE rotation over the whole track, and Horn's largest eigenvalue gives the residual of that best rotation in closed
 * form.  The call here fills the (M, M) tables uu3d_group_views takes; uu3d_gather_view_tracks lays the tracks out as before.
 * predict.lift_pair_sums_host is the same rule in numpy, bit for bit.  In float64 on the float32 inputs, every operation rounded once, no
 * fused multiply-add, correctly rounded square root and division; the order of every sum is part of the rule.
 * INPUTS.  M tracks of one common length T, 1 <= M <= 64, view-major: view_of_host (M) i32 in HOST memory, ascending, as in WHO IS WHO.
 * poses_dev (M, T, J, 3) f32: every track's lifts, root-relative, in its camera's OWN axes; kp2d_dev (M, T, J, 2) f32 in the model's
 * layout; joint_flags_dev (M, T, J) u8 or NULL.  USED and SEES are the tests of SEVERAL VIEWS: track p sees frame f iff at least
 * min_joints of its joints are used there.
 * TERMS.  For tracks p < q of DIFFERENT views, frame f is a term iff both see it.  Eleven values per term, a the lift of p and b the lift
 * of q at the frame:
 *     s_ik = 0.0;  s_ik = s_ik + a[j][i] * b[j][k] over ALL J joints ascending, ik = 00, 01, 02, 10, ..., 22 -- the per-term values of
 *         uu3d_view_moment_sums, the same device function (an unobserved joint's lift is still read)
 *     e = 0.0;  e = e + (((a0 a0 + a1 a1) + a2 a2) + ((b0 b0 + b1 b1) + b2 b2)) over the joints ascending
 *     1.0
 * ORDER.  That of PAIR SUMS: lane l of 256 adds the values of the terms among frames l, l + 256, ... ascending to 0.0; then for stride =
 * 128, 64, ..., 1: x[l] = x[l] + x[l + stride] for l < stride, one value after the other.  There are no chunks.  x[0]: M (nine), E, n.
 * FINISH.  Horn's matrix of M and the 10 Jacobi sweeps of WHERE THE CAMERAS STAND, step 2 -- the same device function --; top = the
 * largest diagonal entry (top = N00; for i = 1, 2, 3: N_ii > top replaces it).  S = (E - 2.0 top) / (double) J; S < 0.0 becomes 0.0; top
 * or S not finite: S = 0.0 and no terms.  sums[p][q] = sums[q][p] = S, terms[p][q] = terms[q][p] = n, the number of term FRAMES.
 * Same-view pairs and the diagonal hold 0.0 and 0.
 * MEANING.  S / n is the mean over the term frames of the mean squared joint distance, in the poses' units, after the best common
 * rotation: what uu3d_group_views compares with max_dist * max_dist; its min_terms counts frames here.  Two persons with the same body
 * who move alike cannot be told apart, and short or noisy tracks close the gap between a true and a wrong pair; the lifts of a real model
 * carry view-dependent errors that are not modelled.  No matching accuracy is claimed.
 *
 *   uu3d_lift_pair_sums(poses_dev, kp2d_dev 8-byte aligned, joint_flags_dev or NULL, view_of_host, tracks, frames, J, views, min_joints,
 *       sums_dev (M, M) f64, terms_dev (M, M) i32, stream): one launch, one workgroup of 256 lanes per unordered pair p <= q; the fixed
 *       tree runs through LDS, lane 0 finishes and writes both mirrored elements.  frames * J must stay below 2^31.
 * tracks > 64, J > 64 or views > 8: UU3D_ERR_UNSUPPORTED; tracks < 1, frames < 1, J < 1, min_joints < 2, NULLs, misalignment or a
 * view_of_host that does not ascend: UU3D_ERR_INVALID_ARGUMENT -- every guard before any device call.  Every output element has one
 * writer, no atomics, the inputs are only read, nothing copies to the host or waits: bitwise repeatable.
 */
int uu3d_lift_pair_sums(const float* poses_dev, const float* kp2d_dev, const uint8_t* joint_flags_dev, const int32_t* view_of_host,
                        int32_t tracks, int64_t frames, int32_t num_keypoints, int32_t views, int32_t min_joints, double* sums_dev,
                        int32_t* terms_dev, void* stream);

/*
 * ANY FRAME RATE (predict.predict_tracks(fps=...)): the front of YOUR OWN 2D TRACKS for tracks that were not filmed at the rate the model
 * was trained for.  The table holds the MODEL's time grid: row `row` (track row_track_dev[row]) is model frame k of its track, which sits at
 * source position p_k = k * fps / model_fps.  The host works the positions out in exact integer arithmetic (predict.resample_plan) and
 * hands over, per table row, left_dev / right_dev (rows) i64 = rows of src_dev (src_rows, J, 2) f32, 8-byte aligned, and weight_dev (rows)
 * f64 = p_k - floor(p_k):
 *     left == right: the table row is source row left, normalised as uu3d_normalize_tracks does (resolution_dev (num_tracks, 2) f64, or NULL:
 *         taken as it is) -- the same bits; the right row is not read.  Model frames that coincide with a source frame (30 fps and input
 *         stride 5: every 5th model frame is every 3rd video frame) are therefore exact, not approximately so.
 *     else: both rows normalised the same way, then per coordinate (float)((double)a * (1.0 - w) + (double)b * w): two products and one
 *         sum in float64, each rounded, no fused multiply-add.
 * table_dev (rows, J, 2) f32, 16-byte aligned, is never src_dev (UU3D_ERR_INVALID_ARGUMENT: there is no in-place form).  A track id or a
 * plan row outside [0, src_rows) yields a NaN row, never a read out of bounds.  One launch for all tracks, one thread per 16 bytes of the
 * table, one writer per element, no atomics: bitwise repeatable.
 * valid_out_dev (rows) u8 or NULL; not NULL: a wave-per-row launch in front on the same stream writes valid_out[row] = the left source
 * frame is valid (valid_in_dev (src_rows) u8 non-zero, NULL = all) with all 2 J coordinates finite and, where left != right, the right one
 * too; a row whose byte is 0 is written as zeros (MISSED DETECTIONS above: hand valid_out to the _valid gathers).  valid_in_dev without
 * valid_out_dev is UU3D_ERR_INVALID_ARGUMENT.
 */
int uu3d_resample_tracks(const float* src_dev, int64_t src_rows, float* table_dev, int64_t rows, int32_t num_keypoints,
                         const int32_t* row_track_dev, int32_t num_tracks, const double* resolution_dev,
                         const int64_t* left_dev, const int64_t* right_dev, const double* weight_dev,
                         const uint8_t* valid_in_dev, uint8_t* valid_out_dev, void* stream);

/*
 * LIVE TRACKS AT ANY FRAME RATE (stream.StreamSession(fps=F)): LIVE TRACKS for a camera that does not run at the model's rate.  One SOURCE
 * frame per slot and push in, at F frames per second; one pose per slot and push out, at the source frame's own time.  Let
 * model_fps / F = a / b in lowest terms (uu3d_stream_rate; a, b < 2^20, so every product with a 31-bit counter is exact in int64).
 *
 * Input side.  Model frame k sits at source position k b / a -- predict.resample_plan's definition -- and is made the moment source frame
 * ceil(k b / a) has been pushed.  Where the position is a whole number the model frame is that source frame (normalised as
 * uu3d_stream_stage does: the same bits); otherwise its two neighbours are normalised first and then mixed in float64 with weight
 * (double)((k b) % a) / (double)a, the double resample_plan computes, by the device functions of uu3d_resample_tracks.  The two newest raw
 * source frames of a slot are all the history this needs.  After a slot's j-th push (0-based) its newest model frame is K = floor(j a / b);
 * the push made K - floor((j - 1) a / b) of them: 1 at j = 0, then between 0 and ceil(a / b).
 * Model side.  Every new model frame is one tick of LIVE TRACKS at cfg->lookahead = a_m (below), a SUB-TICK, with the stage replaced:
 *   uu3d_stream_resample_stage -> uu3d_frame_features -> uu3d_stream_commit with active_dev = sub_active_dev -> uu3d_forward_frames_ex ->
 *   uu3d_stream_emit (into a buffer of the caller's, not the session's output) -> uu3d_stream_file_keyframe
 * A slot whose next model frame is not due yet is inactive in the sub-tick, so a sub-tick in which no slot is due changes no byte of the
 * state and a push may be followed by more sub-ticks than it needs (at most ceil(a / b) are ever needed).  The session with a rate IS a
 * plain session at lookahead a_m fed the resampled model-rate frames.
 * Output side.  After the sub-ticks of a push, uu3d_stream_timed_emit: a slot that took its j-th frame at this push gets the pose of
 * source frame q = j - rate->lookahead (in SOURCE frames) once q >= 0 -- at EVERY such push, not only at keyframes.  It is read at model
 * position u = q a / b from the piecewise-linear motion through the emitted keyframes (centres that are multiples of P = cfg->pred_stride),
 * the rule of evaluation.keyframe_plan_at: k0 = floor(u / P) P, k1 = k0 where u == k0, else k0 + P.  u == k0: keyframe k0's bits.
 * Elsewhere (float)((double)p0 * (1.0 - w) + (double)p1 * w) with w = (double)(q a - k0 b) / (double)(P b), rounded once to float32; both
 * keyframes are already un-flipped, averaged and root-shifted.  Any other slot keeps its previous pose (zeros before its first) and is
 * reported as not fresh.
 * The lookahead.  a_m is the largest integer in [0, (N / 2) * seq_stride] with k1(j - lookahead) <= floor(j a / b) - a_m for every
 * j >= lookahead (periodic in j with period b P; the host enumerates one period: stream.rate_plan), so that k1 has been emitted when it is
 * read.  The emitted keyframes are kept per slot in a ring of key_ring = D poses, centre c at place (c / P) % D, where D - 1 is the largest
 * distance, in keyframes, from the newest emitted centre back to k0 over the same period.
 *
 * Per push, on one stream:
 *   uu3d_stream_source_push(model, cfg, rate, state_dev, kp_dev (slots, J, 2) f32 raw, active_dev (slots) u8, valid_in_dev (slots) u8 or
 *                           NULL, track_valid, stream)
 *       one workgroup per slot.  An active slot's source counter advances and the frame is filed in ring place (index & 1), with its
 *       validity byte: 1, or with track_valid != 0 (MISSED DETECTIONS, per SOURCE frame) valid_in && all 2 J coordinates finite.
 *   n sub-ticks (above), n >= the largest number of model frames an active slot makes at this push.
 *       uu3d_stream_resample_stage(model, cfg, rate, state_dev, resolution_dev or NULL, flip_order_dev, sub_active_dev (slots) u8,
 *                                  valid_out_dev (slots) u8 or NULL, frames_out_dev (halves * slots, J, 2) f32, stream)
 *           per slot: model frame k = the model counter is due iff ceil(k b / a) <= newest source index.  Due: the frame, its mirrored
 *           copy, sub_active = 1; not due: zeros, sub_active = 0.  valid_out_dev not NULL: valid_out = the left source frame's byte and,
 *           where the frame is mixed from two, the right one's -- the rule of uu3d_resample_tracks' valid_out_dev; a missing frame stages
 *           zeros and flows through uu3d_stream_commit_valid as a missing frame of LIVE TRACKS does.
 *       uu3d_stream_file_keyframe(model, cfg, rate, state_dev, fresh_dev, stream): behind uu3d_stream_emit, a fresh slot's pose (the held
 *           pose of the state block) goes to its keyframe ring.
 *   uu3d_stream_timed_emit(model, cfg, rate, state_dev, out_dev (slots, J, 3) f32, fresh_out_dev (slots) u8, stream)
 *
 *   uu3d_stream_rate_reset(model, cfg, rate, state_dev, slot_mask_dev or NULL, stream) = uu3d_stream_reset and, for the same slots, source
 *   counter 0 and held output pose 0.
 *
 * The state block is the one of LIVE TRACKS with more behind it (uu3d_stream_rate_state_layout; bytes is the size of the WHOLE block, all
 * zeros = every slot empty): source counters (slots) i32, pushed (slots) u8, source validity (slots, 2) u8, raw source frames
 * (slots, 2, J, 2) f32, the keyframe ring (slots, key_ring, key_stride) f32 with key_stride = J * 3 rounded up to 4 floats, held output
 * poses (slots, J, 3) f32.  No atomics, one writer per output element, all counters read and advanced on the device, every launch with the
 * same arguments at every push: the sub-tick replays from ONE captured hipGraph, a linear chain, as the tick of LIVE TRACKS does.
 */
typedef struct uu3d_stream_rate { int32_t a, b, lookahead /* source frames */, key_ring /* D */; } uu3d_stream_rate;
typedef struct uu3d_stream_rate_layout {
    int64_t source_frames_offset, pushed_offset, source_valid_offset, source_offset, keys_offset, key_stride, out_held_offset, bytes;
} uu3d_stream_rate_layout;
int uu3d_stream_rate_state_layout(const uu3d_model* model, const uu3d_stream_config* cfg, const uu3d_stream_rate* rate,
                                  uu3d_stream_rate_layout* out);
int uu3d_stream_source_push(uu3d_model* model, const uu3d_stream_config* cfg, const uu3d_stream_rate* rate, void* state_dev,
                            const float* kp_dev, const uint8_t* active_dev, const uint8_t* valid_in_dev, int32_t track_valid, void* stream);
int uu3d_stream_resample_stage(uu3d_model* model, const uu3d_stream_config* cfg, const uu3d_stream_rate* rate, const void* state_dev,
                               const double* resolution_dev, const int32_t* flip_order_dev, uint8_t* sub_active_dev,
                               uint8_t* valid_out_dev, float* frames_out_dev, void* stream);
int uu3d_stream_file_keyframe(uu3d_model* model, const uu3d_stream_config* cfg, const uu3d_stream_rate* rate, void* state_dev,
                              const uint8_t* fresh_dev, void* stream);
int uu3d_stream_timed_emit(uu3d_model* model, const uu3d_stream_config* cfg, const uu3d_stream_rate* rate, void* state_dev,
                           float* out_dev, uint8_t* fresh_out_dev, void* stream);
int uu3d_stream_rate_reset(uu3d_model* model, const uu3d_stream_config* cfg, const uu3d_stream_rate* rate, void* state_dev,
                           const uint8_t* slot_mask_dev, void* stream);

/*
 * ... with an output rate of its own (stream.StreamSession(fps=F, out_fps=G)): every push returns EVERY output frame that became due, not
 * one pose.  Output frame i of a slot lies at time i / G, model position u = i * model_fps / G = i pos_num / pos_den, and is read from
 * the piecewise-linear motion through the emitted keyframes exactly as uu3d_stream_timed_emit reads a source frame: k0 = floor(u / P) P,
 * u == k0 gives keyframe k0's bits, anything else (float)((double)p0 * (1.0 - w) + (double)p1 * w), w = (double)(i pos_num - k0 pos_den) /
 * (double)(P pos_den).  With G / F = c / d in lowest terms: after the push that made source frame j the newest of a slot, q = j -
 * rate->lookahead >= 0, the slot has emitted every output frame i <= floor(q c / d) -- the frames whose time is not later than that of
 * source frame q.  A push returns the ones that became due at it, oldest first: frame 0 alone at q == 0, afterwards floor(q c / d) -
 * floor((q - 1) c / d) of them, at most max_out = ceil(c / d) <= 64, possibly none when G < F; a slot that took no frame returns none.
 * uu3d_stream_out holds c, d, pos_num, pos_den (all in [1, 2^20)) and max_out.  The input and model sides, the lookahead a_m and the
 * rule of the keyframe ring are those above; the ring depth rate->key_ring must also cover the OLDEST output frame of a push, whose k0 can
 * be one keyframe older than that of source frame q (stream.rate_plan enumerates one common period of the three grids).
 *
 * Per push: uu3d_stream_source_push, the sub-ticks, then IN PLACE OF uu3d_stream_timed_emit
 *   uu3d_stream_timed_emit_multi(model, cfg, rate, out, state_dev, poses_dev (slots, max_out, J, 3) f32, 16-byte aligned,
 *                                count_dev (slots) i32, stream)
 *       one workgroup per slot; the slot's output counter is read by that workgroup only and advanced by one lane behind a barrier.
 *       n = floor(q c / d) + 1 - counter, clamped to [0, max_out] (0 for a slot that took no frame or with q < 0); rows r < n of the
 *       slot are output frames counter + r, rows r >= n are zeros, count[slot] = n, counter += n (it stops at INT32_MAX instead of
 *       wrapping).  16-byte stores wherever a quad of floats lies inside the slot's rows.  No atomics, one writer per output element.
 *   uu3d_stream_out_reset(model, cfg, rate, out, state_dev, slot_mask_dev or NULL, stream) = uu3d_stream_rate_reset and, for the same
 *       slots, output counter 0.
 * State: uu3d_stream_out_state_layout -- the block of uu3d_stream_rate_state_layout, unchanged, with the output counters (slots) i32
 * behind it at out_frames_offset; bytes is the size of the WHOLE block, all zeros = every slot empty.  A session without an output rate
 * needs none of this and its layout is the one above.
 */
typedef struct uu3d_stream_out { int32_t c, d /* G / F */, pos_num, pos_den /* model_fps / G */, max_out /* R */; } uu3d_stream_out;
typedef struct uu3d_stream_out_layout { int64_t out_frames_offset, bytes; } uu3d_stream_out_layout;
int uu3d_stream_out_state_layout(const uu3d_model* model, const uu3d_stream_config* cfg, const uu3d_stream_rate* rate,
                                 const uu3d_stream_out* out, uu3d_stream_out_layout* layout);
int uu3d_stream_timed_emit_multi(uu3d_model* model, const uu3d_stream_config* cfg, const uu3d_stream_rate* rate, const uu3d_stream_out* out,
                                 void* state_dev, float* poses_dev, int32_t* count_dev, void* stream);
int uu3d_stream_out_reset(uu3d_model* model, const uu3d_stream_config* cfg, const uu3d_stream_rate* rate, const uu3d_stream_out* out,
                          void* state_dev, const uint8_t* slot_mask_dev, void* stream);

/*
 * LIVE C1 MOTION (stream.StreamSession(fps=F, interpolation="cubic"), with or without out_fps): the poses of the two sessions above read
 * from the C1 Catmull-Rom cubic through the emitted keyframes in place of the line -- the rule of C1 MOTION BETWEEN KEYFRAMES
 * (evaluation.interpolate_cubic_host), live.  A pose at model position u = num / den has k0, k1 and the weight w exactly as above.
 * u == k0: keyframe k0's bits, as above.  Elsewhere the cubic Hermite segment from p1 = keyframe k0 to p2 = keyframe k1 = k0 + P at
 * t = w -- the same single float64 division of two integers -- with Catmull-Rom tangents from p0 = keyframe k0 - P and p3 = keyframe
 * k1 + P: m1 = (p2 - p0) / 2, or p2 - p1 in a slot's first segment (k0 < P: there is no keyframe in front, and its ring place is not
 * read), m2 = (p3 - p1) / 2 always -- a live track has no last segment.  float64 on the float32 keyframes, every operation rounded on
 * its own (no fused multiply-add), rounded once to float32: the bits of the numpy rule.  The root joint of a root-relative pose stays 0.
 * The plan has two more requirements than the linear one (stream.rate_plan(interpolation="cubic") enumerates both over the same
 * period): the newest emitted centre must have reached k1 + P wherever a pose is not on a keyframe, which raises the smallest lookahead
 * and lowers a_m; and rate->key_ring must still hold k0 - P of the oldest pose a push reads while the newest centre is filed.
 * The ring, the state layouts, every other launch and the resets are those above; only the emit of a push changes:
 *   uu3d_stream_timed_emit_cubic(model, cfg, rate, state_dev, out_dev, fresh_out_dev, stream) IN PLACE OF uu3d_stream_timed_emit, and
 *   uu3d_stream_timed_emit_multi_cubic(model, cfg, rate, out, state_dev, poses_dev, count_dev, stream) IN PLACE OF
 *   uu3d_stream_timed_emit_multi: the arguments, the status codes, the held pose and fresh_out, the counter discipline, the zero rows behind
 *   count and the stores of their linear siblings.  Each reads the four ring places (k0 / P - 1) .. (k0 / P + 2) modulo key_ring.
 */
int uu3d_stream_timed_emit_cubic(uu3d_model* model, const uu3d_stream_config* cfg, const uu3d_stream_rate* rate, void* state_dev,
                                 float* out_dev, uint8_t* fresh_out_dev, void* stream);
int uu3d_stream_timed_emit_multi_cubic(uu3d_model* model, const uu3d_stream_config* cfg, const uu3d_stream_rate* rate,
                                       const uu3d_stream_out* out, void* state_dev, float* poses_dev, int32_t* count_dev, void* stream);

/*
 * LIVE PER-JOINT MISSED DETECTIONS (stream.StreamSession(repair_joints=G)): PER-JOINT MISSED DETECTIONS for LIVE TRACKS.  The contract of
 * LIVE TRACKS is unchanged: after the push that made frame t the newest of a slot, the pose of frame t - lookahead is the one of the track
 * cut at t with uu3d_repair_joints (max_gap = G) in front.  The rule looks ahead (a gap is interpolated once it has closed), so a push may
 * REVISE frames the session has filed.  The revisions are bounded:
 *     coordinates change only for frames t - G .. t -- a gap of at most G frames closes at t (held -> interpolated), or a joint is seen for
 *         the first time at t (unfilled -> held from t).  Of those the session keeps the multiples of mask_stride and the edge frame: at
 *         most K = G / mask_stride + 2 frames per slot and tick;
 *     an older frame only ever goes from valid to MISSING -- a gap longer than G closes at t and the up to G frames that were held from
 *         its left end become unfillable: a byte of valid_state_dev, no features.  These frames are the FAR LIST of the tick.
 * 1 <= max_gap <= 32 (a declared cap of the live form: K and every buffer are fixed when the session is made); needs a model with strided
 * input (UU3D_ERR_UNSUPPORTED).  Per tick, on one stream, a linear chain with unchanging arguments that replays from ONE captured hipGraph:
 *
 *   uu3d_stream_repair_stage(model, cfg, max_gap, state_dev, repair_state_dev, kp_dev (slots, J, 2) f32 raw, resolution_dev or NULL,
 *                            active_dev, flip_order_dev, joint_flags_dev (slots, J) u8 or NULL, frames_out_dev (halves * slots * K, J, 2) f32,
 *                            stage_frame_dev (slots, K) i32, stage_valid_dev (slots, K) u8, far_frames_dev (slots, max_gap) i32,
 *                            joint_state_dev (slots, J) u8, stream)
 *       one workgroup per slot, one lane per joint.  A joint is observed iff its flag is non-zero (NULL: none given) and both coordinates
 *       are finite.  Files the raw frame and flags of an active slot (frame t = the slot's counter in state_dev, which it only reads), then
 *       writes: the K frames to re-stage -- the multiples of mask_stride in [max(0, t - G), t], oldest first, then the edge frame where it
 *       lies in that range and is no multiple of mask_stride; stage_frame = -1 for an unused entry --, each repaired by THE RULE of
 *       uu3d_repair_joints (the same float64 expression: the same bits), normalised as uu3d_stream_stage does, with its mirrored copy in
 *       the second half; stage_valid = the frame is a real observation (a missing or unused entry stages zeros); the far list (-1 for an
 *       unused entry); joint_state of frame t (1 observed, 2 filled, 0 neither).  An inactive slot changes nothing of its state, marks every
 *       entry unused and keeps its joint_state.
 *   uu3d_frame_features on frames_out_dev (halves * slots * K frames) -> features_dev (halves * slots * K, d_t)
 *   uu3d_stream_commit_repair(model, cfg, max_gap, state_dev, features_dev, active_dev, stage_frame_dev, stage_valid_dev, far_frames_dev,
 *                             valid_state_dev, rows_dev, stride_mask_dev, fresh_dev, stream)
 *       uu3d_stream_commit_valid with another filing step: staged frame f goes, features and valid byte, into ring place
 *       (f / mask_stride) % ring_capacity where that place still holds it (f a multiple of mask_stride, f > t - ring_capacity * mask_stride)
 *       and into the edge row where f is the edge frame of t; the frames of the far list get valid byte 0 under the same test.  The
 *       counter, the window, its masks and fresh are uu3d_stream_commit_valid's, from the same device code.
 *   uu3d_forward_frames_ex and uu3d_stream_emit as in LIVE TRACKS.
 *
 *   uu3d_stream_repair_reset(model, cfg, max_gap, repair_state_dev, slot_mask_dev or NULL, stream): beside uu3d_stream_reset, the same slots
 *   forget their observations.
 *
 * repair_state_dev: a caller-allocated, 256-byte aligned block of uu3d_stream_repair_bytes bytes, all zeros = every slot empty, laid out by
 * uu3d_stream_repair_layout: the raw frames t - G .. t (slots, window = G + 1, J, 2) f32 and their observed flags (slots, window, J) u8, frame
 * g at place g % window; per joint the last observation that has left that window, last (slots, J) i32 = its index + 1 (0: none) and
 * last_xy (slots, J, 2) f32; held (slots, J) u32: bit k = frame last + 1 + k has left the window as a valid frame in which the joint was
 * held from that observation -- what a long gap turns missing when it closes.  A slot's state is read and written by its own workgroup
 * only; no atomics, one writer per output element.
 */
typedef struct uu3d_stream_repair_state_layout {
    int64_t window, staged_frames /* K */, raw_offset, last_xy_offset, last_offset, held_offset, observed_offset, bytes;
} uu3d_stream_repair_state_layout;
size_t uu3d_stream_repair_bytes(const uu3d_model* model, const uu3d_stream_config* cfg, int32_t max_gap);
int uu3d_stream_repair_layout(const uu3d_model* model, const uu3d_stream_config* cfg, int32_t max_gap, uu3d_stream_repair_state_layout* out);
int uu3d_stream_repair_stage(uu3d_model* model, const uu3d_stream_config* cfg, int32_t max_gap, const void* state_dev, void* repair_state_dev,
                             const float* kp_dev, const double* resolution_dev, const uint8_t* active_dev, const int32_t* flip_order_dev,
                             const uint8_t* joint_flags_dev, float* frames_out_dev, int32_t* stage_frame_dev, uint8_t* stage_valid_dev,
                             int32_t* far_frames_dev, uint8_t* joint_state_dev, void* stream);
int uu3d_stream_commit_repair(uu3d_model* model, const uu3d_stream_config* cfg, int32_t max_gap, void* state_dev, const float* features_dev,
                              const uint8_t* active_dev, const int32_t* stage_frame_dev, const uint8_t* stage_valid_dev,
                              const int32_t* far_frames_dev, void* valid_state_dev, int32_t* rows_dev, uint8_t* stride_mask_dev,
                              uint8_t* fresh_dev, void* stream);
int uu3d_stream_repair_reset(uu3d_model* model, const uu3d_stream_config* cfg, int32_t max_gap, void* repair_state_dev,
                             const uint8_t* slot_mask_dev, void* stream);

/*
 * LIVE ABSOLUTE ROOT (stream.StreamSession(camera=...); stream.LiveRootHost is the same rule in numpy, bit for bit): ABSOLUTE ROOT POSITION
 * for LIVE TRACKS.  Every push returns, beside each slot's pose, where that pose stands in the camera's space.  With a lookahead the pose
 * belongs to an earlier frame than the one pushed, so the session keeps the raw 2D it will need.  No model: the calls take the joint count,
 * like uu3d_solve_roots, and run on any pose / fresh / counter buffers.  No accuracy is claimed (ABSOLUTE ROOT POSITION).
 * STATE per slot, in one caller-allocated block of uu3d_stream_root_bytes(slots, J, lookahead) bytes, 256-byte aligned, zeroed by
 * uu3d_stream_root_reset: a ring of the last W = lookahead + 1 raw frames in the model's joint layout (frame f at place f % W) with one
 * USED byte per joint, the last solved root (3 f64), and the state the slot returned last -- non-zero: a solved root exists.
 * THE RULE.  frames_dev (slots) i32 holds each slot's frame counter AFTER this push (uu3d_stream_commit has advanced it; a session with a
 * frame rate passes its source counters): the pushed frame is t = frames - 1.
 *   filing   active_dev[slot] != 0 (and frames >= 1): joint j of kp2d_dev (slots, J, 2) f32 -- the frame as pushed, behind
 *            uu3d_map_keypoints, before any normalisation or repair -- goes to place t % W.  USED iff its flag is set and both
 *            coordinates are finite; flags_dev: NULL (no flags), (slots) u8 with flags_per_joint == 0 (a frame's flag stands for all of its
 *            joints) or (slots, J) u8.  A joint that a repair fills is not flagged, hence never used; no later push revises the ring.
 *   solving  active and fresh_dev[slot] != 0: poses_dev (slots, J, 3) f32, the pose the push returns, is solved against frame
 *            c = t - lookahead by the per-frame rule of ABSOLUTE ROOT POSITION, unchanged (cameras_dev (slots, 4) f64, min_joints >= 2).
 *            Solved: roots_dev (slots, 3) f32 = the root rounded once, root_state_dev (slots) u8 = 1, and the root is held.  Not solved
 *            (or c < 0): the held root, state 2; no held root yet: zeros, state 0.  The rule is causal: it holds the last solved root and
 *            cannot interpolate towards a later solved frame as uu3d_root_trajectory does, because no later pose exists yet.
 *   any other slot (inactive, or not fresh) returns what it returned last, bit for bit, and nothing of its state changes.
 *
 *   uu3d_stream_root_bytes(slots, J, lookahead): 0 for arguments out of range (slots in [1, 2^20], J in [1, 64], lookahead in [0, 2^24]).
 *   uu3d_stream_root(slots, J, lookahead, root_state_dev, frames_dev, active_dev, fresh_dev, poses_dev, kp2d_dev 8-byte aligned, flags_dev,
 *       flags_per_joint, cameras_dev, min_joints, roots_dev, root_state_out_dev, stream): one launch, one wave per slot -- lane j files joint
 *       j, lane 0 solves.  J > 64: UU3D_ERR_UNSUPPORTED.
 *   uu3d_stream_root_reset(slots, J, lookahead, root_state_dev, slot_mask_dev (slots) u8 or NULL = every slot, stream): the chosen slots
 *       have no filed frame, no held root and state 0; beside uu3d_stream_reset, with the same mask (host-made or written on the device).
 * Every output and state element has one writer, no atomics, the caller's buffers are only read: bitwise repeatable, capturable.
 */
size_t uu3d_stream_root_bytes(int32_t slots, int32_t num_keypoints, int32_t lookahead);
int uu3d_stream_root(int32_t slots, int32_t num_keypoints, int32_t lookahead, void* root_state_dev, const int32_t* frames_dev,
                     const uint8_t* active_dev, const uint8_t* fresh_dev, const float* poses_dev, const float* kp2d_dev, const uint8_t* flags_dev,
                     int32_t flags_per_joint, const double* cameras_dev, int32_t min_joints, float* roots_dev, uint8_t* root_state_out_dev,
                     void* stream);
int uu3d_stream_root_reset(int32_t slots, int32_t num_keypoints, int32_t lookahead, void* root_state_dev, const uint8_t* slot_mask_dev,
                           void* stream);

/*
 * LIVE SEVERAL VIEWS (stream.StreamSession(views=V); stream.LiveViews, and stream.LiveViewsHost, the same rule in numpy, bit for bit):
 * SEVERAL VIEWS for LIVE TRACKS.  A rig of V calibrated cameras, 1 <= V <= 8, watches N persons; the session's V N slots are VIEW-MAJOR:
 * slot v N + i is person i in camera v.  The input side, LIVE ABSOLUTE ROOT and WORLD SPACE run on all slots as they are; this stage joins
 * the V slots of every person to ONE pose and ONE world root per push, on the device.  No model: the calls take the counts.  No accuracy
 * is claimed (SEVERAL VIEWS).  A push is the clock: the frames the slots received at one push are one instant, whatever their counters say.
 * STATE per person, in one caller-allocated block of uu3d_stream_views_bytes(views, persons) bytes, 256-byte aligned, zeroed by
 * uu3d_stream_views_reset: the last solved world root (3 f64), the state the person returned last, the person's tick counter.  The stage
 * READS the ring of LIVE ABSOLUTE ROOT (root_state_dev: the block of uu3d_stream_root for slots = V N, the same J and lookahead) and files
 * nothing itself; it runs in a later launch than the filing, so lookahead 0 needs no special case.
 * THE RULE.  frames_dev / active_dev / fresh_dev (V N): what uu3d_stream_root took; view_poses_dev (V N, J, 3) f32: the slots' poses in
 * world axes (uu3d_camera_to_world); cameras_dev (V, 16) f64: the rows of SEVERAL VIEWS.
 *   taking part  view v takes part in person i's tick iff its slot is active (frames >= 1) and its pose is fresh.
 *   seeing       view v sees the person iff it takes part and at least min_joints USED bytes are set in its own frame
 *                c_v = frames[slot] - 1 - lookahead >= 0 of the ring.
 *   fresh        fresh_out_dev[i] = some view takes part.  poses_dev (N, J, 3) f32 then is the fusion rule of SEVERAL VIEWS over the seeing
 *                views in ascending order, view_count_dev[i] their number; nobody sees: the mean over the views that take part,
 *                view_count 0.  The root is the root rule of SEVERAL VIEWS -- the same statements, the 2^-40 rank guard, the in-front test --
 *                over the seeing views, against the fused pose and each view's own ring frame.  Solved: roots_dev (N, 3) f32 = the root
 *                rounded once, root_state_out_dev[i] = 1, and the root is held (f64).  Not solved: the held root, state 2; no held root
 *                yet: zeros, state 0.
 *   not fresh    the pose row keeps its bits, the held root and the last state are returned, view_count 0.
 *   counter      the person's tick counter grows by one iff any of its slots is active; person_frames_dev (N) i32 is its value after
 *                this push and person_active_dev (N) u8 that flag: what the stages behind (STEADY OUTPUT) take where they take a slot's
 *                counter and active flag.
 *
 *   uu3d_stream_views_bytes(views, persons): 0 for arguments out of range (views in [1, 8], persons >= 1, views * persons <= 2^20).
 *   uu3d_stream_views(views, persons, J, lookahead, views_state_dev, root_state_dev, frames_dev, active_dev, fresh_dev, view_poses_dev,
 *       cameras_dev, min_joints, poses_dev != view_poses_dev, fresh_out_dev, roots_dev, root_state_out_dev, view_count_dev,
 *       person_frames_dev, person_active_dev, stream): one launch, one wave per person -- lane j fuses joint j with one 12-byte store, the
 *       fused pose goes through LDS to lane 0, which solves in the summation order of SEVERAL VIEWS.  views > 8 or J > 64: UU3D_ERR_UNSUPPORTED.
 *   uu3d_stream_views_reset(views, persons, views_state_dev, slot_mask_dev (V N) u8 or NULL = every slot, stream): a person ALL of whose V
 *       slots are chosen has no held root, state 0 and tick counter 0; beside uu3d_stream_reset, with the same mask.
 * Every output and state element has one writer, no atomics, the caller's buffers and the ring are only read: bitwise repeatable,
 * capturable.  Out of scope live: who is who, one clock, where rays meet, where the cameras stand, constant bone lengths on the fused pose.
 */
size_t uu3d_stream_views_bytes(int32_t views, int32_t persons);
int uu3d_stream_views(int32_t views, int32_t persons, int32_t num_keypoints, int32_t lookahead, void* views_state_dev, const void* root_state_dev,
                      const int32_t* frames_dev, const uint8_t* active_dev, const uint8_t* fresh_dev, const float* view_poses_dev,
                      const double* cameras_dev, int32_t min_joints, float* poses_dev, uint8_t* fresh_out_dev, float* roots_dev,
                      uint8_t* root_state_out_dev, uint8_t* view_count_dev, int32_t* person_frames_dev, uint8_t* person_active_dev, void* stream);
int uu3d_stream_views_reset(int32_t views, int32_t persons, void* views_state_dev, const uint8_t* slot_mask_dev, void* stream);

/*
 * STEADY OUTPUT (predict.predict_tracks(smooth=...), predict.one_euro; stream.StreamSession(smooth=...), stream.LiveOneEuro): the One-Euro
 * filter (Casiez, Roussel, Vogel 2012) over the poses and roots a call or a session returns -- an exponential smoother whose cut-off rises
 * with the speed of the signal.  No model: the calls take the channel count C and run on any (rows, C) f32 buffers.  Nothing is claimed
 * about accuracy or jitter; the filter is causal and lags -- offline, the two-pass form below takes the lag out.
 * THE RULE (predict.one_euro_host is it in numpy, bit for bit).  A CHANNEL is one scalar over time; a filter is (min_cutoff > 0, beta >= 0,
 * d_cutoff > 0) in Hz, 1 / unit speed and Hz.  Per channel the state is xh, dxh (f64) and whether a sample was taken; x is the f32 value
 * widened, r the sample rate in Hz:
 *     alpha(fc, r) = 1.0 / (1.0 + r / (6.283185307179586 * fc))
 *     first sample:   xh = x;  dxh = 0.0
 *     later samples:  dx = (x - xh) * r;  ad = alpha(d_cutoff, r);  dxh = ad * dx + (1.0 - ad) * dxh
 *                     a = alpha(min_cutoff + beta * fabs(dxh), r);  xh = a * x + (1.0 - a) * xh
 *     output = (float) xh, rounded once
 * Every operation is one IEEE f64 operation in the written order, no fused multiply-add.  r = rate / n, n the whole number of frames
 * since the channel's previous sample (offline always 1).  A non-finite x is passed through unchanged, takes no sample and touches no
 * state; so does a row whose state byte is 0 (a root that was never solved: zeros).
 *
 *   uu3d_one_euro_tracks(in_dev, out_dev (rows, C) f32, out != in, rows, C in [1, 65536] (beyond: UU3D_ERR_UNSUPPORTED), track_start_dev,
 *       track_len_dev (num_tracks) i64: the rows of each track, rates_dev (num_tracks) f64: its rate in Hz, num_tracks <= 2^20,
 *       state_dev (rows) u8 or NULL, min_cutoff, beta, d_cutoff, stream): one launch, one lane per (track, channel) walks the track's rows
 *       in order; adjacent lanes are adjacent channels of one row.  Rows of no track are not written.
 *   ZERO LAG, OFFLINE ONLY (predict.OneEuro(zero_lag=True)).  A finished track is filtered in two passes: pass 1 is the walk above and
 *   yields the f32 rows y; pass 2 is the same walk over y with the track's rows taken LAST TO FIRST -- the same rate, the same parameters,
 *   the same state bytes reversed with the rows, xh / dxh / taken fresh -- and its output, put back in row order, is the result.  A row
 *   with state 0, or a non-finite sample, is passed through unchanged by both passes and takes no sample in either; each pass takes its
 *   first usable sample as given, so a track's last usable row comes out as pass 1 left it.  The intermediate is the f32 y: per track
 *   the result is reverse(walk(reverse(walk(x)))), bit for bit (predict.one_euro_host with such a filter).  On a ramp the forward and the
 *   backward lag are one constant and cancel.  A live filter cannot do this -- it has no last row -- and the wrappers refuse it.
 *   uu3d_one_euro_tracks_two_pass(the arguments and status codes of uu3d_one_euro_tracks): one launch, the same grid; behind its forward
 *       walk the lane walks back from the track's last row to its first over the values it wrote to out_dev itself and writes the final
 *       value in place.  No scratch buffer, no atomics, every element still has one writer; in_dev is only read, out != in.
 *   LIVE.  The state block of uu3d_stream_one_euro_bytes(slots, C) bytes (0: out of range -- slots in [1, 2^20], C in [1, 65536]), 256-byte
 *   aligned, zeroed by uu3d_stream_one_euro_reset, holds per slot and channel xh, dxh, the frame index of the last sample (i32) and a TAKEN
 *   byte.  frames_dev (slots) i32 is each slot's frame counter AFTER the push; the fresh value belongs to frame f = frames - 1 - lookahead.
 *   uu3d_stream_one_euro(slots, C, lookahead, filter_state_dev, frames_dev, active_dev, fresh_dev (slots) u8, values_dev (slots, C) f32 --
 *       what the push returns, only read --, state_dev (slots) u8 or NULL, rate, min_cutoff, beta, d_cutoff, out_dev (slots, C) f32, a
 *       buffer of its own, stream): one launch, one workgroup per slot, lanes over channels.  An active slot whose value is fresh takes one
 *       sample per channel with n = f - (the frame of the channel's last sample), anything below 1 counting as 1.  Any other slot returns
 *       xh rounded once, zeros before the first sample.
 *   uu3d_stream_one_euro_reset(slots, C, filter_state_dev, slot_mask_dev (slots) u8 or NULL = every slot, stream): the chosen slots have
 *       taken no sample; beside uu3d_stream_reset, with the same mask (host-made or written on the device).
 * Every output and state element has one writer, no atomics, the caller's buffers are only read: bitwise repeatable, capturable.
 */
int uu3d_one_euro_tracks(const float* in_dev, float* out_dev, int64_t rows, int32_t channels, const int64_t* track_start_dev,
                         const int64_t* track_len_dev, const double* rates_dev, int32_t num_tracks, const uint8_t* state_dev, double min_cutoff,
                         double beta, double d_cutoff, void* stream);
int uu3d_one_euro_tracks_two_pass(const float* in_dev, float* out_dev, int64_t rows, int32_t channels, const int64_t* track_start_dev,
                                  const int64_t* track_len_dev, const double* rates_dev, int32_t num_tracks, const uint8_t* state_dev,
                                  double min_cutoff, double beta, double d_cutoff, void* stream);
size_t uu3d_stream_one_euro_bytes(int32_t slots, int32_t channels);
int uu3d_stream_one_euro(int32_t slots, int32_t channels, int32_t lookahead, void* filter_state_dev, const int32_t* frames_dev,
                         const uint8_t* active_dev, const uint8_t* fresh_dev, const float* values_dev, const uint8_t* state_dev, double rate,
                         double min_cutoff, double beta, double d_cutoff, float* out_dev, void* stream);
int uu3d_stream_one_euro_reset(int32_t slots, int32_t channels, void* filter_state_dev, const uint8_t* slot_mask_dev, void* stream);

/*
 * CONSTANT BONE LENGTHS (predict.predict_tracks(bones=...), predict.bone_lengths, predict.fix_bones; stream.StreamSession(bones=...)): the
 * network predicts every frame's skeleton on its own, so a person's bone lengths breathe from frame to frame -- and with them, under
 * ABSOLUTE ROOT POSITION, the depth.  These calls rebuild every pose from the tree root outwards with each bone scaled to ONE length per
 * track (or slot): the lengths measured over the track, or lengths the caller knows.  No model: the calls take the joint count J <= 64
 * (beyond: UU3D_ERR_UNSUPPORTED) and run on any (rows, J, 3) f32 buffers.  No accuracy figure is claimed.
 * THE TREE.  parents_dev (J) i32: the parent of every joint, -1 for the ONE tree root.  paths_dev (J, depth) i32, depth in [1, 64]: row j
 * lists the non-root joints on the way from the root down to j, j included, root side first, -1 behind the last one (the root's row is all
 * -1).  predict.Skeleton makes both.  An entry out of range ends a walk or counts as "no bone": nothing is ever read out of bounds.
 * THE RULE (predict.bone_lengths_host and predict.fix_bones_host are it in numpy, bit for bit).  All in f64, every operation rounded once in
 * the written order, no fused multiply-add, IEEE sqrt and division.  For a non-root joint j with parent p in frame f:
 *     d_c = (double) x[f][j][c] - (double) x[f][p][c];   len = sqrt((d_0 * d_0 + d_1 * d_1) + d_2 * d_2)
 *     track lengths:  L[t][j] = (sum of len over the track's frames in ascending order, only where len is finite and > 0) / (double) count;
 *                     count == 0: NaN = "not corrected";  L[t][root] = 0.  Given lengths are taken as they are; an entry that is not
 *                     finite or <= 0 means not corrected.
 *     fix:  y[root] = x[root], the input bits.  For every other joint j:  acc_c = (double) x[root][c], then for each joint a of j's path
 *           acc_c = acc_c + d_c(a) * s(a),  s(a) = L[a] / len(a) where L[a] and len(a) are finite and > 0, else 1.0;  y[j][c] = (float) acc_c.
 * Directions are kept; a NaN frame stays NaN; a zero-length bone keeps its zero offset; the root joint of a root-relative pose stays 0.
 *
 *   uu3d_bone_lengths(poses_dev (rows, J, 3) f32, rows, J, parents_dev, track_start_dev, track_len_dev (num_tracks) i64: the rows of each
 *       track, num_tracks <= 2^20, lengths_dev (num_tracks, J) f64, counts_dev (num_tracks, J) i64 or NULL, stream): one launch, one lane per
 *       (track, joint) walks the track's rows in order; adjacent lanes are adjacent joints of one row.  rows == 0: nothing is launched.
 *   uu3d_fix_bones(in_dev, out_dev (rows, J, 3) f32, out != in, rows <= 2^32, J, parents_dev, paths_dev, depth, row_track_dev (rows) i32 or
 *       NULL = track 0, num_tracks, lengths_dev (num_tracks, J) f64, stream): one launch, one lane per (row, joint) accumulates its own
 *       path.  Several lanes recompute a bone's scale; this is intended: no lane holds an array of partial positions, so the kernel uses
 *       no scratch memory.  A row whose track id is out of range is rebuilt with nothing corrected.
 *   LIVE.  The state block of uu3d_stream_bones_bytes(slots, J) bytes (0: out of range -- slots in [1, 2^20], J in [1, 64]), 256-byte
 *   aligned, zeroed by uu3d_stream_bones_reset, holds per slot and joint a sum (f64) and a count (i32).
 *   uu3d_stream_bones(slots, J, bones_state_dev, parents_dev, paths_dev, depth, active_dev, fresh_dev (slots) u8, poses_dev (slots, J, 3)
 *       f32 -- what the tick emitted, only read --, given_lengths_dev (slots, J) f64 or NULL, out_dev (slots, J, 3) f32, a buffer of its
 *       own, lengths_out_dev (slots, J) f64 or NULL, stream): one launch, one wave per slot, lane j owns joint j.  With given_lengths_dev
 *       NULL an active slot whose pose is fresh first adds its finite, positive len to the sum and increments the count; its L is then
 *       sum / (double) count.  After that EVERY slot, fresh or not, writes out = fix(poses, L of the slot): the output is a pure function
 *       of the raw pose and the slot's lengths, so a slot that holds its previous raw pose returns its previous fixed pose bit for bit.
 *       The running mean is CAUSAL -- the fresh poses seen so far -- and differs from the offline mean over the whole track, which a live
 *       session cannot know.  With given lengths the state is not touched.
 *   uu3d_stream_bones_reset(slots, J, bones_state_dev, slot_mask_dev (slots) u8 or NULL = every slot, stream): the chosen slots' sums and
 *       counts are zero; beside uu3d_stream_reset, with the same mask (host-made or written on the device).
 * Every output and state element has one writer, no atomics, the caller's buffers are only read: bitwise repeatable, capturable.
 */
int uu3d_bone_lengths(const float* poses_dev, int64_t rows, int32_t num_keypoints, const int32_t* parents_dev, const int64_t* track_start_dev,
                      const int64_t* track_len_dev, int32_t num_tracks, double* lengths_dev, int64_t* counts_dev, void* stream);
int uu3d_fix_bones(const float* in_dev, float* out_dev, int64_t rows, int32_t num_keypoints, const int32_t* parents_dev, const int32_t* paths_dev,
                   int32_t depth, const int32_t* row_track_dev, int32_t num_tracks, const double* lengths_dev, void* stream);
size_t uu3d_stream_bones_bytes(int32_t slots, int32_t num_keypoints);
int uu3d_stream_bones(int32_t slots, int32_t num_keypoints, void* bones_state_dev, const int32_t* parents_dev, const int32_t* paths_dev,
                      int32_t depth, const uint8_t* active_dev, const uint8_t* fresh_dev, const float* poses_dev,
                      const double* given_lengths_dev, float* out_dev, double* lengths_out_dev, void* stream);
int uu3d_stream_bones_reset(int32_t slots, int32_t num_keypoints, void* bones_state_dev, const uint8_t* slot_mask_dev, void* stream);

/*
 * JOINT ROTATIONS (rotations.joint_rotations, predict.predict_tracks(rotations=...), stream.StreamSession(rotations=...), bvh.write_bvh):
 * joint positions are not what a character rig, a game engine or a BVH file takes -- they take ROTATIONS.  This call turns every pose into
 * one unit quaternion (w, x, y, z; v' = q v q*) per joint: joint j's rotation relative to its parent's frame, the root's relative to the
 * pose's space, such that the REST POSE turned by them points every bone where the pose has it.  No model, no state: the call takes the
 * joint count J <= 64 (beyond: UU3D_ERR_UNSUPPORTED) and runs on any (frames, J, 3) f32 buffer.  No accuracy figure is claimed.
 * THE TABLES (rotations.Rotations makes them, uploaded once per device).  tree_dev (4, J) i32: row 0 the parents (-1: the ONE tree root),
 * row 1 every joint's PRIMARY child, row 2 its SECONDARY child (-1: none; by default the two lowest child indices), row 3 its level, the
 * number of bones between it and the root; depth: the largest level, in [0, 63].  rest_dev (J, 3) f64: the UNIT direction of the bone from
 * joint j's parent to j in the rest pose, by child joint (the root's row is not read).  An index out of range counts as "none", a joint
 * whose level is outside [0, depth] gets the identity and flag 0: nothing is ever read or written out of bounds.
 * THE RULE (rotations.joint_rotations_host is it in numpy, bit for bit; its docstring is the normative text).  All in f64, every operation
 * rounded once in the written order, no fused multiply-add, IEEE sqrt and division, no trigonometry.
 *     dot(a, b) = (a0 b0 + a1 b1) + a2 b2;   cross(a, b) = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0);   |a| = sqrt(dot(a, a))
 *     mul(a, b):  w = ((aw bw - ax bx) - ay by) - az bz;   x = ((aw bx + ax bw) + ay bz) - az by;
 *                 y = ((aw by - ax bz) + ay bw) + az bx;   z = ((aw bz + ax by) - ay bx) + az bw
 *     unit(q) = q / sqrt(((w w + x x) + y y) + z z), component by component
 *     rotate(q, v):  t = 2 cross(q.xyz, v);  v'_c = (v_c + q.w t_c) + cross(q.xyz, t)_c
 *     arc(a, b; axis) = unit((|a| |b| + dot(a, b), cross(a, b))).  ANTIPARALLEL -- the scalar part <= 0 and all three cross components
 *         == 0 --: unit((0, axis)) where an axis is given (the twist below), else unit((0, cross(a, e))), e the coordinate axis of a's
 *         smallest-magnitude component, ties to the lowest index.
 * Per frame, level by level from the root outwards; Qpar is the parent's global quaternion Q, (1, 0, 0, 0) for the root:
 *     p has no child:  Q[p] = Qpar, local = (1, 0, 0, 0) exactly, flag 1.
 *     else  b = (double) x[c1] - (double) x[p] per coordinate, c1 the primary child.  |b| not finite or not > 0 (DEGENERATE):  Q[p] = Qpar,
 *           local = (1, 0, 0, 0) exactly, flag 0.  Otherwise flag 1 and
 *           Q1 = unit(mul(arc(rotate(Qpar, rest[c1]), b), Qpar)).
 *     p has a secondary child c2:  u = b / |b|;  s = rotate(Q1, rest[c2]),  t = x[c2] - x[p];  both are projected onto the plane across
 *           the primary bone, s_c = s_c - u_c dot(s, u), t likewise.  Where both are finite and neither is all == 0:
 *           Q[p] = unit(mul(arc(s, t; u), Q1)) -- a TWIST about the primary bone, which it leaves where it is (hence the half turn of the
 *           antiparallel case about u).  Otherwise the twist is the identity, Q[p] = Q1, and the flag stays 1.
 *     local[p] = unit(mul(conj(Qpar), Q[p])), negated as a whole where w < 0, or w == 0 and the first non-zero of x, y, z is negative;
 *           then each component rounded once to f32.  global[p] = Q[p] rounded to f32, its sign as it came out.
 * WHAT THE RULE CANNOT SEE: positions do not show the twist about a bone with one child -- it is zero relative to the parent, so the
 * orientation of end segments (head, hands, feet) is limited.
 *
 *   uu3d_joint_rotations(poses_dev (frames, J, 3) f32, frames <= 2^32, J, tree_dev, depth, rest_dev, row_mask_dev (frames) u8 or NULL:
 *       a frame whose entry is 0 is left untouched -- the live session's "not fresh", local_out_dev (frames, J, 4) f32, global_out_dev
 *       (frames, J, 4) f32 or NULL, flags_out_dev (frames, J) u8 or NULL: 1 = determined from the pose, 0 = fell back, stream): one
 *       launch, one wave per frame (four frames per workgroup), lane j owns joint j; a parent's Q reaches its children through LDS.  The
 *       quaternion buffers are 16-byte aligned and written with 16-byte stores.  frames == 0: nothing is launched.
 *   uu3d_joint_rotations_reset(slots, J, local_dev, global_dev or NULL, flags_dev or NULL, slot_mask_dev (slots) u8 or NULL = every slot,
 *       stream): the chosen slots' quaternions are (1, 0, 0, 0) and their flags 0; beside uu3d_stream_reset, with the same mask.
 * LIVE: no state block.  A session's tick ends with uu3d_joint_rotations on the pose buffer push returns, row_mask_dev = fresh.
 * Every output element has one writer, no atomics, the caller's buffers are only read: bitwise repeatable, capturable.
 */
int uu3d_joint_rotations(const float* poses_dev, int64_t frames, int32_t num_keypoints, const int32_t* tree_dev, int32_t depth,
                         const double* rest_dev, const uint8_t* row_mask_dev, float* local_out_dev, float* global_out_dev,
                         uint8_t* flags_out_dev, void* stream);
int uu3d_joint_rotations_reset(int32_t slots, int32_t num_keypoints, float* local_dev, float* global_dev, uint8_t* flags_dev,
                               const uint8_t* slot_mask_dev, void* stream);

/*
 * LIVE TRACKS: END OF A TRACK (stream.StreamSession.finish): a session with lookahead a answers the push that made frame t the newest with
 * the pose of frame t - a, so a track that ENDS still owes the poses of its last a frames.  A DRAIN TICK moves the centre of the slot's
 * window one frame towards its newest frame without filing a frame: for a slot with `frames` frames the k-th drain tick (k = 1 .. a) gives
 * the pose of frame c = frames - 1 - a + k, and the frames behind the track's end are padded as the end of a video is -- the pose
 * uu3d_gather_window_frames + uu3d_forward_frames_ex give for frame c of the whole track, and the one a session of lookahead a - k returns
 * at its last push.  Everything a drain tick reads is still in the session's state: the keyframe ring covers centre - half span .. newest,
 * the edge row is the last one filed, the root ring of LIVE ABSOLUTE ROOT holds the raw frames newest - a .. newest.  Not for sessions with
 * a frame rate (their drain needs the model-rate end of the track).
 * STATE per slot, in one caller-allocated block of uu3d_stream_drain_bytes(slots) bytes, 256-byte aligned, zeroed by
 * uu3d_stream_drain_reset, apart from the session's state block (a session that never ends a track allocates none):
 * drained (i32), the drain ticks taken, at most a; virtual_frames (i32) = frames + drained, the counter the drained pose's frame is
 * counted from (c = virtual_frames - 1 - a): what uu3d_stream_one_euro takes as frames_dev in a drain tick; ticked (u8), whether the slot
 * advanced at the last drain tick.  uu3d_stream_drain_layout gives the three offsets.
 * A drain tick: uu3d_stream_drain_commit -> uu3d_forward_frames_ex and uu3d_stream_emit with the session's own arguments ->
 * uu3d_stream_root_drain -> uu3d_stream_one_euro (frames_dev = virtual_frames, active_dev = chosen) -> uu3d_stream_drain_file; then, after
 * a ticks, uu3d_stream_reset (and its companions) and uu3d_stream_drain_reset for the chosen slots.  No stage, no uu3d_frame_features.
 *
 *   uu3d_stream_drain_bytes(slots): 0 for slots outside [1, 2^20].
 *   uu3d_stream_drain_commit(model, cfg, state_dev (only read), drain_state_dev, chosen_dev (slots) u8: the slots whose tracks have ended,
 *       valid_state_dev or NULL: the validity bytes of uu3d_stream_commit_valid / uu3d_stream_commit_repair, only read, rows_dev,
 *       stride_mask_dev, fresh_dev as uu3d_stream_commit, stream): one launch, one workgroup per slot.  A chosen slot with frames >= 1 and
 *       drained < lookahead advances drained and gets the window of centre frames - 1 - lookahead + drained (fresh iff the centre is >= 0
 *       and a multiple of pred_stride); it files nothing and `frames` is unchanged.  Any other slot gets the all-masked, not-fresh window
 *       of an inactive slot.
 *   uu3d_stream_root_drain(slots, J, lookahead, root_state_dev, drain_state_dev, chosen_dev, fresh_dev, poses_dev, cameras_dev, min_joints,
 *       roots_dev, root_state_out_dev, stream): uu3d_stream_root's solve for frame c of a chosen, fresh slot, read from the ring; nothing
 *       is filed; held root and states by the same rule; any other slot returns what it returned last.  One thread per slot.
 *   uu3d_stream_drain_file(slots, lookahead >= 1, drain_state_dev, num_buffers in [1, 4], src (HOST array of num_buffers device pointers,
 *       each (slots, widths[b]) f32), widths (HOST array), dst (HOST array of device pointers, each (slots, lookahead, widths[b]) f32),
 *       fresh_dev (slots) u8 -> fresh_rows_dev (slots, lookahead) u8, root_state_dev -> root_state_rows_dev likewise or both NULL, stream):
 *       a slot that advanced at this tick copies its rows into row drained - 1; the row comes from the device counter, so the arguments
 *       are the same at every drain tick.  One launch, one workgroup per slot; any other slot writes nothing.
 *   uu3d_stream_drain_reset(slots, drain_state_dev, slot_mask_dev (slots) u8 or NULL = every slot, stream): the chosen slots have drained
 *       nothing.
 * Every output and state element has one writer, no atomics: bitwise repeatable, capturable.
 */
typedef struct uu3d_stream_drain_state_layout { int64_t drained_offset, virtual_frames_offset, ticked_offset, bytes; } uu3d_stream_drain_state_layout;
size_t uu3d_stream_drain_bytes(int32_t slots);
int uu3d_stream_drain_layout(int32_t slots, uu3d_stream_drain_state_layout* out);
int uu3d_stream_drain_commit(uu3d_model* model, const uu3d_stream_config* cfg, const void* state_dev, void* drain_state_dev,
                             const uint8_t* chosen_dev, const void* valid_state_dev, int32_t* rows_dev, uint8_t* stride_mask_dev,
                             uint8_t* fresh_dev, void* stream);
int uu3d_stream_root_drain(int32_t slots, int32_t num_keypoints, int32_t lookahead, void* root_state_dev, const void* drain_state_dev,
                           const uint8_t* chosen_dev, const uint8_t* fresh_dev, const float* poses_dev, const double* cameras_dev,
                           int32_t min_joints, float* roots_dev, uint8_t* root_state_out_dev, void* stream);
int uu3d_stream_drain_file(int32_t slots, int32_t lookahead, const void* drain_state_dev, int32_t num_buffers, const float* const* src,
                           const int32_t* widths, float* const* dst, const uint8_t* fresh_dev, uint8_t* fresh_rows_dev,
                           const uint8_t* root_state_dev, uint8_t* root_state_rows_dev, void* stream);
int uu3d_stream_drain_reset(int32_t slots, void* drain_state_dev, const uint8_t* slot_mask_dev, void* stream);

/*
 * Per-kernel timing of the next uu3d_forward calls with HIP events on the launch stream.
 * When enabled, uu3d_forward records an event pair around every launch; uu3d_profile_read
 * synchronises those events and returns the per-launch records of the LAST forward.
 */
typedef struct uu3d_profile_entry {
    char name[48];        /* launch label, e.g. "t1.ln_qkv"              */
    char kernel[32];      /* kernel family, e.g. "gemm_f32"              */
    float ms;             /* event-measured duration                      */
    double flops;         /* algorithmic FLOPs (2*MAC) of this launch     */
    double bytes;         /* algorithmic HBM bytes (operands in + out)    */
} uu3d_profile_entry;
int uu3d_set_profiling(uu3d_model* model, int32_t enabled);
int uu3d_profile_read(uu3d_model* model, uu3d_profile_entry* out_entries, int32_t capacity,
                      int32_t* out_count);

/* ------------------------------------------------------------------------------------------
 * The training step: loss, optimizer and EMA kernels first, then the
 * training-mode forward + backward pass (T2, uu3d_train_forward_backward).
 * ------------------------------------------------------------------------------------------ */

/*
 * T1 -- replaces the loss of train_step (train.py:464-494, common/utils/losses_3d.py:13-14):
 *   gt      = gt3d - gt3d[:, :, root]                 (root shift, :467)
 *   central = sum ||pred_central - gt[:, N/2]||_2 / (batch_size_norm * J)
 *   seq     = sum ||pred_full    - gt        ||_2 / (batch_size_norm * N * J)
 *   loss    = w_center * central + w_seq * seq        (pred_full_dev == NULL: (w_center + w_seq) * central, :491-494)
 * and returns d loss / d pred (what tape.gradient feeds into the network's backward).
 *   pred_full_dev (B,N,J,3) or NULL, pred_central_dev (B,J,3), gt3d_dev (B,N,J,3) absolute 3D poses.
 *   batch_size_norm is config.BATCH_SIZE (the GLOBAL batch: per-rank sums simply add up).
 *   loss_out_dev[3] = {loss, central, seq}; grad_* may be NULL; scratch_dev >= 4096 floats.
 * Deterministic (fixed-order two-stage reduction).
 */
int uu3d_mpjpe_loss(const float* pred_full_dev, const float* pred_central_dev, const float* gt3d_dev,
                    int32_t batch, int32_t num_frames, int32_t num_keypoints, int32_t root_index,
                    float w_center, float w_seq, int32_t batch_size_norm,
                    float* loss_out_dev, float* grad_full_dev, float* grad_central_dev,
                    float* scratch_dev, void* stream);

/*
 * T3 -- replaces optimizer.apply_gradients for tfa.optimizers.AdamW (train.py:404-415,499) on
 * one flat parameter buffer: decoupled decay first, then the Keras/TF ApplyAdam update
 *   var -= wd * var
 *   alpha = lr * sqrt(1 - beta2^t) / (1 - beta1^t)              (t = step = iterations + 1)
 *   m += (g - m) * (1 - beta1);  v += (g*g - v) * (1 - beta2)
 *   var -= (m * alpha) / (sqrt(v) + epsilon)
 * vhat_dev != NULL selects Keras Adam's amsgrad=True form (TF ApplyAdamWithAmsgrad; the config class default
 * OPTIMIZER_PARAMS {"amsgrad": True}, uplift_upsample_transformer_config.py:88):
 *   vhat = max(vhat, v);  var -= (m * alpha) / (sqrt(vhat) + epsilon)
 * lr and wd are the schedule values at `iterations` (both ExponentialDecay for the shipped configs).
 * HBM-bound: 28 bytes per parameter (read var, g, m, v; write var, m, v), 36 with vhat.
 */
int uu3d_adamw_update(float* var_dev, float* m_dev, float* v_dev, float* vhat_dev, const float* grad_dev, int64_t n,
                      float lr, float wd, float beta1, float beta2, float epsilon, int64_t step,
                      void* stream);
/* The same update, skipped ON THE DEVICE (weights and moments untouched) when *skip_flag_dev != 0 -- no host synchronisation.
 * skip_flag_dev = uu3d_train_nonfinite_flag(model): uu3d_train_forward_backward clears it and its loss-scaled backward pass
 * (f16x3 gradient GEMMs, train.py:477,498 replaced) raises it when a finished gradient range holds a non-finite value; NULL =
 * uu3d_adamw_update.  A skipped step keeps TF's semantics of "no update" only approximately: the host-side iteration counter
 * (bias correction, schedules) still advances. */
int uu3d_adamw_update_guarded(float* var_dev, float* m_dev, float* v_dev, float* vhat_dev, const float* grad_dev, int64_t n,
                              float lr, float wd, float beta1, float beta2, float epsilon, int64_t step,
                              const uint32_t* skip_flag_dev, void* stream);
/* Device address of the model's non-finite-gradient word (valid after uu3d_train_init, until the next uu3d_train_init /
 * uu3d_destroy); NULL without training state. */
uint32_t* uu3d_train_nonfinite_flag(const uu3d_model* model);
/* Host-side read of that word (synchronises the device): *out = 1 when the last backward pass flagged non-finite gradients. */
int uu3d_train_nonfinite(uu3d_model* model, int32_t* out);


/* T4 -- replaces the EMA update of train_step (train.py:502-504): ema -= (1 - decay) * (ema - w). */
int uu3d_ema_update(float* ema_dev, const float* w_dev, int64_t n, float decay, void* stream);

/*
 * T2 -- replaces `with tf.GradientTape(): model(..., training=True)` + `tape.gradient(loss, model.trainable_variables)`
 * (train.py:477-498).  The optimizer owns ONE flat float32 master buffer of all parameters in inventory order,
 * Keras layouts (uu3d_num_params floats); gradients are returned in a buffer of the same layout.
 *   uu3d_train_init     uploads the model's current weights into params_dev and builds the device-side operand packs
 *   uu3d_train_repack   regenerates the packs from params_dev (call after every optimizer step)
 *   uu3d_train_export   params_dev -> host weights -> inference operands (so uu3d_forward evaluates the trained model)
 *   uu3d_train_forward_backward: training-mode forward (DropPath, vision_transformer.py:16-43), the loss of
 *       uu3d_mpjpe_loss, and the full backward pass.
 *       drop_path_rates[3] = DROP_PATH_RATE (spatial, temporal, strided); per block rate linspace(0, rate, depth)
 *       drop_path_uniform_dev: U[0,1) draws, layout [spatial blocks][2][B*N] then [temporal blocks][2][B]
 *                              (two draws per block: attention branch, MLP branch); NULL disables DropPath.
 *       full_out_dev / central_out_dev may be NULL.  loss_out_dev[3] = {loss, central, sequence}.  Without the full-sequence head
 *       (temporal_depth == 0) full_out_dev is not written, loss = (w_center + w_seq) * central (train.py:491-494) and sequence = 0.
 *       gt3d_dev == NULL: training-mode FORWARD ONLY (model(inputs, training=True) outside a tape, train.py:478);
 *       loss_out_dev / grads_dev may then be NULL.  drop_path_rates[2] != 0: DropPath inside the strided blocks, its draws behind the
 *       temporal stack's ([strided blocks][2][B]).
 *       uu3d_config.output_bn: the heads' BatchNormalization runs in TRAINING mode (uplift_upsample_transformer.py:275-285: batch mean
 *       and biased variance of the head's input over all rows) and -- the one exception to `const` -- the moving statistics, the last
 *       tensors of params_dev, are updated in place (moving = 0.1 moving + 0.9 batch), as Keras does inside the training-mode call; they are
 *       not trainable: their slots of grads_dev are zeros and the optimizer must leave them alone (trainer.Trainer steps the prefix in
 *       front of them).
 *   uu3d_train_set_grad_callback: `fn(user, first, count, stream)` is called on the calling host thread from inside
 *       uu3d_train_forward_backward each time the range [first, first + count) of grads_dev is final; every kernel that
 *       writes it has been enqueued on `stream` before the call (a bucketed all-reduce makes its communication stream wait
 *       for `stream` and overlaps with the rest of the backward pass).  Ranges are disjoint and cover the buffer.
 */
typedef void (*uu3d_grad_ready_fn)(void* user, int64_t first, int64_t count, void* stream);
int uu3d_train_set_grad_callback(uu3d_model* model, uu3d_grad_ready_fn fn, void* user);
/*
 * The Dropout layers of the model in TRAINING mode (config DROP_RATE / ATTENTION_DROP_RATE: kl.Dropout in
 * common/net/vision_transformer.py:57-58,63-67 (MLP: behind the activation and behind fc2), :87-90,127-128 (attention weights),
 * :153-154 (projection output); common/net/uplift_upsample_transformer.py:78-79,84-89 (StridedMLP), :201,324 (token_dropout behind
 * the keypoint embedding + positional encoding)).  Applies to the following uu3d_train_forward_backward* calls of this model
 * (forward-only calls included) until changed; rates 0 (the default, and every shipped config) = no layer.  An element is kept iff
 * u >= rate, kept elements are scaled by 1 / (1 - rate) (Keras); u is a counter-based function of (seed, layer site, element
 * index) -- csrc/uu3d_dropout.h lists the sites -- so the backward pass recomputes the masks instead of storing them and a CPU
 * restatement can evaluate the same masks (oracle/dropout_oracle.py).  Give every step a fresh seed.  With a rate > 0 the
 * spatial stack runs as its unfused chain of launches and attention on the generic kernels (the fused / MFMA kernels have no
 * Dropout sites): correct, slower.
 */
int uu3d_train_set_dropout(uu3d_model* model, float drop_rate, float attention_drop_rate, uint64_t seed);
int64_t uu3d_num_params(const uu3d_model* model);
int uu3d_train_init(uu3d_model* model, float* params_dev, void* stream);
int uu3d_train_repack(uu3d_model* model, const float* params_dev, void* stream);
int uu3d_train_export(uu3d_model* model, const float* params_dev, void* stream);
size_t uu3d_train_workspace_bytes(const uu3d_model* model, int32_t batch);
int uu3d_train_forward_backward(uu3d_model* model, const float* params_dev, const float* kp2d_dev,
                                const uint8_t* stride_mask_dev, const float* gt3d_dev, int32_t batch,
                                int32_t batch_size_norm, float w_center, float w_seq, int32_t root_index,
                                const float* drop_path_rates, const float* drop_path_uniform_dev,
                                float* loss_out_dev, float* full_out_dev, float* central_out_dev,
                                float* grads_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* The same step with random token masking (uplift_upsample_transformer.py:287-311, 336-338; TOKEN_MASK_RATE > 0): token (b, n) entering the temporal transformer -- spatial_to_temporal_fc's output, before the
 * strided-input token blend and the positional encoding -- is replaced by 0 (by the learnable masked token when the model was
 * created with uu3d_config.learnable_masked_token, whose gradient is the sum of d x over the replaced rows) where
 * token_mask_uniform_dev[b * N + n] < token_mask_rate, never at the central frame n = N / 2.  token_mask_uniform_dev: B * N draws of U[0, 1) (the caller's generator,
 * like drop_path_uniform_dev); NULL or rate 0: no masking (= uu3d_train_forward_backward). */
int uu3d_train_forward_backward_masked(uu3d_model* model, const float* params_dev, const float* kp2d_dev,
                                       const uint8_t* stride_mask_dev, const float* gt3d_dev, int32_t batch,
                                       int32_t batch_size_norm, float w_center, float w_seq, int32_t root_index,
                                       const float* drop_path_rates, const float* drop_path_uniform_dev,
                                       const float* token_mask_uniform_dev, float token_mask_rate,
                                       float* loss_out_dev, float* full_out_dev, float* central_out_dev,
                                       float* grads_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/*
 * GradientTape -- the training step with the loss left to the caller (autograd: `loss.backward()` through model(..., training=True)).
 *   uu3d_train_forward_tape: the training-mode forward of uu3d_train_forward_backward_masked (same arguments, same draws and Dropout)
 *       that keeps its activations in the workspace and returns a tape instead of running a loss.  It makes every up-front check of
 *       the backward pass (token limits -- 416 at head dim 48, see uu3d_create --, LDS of the backward attention kernels), so the tape's backward is never refused.  The models
 *       the training step refuses are refused with the same messages.
 *   uu3d_train_backward_tape: the backward pass of that forward, seeded with d loss / d full_output (B,N,J,3) and
 *       d loss / d central_output (B,J,3) supplied by the caller (NULL = 0; without the full-sequence head -- temporal_depth == 0, where the
 *       tape's forward takes full_out_dev == NULL -- grad_full_dev must be NULL: UU3D_ERR_INVALID_ARGUMENT otherwise).  grads_dev (uu3d_num_params floats, inventory order) is
 *       OVERWRITTEN with d loss / d params; NULL = not wanted.  grad_kp2d_dev (B,N,J,2), or NULL, receives d loss / d kp2d_dev; rows of
 *       frames the stride mask (or the token mask) discards are exactly 0.  The cotangents are multiplied on the device by a power of
 *       two that puts their largest magnitude into (0.5, 1] (loss scaling without a host synchronisation) and the results unscaled.
 *       A non-finite cotangent or gradient RAISES the model's non-finite word (uu3d_train_nonfinite_flag); it is never cleared here, so
 *       several backward passes before one optimizer step accumulate it.  uu3d_train_clear_nonfinite clears it.  The grad-ready
 *       callback is not called.  A backward may run once or several times per tape.
 *   The caller keeps params_dev, kp2d_dev, stride_mask_dev, the draws and the WORKSPACE alive and unchanged from the forward until the
 *       last backward of a tape (the saved activations live in the workspace): one workspace per open tape; several tapes with
 *       separate workspaces may be open at once.  The tape records batch, buffers and the Dropout rates and seed of its forward
 *       (uu3d_train_set_dropout may change them before the backward).  If another call has regenerated the operand packs from a
 *       different parameter buffer in between, the backward regenerates them first.
 *   uu3d_tape_destroy frees the tape (not the caller's buffers); call it when no backward will follow.
 */
typedef struct uu3d_tape uu3d_tape;
int uu3d_train_forward_tape(uu3d_model* model, const float* params_dev, const float* kp2d_dev, const uint8_t* stride_mask_dev, int32_t batch,
                            const float* drop_path_rates, const float* drop_path_uniform_dev,
                            const float* token_mask_uniform_dev, float token_mask_rate,
                            float* full_out_dev, float* central_out_dev,
                            void* workspace_dev, size_t workspace_bytes, uu3d_tape** out_tape, void* stream);
int uu3d_train_backward_tape(uu3d_model* model, uu3d_tape* tape, const float* grad_full_dev, const float* grad_central_dev,
                             float* grads_dev, float* grad_kp2d_dev, void* stream);
void uu3d_tape_destroy(uu3d_tape* tape);
/* Clears the model's non-finite-gradient word on `stream` (what a new accumulation of tape backward passes starts from). */
int uu3d_train_clear_nonfinite(uu3d_model* model, void* stream);
/* Copies the model's non-finite-gradient word into the caller's device word out_dev on `stream` (no host synchronisation): what a
 * data-parallel caller combines over ranks before the guarded optimizer update. */
int uu3d_train_copy_nonfinite(uu3d_model* model, uint32_t* out_dev, void* stream);

/*
 * GradientTape over several ranks -- the tape backward for data-parallel training (DDP-like: collectives start while it runs).
 *   uu3d_train_backward_tape_accumulate: the backward pass of uu3d_train_backward_tape (same tape rules, same kernels, same
 *       cotangent scaling).  It writes the loss-scaled parameter gradients into grads_scratch_dev (uu3d_num_params floats, contents
 *       undefined afterwards) and, as each contiguous range of the inventory is final, ADDS that range unscaled into
 *       grads_accum_dev: grads_accum[i] = grads_accum[i] + g[i] * s, multiply and add rounded separately, so the result is bit for
 *       bit what uu3d_train_backward_tape's gradients added to grads_accum afterwards give.  A non-finite unscaled gradient or
 *       cotangent raises the non-finite word as there.  report_ranges != 0: after each range's add the grad-ready callback
 *       (uu3d_train_set_grad_callback) receives (first, count) and the stream the add ran on, as in uu3d_train_forward_backward;
 *       the reported ranges tile [0, uu3d_num_params) exactly once per call.  report_ranges == 0: no callback (local accumulation
 *       of micro-batches).  grad_kp2d_dev as in uu3d_train_backward_tape.  A NULL handle, tape, grads_scratch_dev or
 *       grads_accum_dev, or the two buffers overlapping, is refused with UU3D_ERR_INVALID_ARGUMENT before anything is enqueued.
 */
int uu3d_train_backward_tape_accumulate(uu3d_model* model, uu3d_tape* tape, const float* grad_full_dev, const float* grad_central_dev,
                                        float* grads_scratch_dev, float* grads_accum_dev, float* grad_kp2d_dev,
                                        int32_t report_ranges, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UU3D_H_ */
