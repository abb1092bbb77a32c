"""ctypes binding of ``include/uu3d.h`` (the C-ABI shared library ``csrc/libuu3d.so``).

There is NO fallback: if the HIP library is missing or fails to load, importing a symbol
raises ``Uu3dLibraryError`` -- the product path never computes on the CPU.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (UU3D_LIB: another build of the same library, e.g. csrc/libuu3d_timing.so of `build.py --timing` for the marginal-cost experiments of tools/)
LIB_PATH = os.environ.get("UU3D_LIB") or os.path.join(_HERE, "csrc", "libuu3d.so")

UU3D_MAX_STRIDED = 8
UU3D_PREC_F32 = 0
UU3D_PREC_F16X3 = 1

(UU3D_OK, UU3D_ERR_INVALID_ARGUMENT, UU3D_ERR_UNSUPPORTED, UU3D_ERR_SHAPE, UU3D_ERR_NOT_READY,
 UU3D_ERR_WORKSPACE, UU3D_ERR_HIP, UU3D_ERR_NO_DEVICE, UU3D_ERR_RANGE) = range(9)
UU3D_SCHEDULE_LATENCY, UU3D_SCHEDULE_THROUGHPUT, UU3D_SCHEDULE_EXACT_F32 = 0, 1, 0x100

# every symbol include/uu3d.h declares
EXPORTED_SYMBOLS = (
    "uu3d_version", "uu3d_status_string", "uu3d_last_error", "uu3d_create", "uu3d_destroy",
    "uu3d_num_weights", "uu3d_weight_info", "uu3d_set_weight", "uu3d_get_weight",
    "uu3d_commit_weights", "uu3d_workspace_bytes", "uu3d_forward", "uu3d_forward_attention", "uu3d_forward_ex", "uu3d_range_status", "uu3d_mpjpe",
    "uu3d_set_schedule", "uu3d_set_profiling", "uu3d_profile_read", "uu3d_gather_windows", "uu3d_world_to_cam_2d",
    "uu3d_mpjpe_loss", "uu3d_adamw_update", "uu3d_adamw_update_guarded", "uu3d_train_nonfinite_flag", "uu3d_train_nonfinite", "uu3d_ema_update",
    "uu3d_num_params", "uu3d_train_init", "uu3d_train_repack", "uu3d_train_export",
    "uu3d_train_workspace_bytes", "uu3d_train_forward_backward", "uu3d_train_forward_backward_masked", "uu3d_train_set_grad_callback", "uu3d_train_set_dropout",
    "uu3d_train_forward_tape", "uu3d_train_backward_tape", "uu3d_tape_destroy", "uu3d_train_clear_nonfinite",
    "uu3d_train_backward_tape_accumulate", "uu3d_train_copy_nonfinite",
    "uu3d_frame_features_bytes", "uu3d_frame_features", "uu3d_gather_window_frames", "uu3d_forward_frames_ex",
    "uu3d_pose_errors", "uu3d_error_sums", "uu3d_error_sums_scratch_bytes",
    "uu3d_normalize_tracks", "uu3d_assemble_tracks",
    "uu3d_stream_state_bytes", "uu3d_stream_state_layout", "uu3d_stream_stage", "uu3d_stream_commit", "uu3d_stream_emit", "uu3d_stream_reset",
    "uu3d_normalize_tracks_valid", "uu3d_gather_windows_valid", "uu3d_gather_window_frames_valid", "uu3d_stream_valid_bytes",
    "uu3d_stream_stage_valid", "uu3d_stream_commit_valid",
    "uu3d_resample_tracks",
    "uu3d_repair_joints", "uu3d_repair_joints_scratch_bytes",
    "uu3d_stream_rate_state_layout", "uu3d_stream_source_push", "uu3d_stream_resample_stage", "uu3d_stream_file_keyframe",
    "uu3d_stream_timed_emit", "uu3d_stream_rate_reset",
    "uu3d_stream_out_state_layout", "uu3d_stream_timed_emit_multi", "uu3d_stream_out_reset",
    "uu3d_stream_repair_bytes", "uu3d_stream_repair_layout", "uu3d_stream_repair_stage", "uu3d_stream_commit_repair", "uu3d_stream_repair_reset",
    "uu3d_keypoint_map_bytes", "uu3d_keypoint_map_pack", "uu3d_map_keypoints",
    "uu3d_associate_state_bytes", "uu3d_associate_reset", "uu3d_associate_detections", "uu3d_stream_associate",
    "uu3d_solve_roots", "uu3d_root_trajectory_scratch_bytes", "uu3d_root_trajectory",
    "uu3d_stream_root_bytes", "uu3d_stream_root", "uu3d_stream_root_reset",
    "uu3d_one_euro_tracks", "uu3d_one_euro_tracks_two_pass", "uu3d_stream_one_euro_bytes", "uu3d_stream_one_euro", "uu3d_stream_one_euro_reset",
    "uu3d_stream_drain_bytes", "uu3d_stream_drain_layout", "uu3d_stream_drain_commit", "uu3d_stream_root_drain", "uu3d_stream_drain_file",
    "uu3d_stream_drain_reset",
    "uu3d_bone_lengths", "uu3d_fix_bones", "uu3d_stream_bones_bytes", "uu3d_stream_bones", "uu3d_stream_bones_reset",
    "uu3d_joint_rotations", "uu3d_joint_rotations_reset",
    "uu3d_assemble_tracks_cubic",
    "uu3d_stream_timed_emit_cubic", "uu3d_stream_timed_emit_multi_cubic",
    "uu3d_undistort_points",
    "uu3d_camera_to_world",
    "uu3d_fuse_views", "uu3d_solve_view_roots",
    "uu3d_view_pair_sums", "uu3d_group_views", "uu3d_gather_view_tracks",
    "uu3d_view_lag_scratch_bytes", "uu3d_view_lag_sums", "uu3d_view_offsets",
    "uu3d_triangulate_joints", "uu3d_place_joints",
    "uu3d_view_calibrate_chunks", "uu3d_view_moment_sums", "uu3d_view_position_sums", "uu3d_solve_view_pose",
    "uu3d_lift_pair_sums",
    "uu3d_stream_views_bytes", "uu3d_stream_views", "uu3d_stream_views_reset",
)
# include/uu3d_ops.h
OPS_SYMBOLS = (
    "uu3d_op_gemm_tn", "uu3d_op_gemm_tn_h3", "uu3d_op_gemm_nt", "uu3d_op_colsum", "uu3d_op_row_stats", "uu3d_op_ln_bwd",
    "uu3d_op_attn_fwd", "uu3d_op_attn_bwd", "uu3d_op_attn_long_fwd", "uu3d_op_attn_long_bwd", "uu3d_op_attn_long_infer", "uu3d_op_scratch_floats",
    "uu3d_op_panel_operand_bytes", "uu3d_op_panel_a_bytes", "uu3d_op_panel_pack", "uu3d_op_ln_dense_panel",
    "uu3d_op_ln_dense_panel_ex", "uu3d_op_panel_a_unpack", "uu3d_op_mlp_operand_bytes", "uu3d_op_mlp_pack", "uu3d_op_mlp_fused",
    "uu3d_op_wt_operand_bytes", "uu3d_op_wt_pack", "uu3d_op_ln_dense_wt",
    "uu3d_op_attn_infer", "uu3d_op_attn_qf_bytes", "uu3d_op_attn_qf_pack",
    "uu3d_op_tiled_operand_bytes", "uu3d_op_tiled_pack", "uu3d_op_tiled_dense", "uu3d_op_tiled_split",
    "uu3d_op_spatial_stack", "uu3d_op_compact_frames", "uu3d_op_spatial_choice",
    "uu3d_op_panel_a_pack", "uu3d_op_attn_qf_unpack",
    "uu3d_op_tchain", "uu3d_op_tchain_scratch_bytes", "uu3d_op_tchain_launches", "uu3d_op_tchain_xs_pack", "uu3d_op_tchain_xs_unpack",
    "uu3d_op_train_operand_bytes", "uu3d_op_train_pack", "uu3d_op_train_dense", "uu3d_op_train_wgrad", "uu3d_op_colsum3", "uu3d_op_ln_bwd_ex",
    "uu3d_op_identity_bwd", "uu3d_op_scale_rows",
)
# epilogues of uu3d_op_ln_dense_panel_ex / uu3d_op_ln_dense_wt (include/uu3d_ops.h)
UU3D_EP_BIAS, UU3D_EP_BIAS_RELU_SPLIT, UU3D_EP_BIAS_SPLIT_Q, UU3D_EP_BIAS_RESIDUAL, UU3D_EP_BIAS_RESIDUAL_LN = range(5)
# kernels and layouts of uu3d_op_attn_infer (include/uu3d_ops.h)
UU3D_ATTN_AUTO, UU3D_ATTN_F32_WG, UU3D_ATTN_HEAD_WAVE, UU3D_ATTN_H3 = range(4)
UU3D_ATTN_IN_F32, UU3D_ATTN_IN_PLANES, UU3D_ATTN_IN_QFRAG = range(3)
UU3D_ATTN_OUT_F32, UU3D_ATTN_OUT_PLANES, UU3D_ATTN_OUT_FRAG = range(3)
# A sources and further epilogues of uu3d_op_tiled_dense (include/uu3d_ops.h)
UU3D_A_F32, UU3D_A_F32_LN, UU3D_A_PLANES, UU3D_A_CONV3_F32, UU3D_A_CONV3_PLANES = range(5)
UU3D_EP_BIAS_RELU, UU3D_EP_CONV_RESIDUAL, UU3D_EP_S2T = 5, 6, 7
# kernels and output layouts of uu3d_op_spatial_stack (include/uu3d_ops.h)
UU3D_SPATIAL_AUTO, UU3D_SPATIAL_F32, UU3D_SPATIAL_H3_TILES, UU3D_SPATIAL_P16 = range(4)
UU3D_SPATIAL_OUT_F32, UU3D_SPATIAL_OUT_PLANES = range(2)
# stage sets of the temporal chain's launches (uu3d_op_tchain, include/uu3d_ops.h)
UU3D_TC_PROJ, UU3D_TC_MLP, UU3D_TC_QKV, UU3D_TC_FC1_PLANES, UU3D_TC_PE = 1, 2, 4, 8, 16
# A sources and epilogues of uu3d_op_train_dense / uu3d_op_train_wgrad (include/uu3d_ops.h)
UU3D_TA_PLAIN, UU3D_TA_LN, UU3D_TA_GELU, UU3D_TA_CONV3, UU3D_TA_CONVT = range(5)
(UU3D_TEP_STORE, UU3D_TEP_BIAS, UU3D_TEP_BIAS_RELU, UU3D_TEP_BIAS_RES_GATE, UU3D_TEP_ADD, UU3D_TEP_RELU_MASK, UU3D_TEP_GELU_GRAD,
 UU3D_TEP_CONV_RESIDUAL) = range(8)
UU3D_WEP_STORE, UU3D_WEP_STORE3 = range(2)


class Uu3dTiledDenseArgs(C.Structure):
    """``uu3d_tiled_dense_args`` of include/uu3d_ops.h."""
    _fields_ = ([(n, C.c_void_p) for n in ("a_dev", "a_lo_dev", "ln_stats_dev", "ln_gamma_dev", "ln_beta_dev", "operand_dev", "bias_dev", "out_dev", "out2_dev",
                                           "xin_dev", "pe_dev", "token_dev", "mask_dev", "slab_dev")]
                + [("slab_floats", C.c_size_t)]
                + [(n, C.c_int32) for n in ("a_source", "epilogue", "precision", "splitk_target", "M", "N", "K", "lda", "ldo",
                                            "conv_C", "conv_L_in", "conv_L_out", "conv_stride", "conv_pad_left", "period")]
                + [("qscale", C.c_float)])


class Uu3dTrainDenseArgs(C.Structure):
    """``uu3d_train_dense_args`` of include/uu3d_ops.h."""
    _fields_ = ([(n, C.c_void_p) for n in ("a_dev", "ln_stats_dev", "ln_gamma_dev", "ln_beta_dev", "operand_dev", "bias_dev", "out_dev", "out2_dev",
                                           "aux_dev", "pe_dev", "gate_dev", "slab_dev")]
                + [("slab_floats", C.c_size_t), ("drop_seed", C.c_uint64)]
                + [(n, C.c_int32) for n in ("a_source", "epilogue", "precision", "operand_kind", "M", "N", "K", "lda", "ldo",
                                            "conv_C", "conv_L_in", "conv_L_out", "conv_stride", "conv_pad_left", "rps", "period")]
                + [("drop_site", C.c_uint32)]
                + [(n, C.c_float) for n in ("keep", "scale", "drop_rate")])


class Uu3dTrainWgradArgs(C.Structure):
    """``uu3d_train_wgrad_args`` of include/uu3d_ops.h."""
    _fields_ = ([(n, C.c_void_p) for n in ("a_dev", "ln_stats_dev", "ln_gamma_dev", "ln_beta_dev", "b_dev", "out_dev", "out1_dev", "out2_dev", "slab_dev")]
                + [("slab_floats", C.c_size_t)]
                + [(n, C.c_int32) for n in ("a_source", "epilogue", "h3", "R", "P", "Q", "lda", "ldb", "ldo",
                                            "conv_C", "conv_L_in", "conv_L_out", "conv_stride", "conv_pad_left")])


class Uu3dLibraryError(RuntimeError):
    pass


class Uu3dError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"uu3d status {status}: {message}")
        self.status = status


class Uu3dRangeError(Uu3dError):
    """A forward produced non-finite outputs: activations left the f16 range of the f16x3 products (include/uu3d.h, RANGE CONTRACT)."""


class Uu3dConfig(C.Structure):
    _fields_ = [
        ("num_frames", C.c_int32), ("num_keypoints", C.c_int32),
        ("d_spatial", C.c_int32), ("d_temporal", C.c_int32),
        ("h_spatial", C.c_int32), ("h_temporal", C.c_int32),
        ("spatial_depth", C.c_int32), ("temporal_depth", C.c_int32),
        ("num_strided", C.c_int32),
        ("strides", C.c_int32 * UU3D_MAX_STRIDED),
        ("pad_left", C.c_int32 * UU3D_MAX_STRIDED),
        ("pad_right", C.c_int32 * UU3D_MAX_STRIDED),
        ("num_heads", C.c_int32), ("qkv_bias", C.c_int32), ("has_strided_input", C.c_int32),
        ("first_strided_token_attention_layer", C.c_int32), ("full_output", C.c_int32),
        ("precision", C.c_int32), ("output_bn", C.c_int32), ("learnable_masked_token", C.c_int32),
    ]


class Uu3dProfileEntry(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("kernel", C.c_char * 32), ("ms", C.c_float),
                ("flops", C.c_double), ("bytes", C.c_double)]


class Uu3dStreamConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("slots", "seq_stride", "mask_stride", "pred_stride", "lookahead", "flip", "pad_edge", "root_index")]


class Uu3dStreamLayout(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("ring_capacity", "table_rows", "zero_row", "frames_offset", "held_offset", "table_offset", "bytes")]


class Uu3dStreamRate(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("a", "b", "lookahead", "key_ring")]


class Uu3dStreamRateLayout(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("source_frames_offset", "pushed_offset", "source_valid_offset", "source_offset", "keys_offset",
                                         "key_stride", "out_held_offset", "bytes")]


class Uu3dStreamOut(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("c", "d", "pos_num", "pos_den", "max_out")]


class Uu3dStreamOutLayout(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("out_frames_offset", "bytes")]


class Uu3dStreamRepairLayout(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("window", "staged_frames", "raw_offset", "last_xy_offset", "last_offset", "held_offset", "observed_offset",
                                         "bytes")]


class Uu3dStreamDrainLayout(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("drained_offset", "virtual_frames_offset", "ticked_offset", "bytes")]


class Uu3dAssociateParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("slots", "detections", "keypoints", "max_age", "min_common", "reserved")] + [("max_dist", C.c_double)]


# void (*uu3d_grad_ready_fn)(void* user, int64_t first, int64_t count, void* stream)
GRAD_READY_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p)

_lib = None


def load_library(path=None):
    """dlopen the HIP library and declare every prototype.  Raises if it is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise Uu3dLibraryError(
            f"{p} not found: build it with `python __graft_entry__.py build` "
            f"(hipcc --offload-arch=gfx950); there is no CPU fallback")
    try:
        lib = C.CDLL(p)
    except OSError as e:  # pragma: no cover
        raise Uu3dLibraryError(f"cannot load {p}: {e}") from e
    vp, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
    lib.uu3d_version.restype = C.c_char_p
    lib.uu3d_version.argtypes = []
    lib.uu3d_status_string.restype = C.c_char_p
    lib.uu3d_status_string.argtypes = [C.c_int]
    lib.uu3d_last_error.restype = C.c_char_p
    lib.uu3d_last_error.argtypes = [vp]
    lib.uu3d_create.restype = C.c_int
    lib.uu3d_create.argtypes = [C.POINTER(Uu3dConfig), C.c_int, C.POINTER(vp)]
    lib.uu3d_destroy.restype = None
    lib.uu3d_destroy.argtypes = [vp]
    lib.uu3d_num_weights.restype = C.c_int
    lib.uu3d_num_weights.argtypes = [vp]
    lib.uu3d_weight_info.restype = C.c_int
    lib.uu3d_weight_info.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(i32), C.POINTER(i64 * 4)]
    lib.uu3d_set_weight.restype = C.c_int
    lib.uu3d_set_weight.argtypes = [vp, C.c_char_p, vp, i64]
    lib.uu3d_get_weight.restype = C.c_int
    lib.uu3d_get_weight.argtypes = [vp, C.c_char_p, vp, i64]
    lib.uu3d_commit_weights.restype = C.c_int
    lib.uu3d_commit_weights.argtypes = [vp, vp]
    lib.uu3d_workspace_bytes.restype = sz
    lib.uu3d_workspace_bytes.argtypes = [vp, i32]
    lib.uu3d_forward.restype = C.c_int
    lib.uu3d_forward.argtypes = [vp, vp, vp, i32, vp, vp, vp, sz, vp]
    lib.uu3d_forward_attention.restype = C.c_int
    lib.uu3d_forward_attention.argtypes = [vp, vp, vp, i32, vp, vp, C.POINTER(vp), vp, sz, vp]
    lib.uu3d_forward_ex.restype = C.c_int
    lib.uu3d_forward_ex.argtypes = [vp, vp, vp, i32, vp, vp, C.POINTER(vp), vp, sz, i32, vp]
    lib.uu3d_range_status.restype = C.c_int
    lib.uu3d_range_status.argtypes = [vp, vp, C.POINTER(i32)]
    lib.uu3d_mpjpe.restype = C.c_int
    lib.uu3d_mpjpe.argtypes = [vp, vp, i32, i32, i32, vp, vp]
    lib.uu3d_pose_errors.restype = C.c_int
    lib.uu3d_pose_errors.argtypes = [vp, i64, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp, vp, i32, vp, vp, vp, sz, vp]
    lib.uu3d_error_sums.restype = C.c_int
    lib.uu3d_error_sums.argtypes = [vp, i64, i32, vp, i32, vp, vp, vp, sz, vp]
    lib.uu3d_error_sums_scratch_bytes.restype = sz
    lib.uu3d_error_sums_scratch_bytes.argtypes = [i64, i32]
    lib.uu3d_gather_windows.restype = C.c_int
    lib.uu3d_gather_windows.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp]
    lib.uu3d_normalize_tracks.restype = C.c_int
    lib.uu3d_normalize_tracks.argtypes = [vp, i64, vp, i64, i32, vp, i32, vp, vp, vp, i32, vp]
    lib.uu3d_assemble_tracks.restype = C.c_int
    lib.uu3d_assemble_tracks.argtypes = [vp, vp, i64, vp, vp, vp, vp, i64, i32, i32, vp, vp]
    lib.uu3d_assemble_tracks_cubic.restype = C.c_int
    lib.uu3d_assemble_tracks_cubic.argtypes = [vp, vp, i64, vp, vp, vp, vp, vp, vp, i64, i32, i32, vp, vp]
    lib.uu3d_frame_features_bytes.restype = sz
    lib.uu3d_frame_features_bytes.argtypes = [vp, i32]
    lib.uu3d_frame_features.restype = C.c_int
    lib.uu3d_frame_features.argtypes = [vp, vp, i32, vp, vp, sz, i32, vp]
    lib.uu3d_gather_window_frames.restype = C.c_int
    lib.uu3d_gather_window_frames.argtypes = [vp, vp, vp, i32, i32, i32, i32, i64, i64, vp, vp, vp, vp]
    lib.uu3d_forward_frames_ex.restype = C.c_int
    lib.uu3d_forward_frames_ex.argtypes = [vp, vp, i64, vp, vp, i32, vp, vp, C.POINTER(vp), vp, sz, i32, vp]
    scfg = C.POINTER(Uu3dStreamConfig)
    lib.uu3d_stream_state_bytes.restype = sz
    lib.uu3d_stream_state_bytes.argtypes = [vp, scfg]
    lib.uu3d_stream_state_layout.restype = C.c_int
    lib.uu3d_stream_state_layout.argtypes = [vp, scfg, C.POINTER(Uu3dStreamLayout)]
    lib.uu3d_stream_stage.restype = C.c_int
    lib.uu3d_stream_stage.argtypes = [vp, scfg, vp, vp, vp, vp, vp, vp]
    lib.uu3d_stream_commit.restype = C.c_int
    lib.uu3d_stream_commit.argtypes = [vp, scfg, vp, vp, vp, vp, vp, vp, vp]
    lib.uu3d_stream_emit.restype = C.c_int
    lib.uu3d_stream_emit.argtypes = [vp, scfg, vp, vp, vp, vp, vp, vp]
    lib.uu3d_stream_reset.restype = C.c_int
    lib.uu3d_stream_reset.argtypes = [vp, scfg, vp, vp, vp]
    # missed detections: the same calls with the validity pointers
    lib.uu3d_normalize_tracks_valid.restype = C.c_int
    lib.uu3d_normalize_tracks_valid.argtypes = [vp, i64, vp, i64, i32, vp, i32, vp, vp, vp, i32, vp, vp, vp]
    lib.uu3d_gather_windows_valid.restype = C.c_int
    lib.uu3d_gather_windows_valid.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    lib.uu3d_gather_window_frames_valid.restype = C.c_int
    lib.uu3d_gather_window_frames_valid.argtypes = [vp, vp, vp, i32, i32, i32, i32, i64, i64, vp, vp, vp, vp, vp]
    srate = C.POINTER(Uu3dStreamRate)
    lib.uu3d_stream_rate_state_layout.restype = C.c_int
    lib.uu3d_stream_rate_state_layout.argtypes = [vp, scfg, srate, C.POINTER(Uu3dStreamRateLayout)]
    lib.uu3d_stream_source_push.restype = C.c_int
    lib.uu3d_stream_source_push.argtypes = [vp, scfg, srate, vp, vp, vp, vp, C.c_int32, vp]
    lib.uu3d_stream_resample_stage.restype = C.c_int
    lib.uu3d_stream_resample_stage.argtypes = [vp, scfg, srate, vp, vp, vp, vp, vp, vp, vp]
    lib.uu3d_stream_file_keyframe.restype = C.c_int
    lib.uu3d_stream_file_keyframe.argtypes = [vp, scfg, srate, vp, vp, vp]
    lib.uu3d_stream_timed_emit.restype = C.c_int
    lib.uu3d_stream_timed_emit.argtypes = [vp, scfg, srate, vp, vp, vp, vp]
    lib.uu3d_stream_timed_emit_cubic.restype = C.c_int
    lib.uu3d_stream_timed_emit_cubic.argtypes = [vp, scfg, srate, vp, vp, vp, vp]
    lib.uu3d_stream_rate_reset.restype = C.c_int
    lib.uu3d_stream_rate_reset.argtypes = [vp, scfg, srate, vp, vp, vp]
    sout = C.POINTER(Uu3dStreamOut)
    lib.uu3d_stream_out_state_layout.restype = C.c_int
    lib.uu3d_stream_out_state_layout.argtypes = [vp, scfg, srate, sout, C.POINTER(Uu3dStreamOutLayout)]
    lib.uu3d_stream_timed_emit_multi.restype = C.c_int
    lib.uu3d_stream_timed_emit_multi.argtypes = [vp, scfg, srate, sout, vp, vp, vp, vp]
    lib.uu3d_stream_timed_emit_multi_cubic.restype = C.c_int
    lib.uu3d_stream_timed_emit_multi_cubic.argtypes = [vp, scfg, srate, sout, vp, vp, vp, vp]
    lib.uu3d_stream_out_reset.restype = C.c_int
    lib.uu3d_stream_out_reset.argtypes = [vp, scfg, srate, sout, vp, vp, vp]
    lib.uu3d_stream_repair_bytes.restype = sz
    lib.uu3d_stream_repair_bytes.argtypes = [vp, scfg, C.c_int32]
    lib.uu3d_stream_repair_layout.restype = C.c_int
    lib.uu3d_stream_repair_layout.argtypes = [vp, scfg, C.c_int32, C.POINTER(Uu3dStreamRepairLayout)]
    lib.uu3d_stream_repair_stage.restype = C.c_int
    lib.uu3d_stream_repair_stage.argtypes = [vp, scfg, C.c_int32] + [vp] * 13
    lib.uu3d_stream_commit_repair.restype = C.c_int
    lib.uu3d_stream_commit_repair.argtypes = [vp, scfg, C.c_int32] + [vp] * 11
    lib.uu3d_stream_repair_reset.restype = C.c_int
    lib.uu3d_stream_repair_reset.argtypes = [vp, scfg, C.c_int32, vp, vp, vp]
    lib.uu3d_stream_valid_bytes.restype = sz
    lib.uu3d_stream_valid_bytes.argtypes = [vp, scfg]
    lib.uu3d_stream_stage_valid.restype = C.c_int
    lib.uu3d_stream_stage_valid.argtypes = [vp, scfg, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.uu3d_stream_commit_valid.restype = C.c_int
    lib.uu3d_stream_commit_valid.argtypes = [vp, scfg, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    # any frame rate: the pose table on the model's time grid
    lib.uu3d_resample_tracks.restype = C.c_int
    lib.uu3d_resample_tracks.argtypes = [vp, i64, vp, i64, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    # per-joint missed detections: joints filled on the device in front of the two calls above
    lib.uu3d_repair_joints_scratch_bytes.restype = sz
    lib.uu3d_repair_joints_scratch_bytes.argtypes = [i64, i32]
    lib.uu3d_repair_joints.restype = C.c_int
    lib.uu3d_repair_joints.argtypes = [vp, i64, i32, vp, vp, i32, i32, vp, vp, vp, vp, sz, vp]
    # any skeleton: the detector's joints -> the model's, in front of everything above
    lib.uu3d_keypoint_map_bytes.restype = sz
    lib.uu3d_keypoint_map_bytes.argtypes = [i32, i32]
    lib.uu3d_keypoint_map_pack.restype = C.c_int
    lib.uu3d_keypoint_map_pack.argtypes = [i32, i32, vp, vp, vp, vp, sz]
    lib.uu3d_map_keypoints.restype = C.c_int
    lib.uu3d_map_keypoints.argtypes = [vp, vp, i32, vp, vp, i64, vp, vp, vp]
    # per-frame detections: people -> tracks and slots, in front of everything above
    apar = C.POINTER(Uu3dAssociateParams)
    lib.uu3d_associate_state_bytes.restype = sz
    lib.uu3d_associate_state_bytes.argtypes = [i32, i32]
    lib.uu3d_associate_reset.restype = C.c_int
    lib.uu3d_associate_reset.argtypes = [apar, vp, vp, vp]
    lib.uu3d_associate_detections.restype = C.c_int
    lib.uu3d_associate_detections.argtypes = [apar, vp, vp, vp, i32, vp, i32, i64] + [vp] * 8
    lib.uu3d_stream_associate.restype = C.c_int
    lib.uu3d_stream_associate.argtypes = [apar, vp, vp, vp, vp, i32, vp, vp, i32] + [vp] * 6
    # absolute root position: the solve per given frame, the trajectory at the returned frames
    lib.uu3d_solve_roots.restype = C.c_int
    lib.uu3d_solve_roots.argtypes = [vp, vp, vp, i64, i32, vp, i32, vp, i32, vp, vp, vp]
    lib.uu3d_root_trajectory_scratch_bytes.restype = sz
    lib.uu3d_root_trajectory_scratch_bytes.argtypes = [i64]
    lib.uu3d_root_trajectory.restype = C.c_int
    lib.uu3d_root_trajectory.argtypes = [vp, vp, i64, vp, i32, vp, vp, vp, i64, vp, vp, vp, sz, vp]
    # live absolute root: the ring of raw frames and the held root of a session with a camera
    lib.uu3d_stream_root_bytes.restype = sz
    lib.uu3d_stream_root_bytes.argtypes = [i32, i32, i32]
    lib.uu3d_stream_root.restype = C.c_int
    lib.uu3d_stream_root.argtypes = [i32, i32, i32] + [vp] * 7 + [i32, vp, i32, vp, vp, vp]
    lib.uu3d_stream_root_reset.restype = C.c_int
    lib.uu3d_stream_root_reset.argtypes = [i32, i32, i32, vp, vp, vp]
    # live several views: the V slots of a person joined to one pose and one world root per push
    lib.uu3d_stream_views_bytes.restype = sz
    lib.uu3d_stream_views_bytes.argtypes = [i32, i32]
    lib.uu3d_stream_views.restype = C.c_int
    lib.uu3d_stream_views.argtypes = [i32, i32, i32, i32] + [vp] * 7 + [i32] + [vp] * 8
    lib.uu3d_stream_views_reset.restype = C.c_int
    lib.uu3d_stream_views_reset.argtypes = [i32, i32, vp, vp, vp]
    # steady output: the One-Euro filter over finished tracks and the live filter of a session
    f64 = C.c_double
    lib.uu3d_one_euro_tracks.restype = C.c_int
    lib.uu3d_one_euro_tracks.argtypes = [vp, vp, i64, i32, vp, vp, vp, i32, vp, f64, f64, f64, vp]
    lib.uu3d_one_euro_tracks_two_pass.restype = C.c_int
    lib.uu3d_one_euro_tracks_two_pass.argtypes = lib.uu3d_one_euro_tracks.argtypes
    lib.uu3d_stream_one_euro_bytes.restype = sz
    lib.uu3d_stream_one_euro_bytes.argtypes = [i32, i32]
    lib.uu3d_stream_one_euro.restype = C.c_int
    lib.uu3d_stream_one_euro.argtypes = [i32, i32, i32] + [vp] * 6 + [f64] * 4 + [vp, vp]
    lib.uu3d_stream_one_euro_reset.restype = C.c_int
    lib.uu3d_stream_one_euro_reset.argtypes = [i32, i32, vp, vp, vp]
    # live tracks, end of a track: the drain state, the commit of a drain tick, the root solve without filing, the result rows, the reset
    lib.uu3d_stream_drain_bytes.restype = sz
    lib.uu3d_stream_drain_bytes.argtypes = [i32]
    lib.uu3d_stream_drain_layout.restype = C.c_int
    lib.uu3d_stream_drain_layout.argtypes = [i32, C.POINTER(Uu3dStreamDrainLayout)]
    lib.uu3d_stream_drain_commit.restype = C.c_int
    lib.uu3d_stream_drain_commit.argtypes = [vp, scfg] + [vp] * 8
    lib.uu3d_stream_root_drain.restype = C.c_int
    lib.uu3d_stream_root_drain.argtypes = [i32, i32, i32] + [vp] * 6 + [i32, vp, vp, vp]
    lib.uu3d_stream_drain_file.restype = C.c_int
    lib.uu3d_stream_drain_file.argtypes = [i32, i32, vp, i32, C.POINTER(vp), C.POINTER(i32), C.POINTER(vp)] + [vp] * 5
    lib.uu3d_stream_drain_reset.restype = C.c_int
    lib.uu3d_stream_drain_reset.argtypes = [i32, vp, vp, vp]
    # constant bone lengths: the lengths of finished tracks, their fix, and the live form of a session
    lib.uu3d_bone_lengths.restype = C.c_int
    lib.uu3d_bone_lengths.argtypes = [vp, i64, i32, vp, vp, vp, i32, vp, vp, vp]
    lib.uu3d_fix_bones.restype = C.c_int
    lib.uu3d_fix_bones.argtypes = [vp, vp, i64, i32, vp, vp, i32, vp, i32, vp, vp]
    lib.uu3d_stream_bones_bytes.restype = sz
    lib.uu3d_stream_bones_bytes.argtypes = [i32, i32]
    lib.uu3d_stream_bones.restype = C.c_int
    lib.uu3d_stream_bones.argtypes = [i32, i32, vp, vp, vp, i32] + [vp] * 7
    lib.uu3d_stream_bones_reset.restype = C.c_int
    lib.uu3d_stream_bones_reset.argtypes = [i32, i32, vp, vp, vp]
    lib.uu3d_undistort_points.restype = C.c_int
    lib.uu3d_undistort_points.argtypes = [vp, vp, i64, i32, vp, i32, vp, vp]
    lib.uu3d_camera_to_world.restype = C.c_int
    lib.uu3d_camera_to_world.argtypes = [vp, vp, vp, vp, vp, i64, i32, vp, i32, vp, vp]
    lib.uu3d_fuse_views.restype = C.c_int
    lib.uu3d_fuse_views.argtypes = [vp, vp, vp, i32, i64, i32, i32, vp, vp, vp, vp]
    lib.uu3d_solve_view_roots.restype = C.c_int
    lib.uu3d_solve_view_roots.argtypes = [vp, vp, vp, i32, i64, i32, vp, i32, vp, vp, vp]
    # who is who: view_of is HOST memory (its order is a guard), everything else device memory
    lib.uu3d_view_pair_sums.restype = C.c_int
    lib.uu3d_view_pair_sums.argtypes = [vp, vp, C.POINTER(i32), i32, i64, i32, i32, vp, vp, vp, vp]
    lib.uu3d_group_views.restype = C.c_int
    lib.uu3d_group_views.argtypes = [vp, vp, C.POINTER(i32), i32, i32, C.c_double, i32, vp, vp, vp, vp]
    lib.uu3d_gather_view_tracks.restype = C.c_int
    lib.uu3d_gather_view_tracks.argtypes = [vp, vp, vp, vp, i32, i32, i64, i32, i32, vp, vp, vp, vp]
    lib.uu3d_view_lag_scratch_bytes.restype = sz
    lib.uu3d_view_lag_scratch_bytes.argtypes = [i64, i32]
    lib.uu3d_view_lag_sums.restype = C.c_int
    lib.uu3d_view_lag_sums.argtypes = [vp, vp, C.POINTER(i32), C.POINTER(i64), i32, i32, i32, vp, i32, vp, vp, vp, vp]
    lib.uu3d_view_offsets.restype = C.c_int
    lib.uu3d_view_offsets.argtypes = [vp, vp, C.POINTER(i32), i32, i32, i32, i32, i32, vp, vp, vp, vp]
    lib.uu3d_triangulate_joints.restype = C.c_int
    lib.uu3d_triangulate_joints.argtypes = [vp, vp, vp, i32, i64, i32, vp, i32, C.c_double, vp, vp, vp]
    lib.uu3d_place_joints.restype = C.c_int
    lib.uu3d_place_joints.argtypes = [vp, vp, vp, i64, i32, i32, vp, vp, vp]
    lib.uu3d_view_calibrate_chunks.restype = i64
    lib.uu3d_view_calibrate_chunks.argtypes = [i64]
    lib.uu3d_view_moment_sums.restype = C.c_int
    lib.uu3d_view_moment_sums.argtypes = [vp, vp, vp, i32, i64, i32, i32, vp, vp]
    lib.uu3d_view_position_sums.restype = C.c_int
    lib.uu3d_view_position_sums.argtypes = [vp, vp, vp, i32, i64, i32, vp, i32, vp, vp, vp]
    lib.uu3d_solve_view_pose.restype = C.c_int
    lib.uu3d_solve_view_pose.argtypes = [vp, i32, i64, i32, i32, vp, vp, vp, vp]
    # who is who without a world: view_of is HOST memory, as in who is who
    lib.uu3d_lift_pair_sums.restype = C.c_int
    lib.uu3d_lift_pair_sums.argtypes = [vp, vp, vp, C.POINTER(i32), i32, i64, i32, i32, i32, vp, vp, vp]
    lib.uu3d_joint_rotations.restype = C.c_int
    lib.uu3d_joint_rotations.argtypes = [vp, i64, i32, vp, i32] + [vp] * 6
    lib.uu3d_joint_rotations_reset.restype = C.c_int
    lib.uu3d_joint_rotations_reset.argtypes = [i32, i32] + [vp] * 5
    lib.uu3d_world_to_cam_2d.restype = C.c_int
    lib.uu3d_world_to_cam_2d.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp]
    lib.uu3d_set_schedule.restype = C.c_int
    lib.uu3d_set_schedule.argtypes = [vp, i32]
    lib.uu3d_set_profiling.restype = C.c_int
    lib.uu3d_set_profiling.argtypes = [vp, i32]
    lib.uu3d_profile_read.restype = C.c_int
    lib.uu3d_profile_read.argtypes = [vp, C.POINTER(Uu3dProfileEntry), i32, C.POINTER(i32)]
    lib.uu3d_mpjpe_loss.restype = C.c_int
    lib.uu3d_mpjpe_loss.argtypes = [vp, vp, vp, i32, i32, i32, i32, C.c_float, C.c_float, i32, vp, vp, vp, vp, vp]
    lib.uu3d_adamw_update.restype = C.c_int
    lib.uu3d_adamw_update.argtypes = [vp, vp, vp, vp, vp, i64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, i64, vp]
    lib.uu3d_adamw_update_guarded.restype = C.c_int
    lib.uu3d_adamw_update_guarded.argtypes = [vp, vp, vp, vp, vp, i64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, i64, vp, vp]
    lib.uu3d_train_nonfinite_flag.restype = vp
    lib.uu3d_train_nonfinite_flag.argtypes = [vp]
    lib.uu3d_train_nonfinite.restype = C.c_int
    lib.uu3d_train_nonfinite.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.uu3d_ema_update.restype = C.c_int
    lib.uu3d_ema_update.argtypes = [vp, vp, i64, C.c_float, vp]
    lib.uu3d_num_params.restype = i64
    lib.uu3d_num_params.argtypes = [vp]
    lib.uu3d_train_init.restype = C.c_int
    lib.uu3d_train_init.argtypes = [vp, vp, vp]
    lib.uu3d_train_repack.restype = C.c_int
    lib.uu3d_train_repack.argtypes = [vp, vp, vp]
    lib.uu3d_train_export.restype = C.c_int
    lib.uu3d_train_export.argtypes = [vp, vp, vp]
    lib.uu3d_train_workspace_bytes.restype = sz
    lib.uu3d_train_workspace_bytes.argtypes = [vp, i32]
    lib.uu3d_train_forward_backward.restype = C.c_int
    lib.uu3d_train_forward_backward.argtypes = [vp, vp, vp, vp, vp, i32, i32, C.c_float, C.c_float, i32,
                                                C.POINTER(C.c_float), vp, vp, vp, vp, vp, vp, sz, vp]
    lib.uu3d_train_forward_backward_masked.restype = C.c_int
    lib.uu3d_train_forward_backward_masked.argtypes = [vp, vp, vp, vp, vp, i32, i32, C.c_float, C.c_float, i32,
                                                       C.POINTER(C.c_float), vp, vp, C.c_float, vp, vp, vp, vp, vp, sz, vp]
    lib.uu3d_train_set_grad_callback.restype = C.c_int
    lib.uu3d_train_set_grad_callback.argtypes = [vp, GRAD_READY_FN, vp]
    lib.uu3d_train_set_dropout.restype = C.c_int
    lib.uu3d_train_set_dropout.argtypes = [vp, C.c_float, C.c_float, C.c_uint64]
    lib.uu3d_train_forward_tape.restype = C.c_int
    lib.uu3d_train_forward_tape.argtypes = [vp, vp, vp, vp, i32, C.POINTER(C.c_float), vp, vp, C.c_float, vp, vp, vp, sz, C.POINTER(vp), vp]
    lib.uu3d_train_backward_tape.restype = C.c_int
    lib.uu3d_train_backward_tape.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    lib.uu3d_tape_destroy.restype = None
    lib.uu3d_tape_destroy.argtypes = [vp]
    lib.uu3d_train_clear_nonfinite.restype = C.c_int
    lib.uu3d_train_clear_nonfinite.argtypes = [vp, vp]
    lib.uu3d_train_backward_tape_accumulate.restype = C.c_int
    lib.uu3d_train_backward_tape_accumulate.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, vp]
    lib.uu3d_train_copy_nonfinite.restype = C.c_int
    lib.uu3d_train_copy_nonfinite.argtypes = [vp, vp, vp]
    lib.uu3d_op_scratch_floats.restype = sz
    lib.uu3d_op_scratch_floats.argtypes = []
    lib.uu3d_op_gemm_tn.restype = C.c_int
    lib.uu3d_op_gemm_tn.argtypes = [vp, i32, vp, i32, i32, i32, i32, vp, i32, vp, sz, vp]
    lib.uu3d_op_gemm_tn_h3.restype = C.c_int
    lib.uu3d_op_gemm_tn_h3.argtypes = [vp, i32, vp, i32, i32, i32, i32, vp, i32, vp, sz, vp]
    lib.uu3d_op_gemm_nt.restype = C.c_int
    lib.uu3d_op_gemm_nt.argtypes = [vp, i32, vp, i32, i32, i32, i32, vp, i32, vp, sz, vp]
    lib.uu3d_op_colsum.restype = C.c_int
    lib.uu3d_op_colsum.argtypes = [vp, i32, i32, i32, i32, vp, i32, vp, i32, vp, sz, vp]
    lib.uu3d_op_row_stats.restype = C.c_int
    lib.uu3d_op_row_stats.argtypes = [vp, i32, i32, i32, C.c_float, vp, vp]
    lib.uu3d_op_ln_bwd.restype = C.c_int
    lib.uu3d_op_ln_bwd.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, i32, vp, vp, vp, sz, vp]
    lib.uu3d_op_attn_fwd.restype = C.c_int
    lib.uu3d_op_attn_fwd.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp, vp, i32, vp]
    lib.uu3d_op_attn_bwd.restype = C.c_int
    lib.uu3d_op_attn_bwd.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, i32, vp]
    lib.uu3d_op_attn_long_fwd.restype = C.c_int
    lib.uu3d_op_attn_long_fwd.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, i32, vp, vp]
    lib.uu3d_op_attn_long_bwd.restype = C.c_int
    lib.uu3d_op_attn_long_bwd.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, i32, vp]
    lib.uu3d_op_attn_long_infer.restype = C.c_int
    lib.uu3d_op_attn_long_infer.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, i32, vp]
    lib.uu3d_op_panel_operand_bytes.restype = sz
    lib.uu3d_op_panel_operand_bytes.argtypes = [i32]
    lib.uu3d_op_panel_a_bytes.restype = sz
    lib.uu3d_op_panel_a_bytes.argtypes = [i32]
    lib.uu3d_op_panel_pack.restype = C.c_int
    lib.uu3d_op_panel_pack.argtypes = [vp, i32, vp, vp]
    lib.uu3d_op_ln_dense_panel.restype = C.c_int
    lib.uu3d_op_ln_dense_panel.argtypes = [vp, i32, i32, vp, vp, C.c_float, vp, vp, i32, i32, vp, vp, i32, vp]
    lib.uu3d_op_ln_dense_panel_ex.restype = C.c_int
    lib.uu3d_op_ln_dense_panel_ex.argtypes = [vp, i32, i32, vp, vp, C.c_float, vp, vp, i32, i32, i32, i32, C.c_float, vp, vp, i32, vp, vp, vp, vp, vp]
    lib.uu3d_op_panel_a_unpack.restype = C.c_int
    lib.uu3d_op_panel_a_unpack.argtypes = [vp, i32, vp, vp]
    lib.uu3d_op_mlp_operand_bytes.restype = sz
    lib.uu3d_op_mlp_operand_bytes.argtypes = []
    lib.uu3d_op_mlp_pack.restype = C.c_int
    lib.uu3d_op_mlp_pack.argtypes = [vp, vp, vp, vp]
    lib.uu3d_op_mlp_fused.restype = C.c_int
    lib.uu3d_op_mlp_fused.argtypes = [vp, i32, i32, vp, vp, C.c_float, vp, vp, vp, vp, vp]
    lib.uu3d_op_wt_operand_bytes.restype = sz
    lib.uu3d_op_wt_operand_bytes.argtypes = [i32, i32]
    lib.uu3d_op_wt_pack.restype = C.c_int
    lib.uu3d_op_wt_pack.argtypes = [vp, i32, i32, vp, vp]
    lib.uu3d_op_ln_dense_wt.restype = C.c_int
    lib.uu3d_op_ln_dense_wt.argtypes = [vp, i32, i32, i32, vp, vp, C.c_float, vp, vp, i32, i32, C.c_float, vp, i32, vp]
    lib.uu3d_op_attn_infer.restype = C.c_int
    lib.uu3d_op_attn_infer.argtypes = [vp, i32, i32, i32, i32, i32, vp, i32, vp, i32, vp]
    lib.uu3d_op_attn_qf_bytes.restype = sz
    lib.uu3d_op_attn_qf_bytes.argtypes = [i32]
    lib.uu3d_op_attn_qf_pack.restype = C.c_int
    lib.uu3d_op_attn_qf_pack.argtypes = [vp, vp, i32, vp]
    lib.uu3d_op_tiled_operand_bytes.restype = sz
    lib.uu3d_op_tiled_operand_bytes.argtypes = [i32, i32]
    lib.uu3d_op_tiled_pack.restype = C.c_int
    lib.uu3d_op_tiled_pack.argtypes = [vp, i32, i32, vp, vp]
    lib.uu3d_op_tiled_dense.restype = C.c_int
    lib.uu3d_op_tiled_dense.argtypes = [C.POINTER(Uu3dTiledDenseArgs), vp]
    lib.uu3d_op_tiled_split.restype = C.c_int
    lib.uu3d_op_tiled_split.argtypes = [i32, i32, i32, i32, sz, C.POINTER(i32), C.POINTER(i32)]
    lib.uu3d_op_spatial_stack.restype = C.c_int
    lib.uu3d_op_spatial_stack.argtypes = [vp, vp, i32, vp, vp, i32, i32, vp, vp]
    lib.uu3d_op_compact_frames.restype = C.c_int
    lib.uu3d_op_compact_frames.argtypes = [vp, i32, vp, vp]
    lib.uu3d_op_spatial_choice.restype = C.c_int
    lib.uu3d_op_spatial_choice.argtypes = [vp, i32, i32, C.POINTER(i32), C.POINTER(i32)]
    lib.uu3d_op_panel_a_pack.restype = C.c_int
    lib.uu3d_op_panel_a_pack.argtypes = [vp, vp, i32, vp]
    lib.uu3d_op_attn_qf_unpack.restype = C.c_int
    lib.uu3d_op_attn_qf_unpack.argtypes = [vp, i32, vp, vp]
    lib.uu3d_op_tchain.restype = C.c_int
    lib.uu3d_op_tchain.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.uu3d_op_tchain_scratch_bytes.restype = sz
    lib.uu3d_op_tchain_scratch_bytes.argtypes = [i32]
    lib.uu3d_op_tchain_launches.restype = C.c_int
    lib.uu3d_op_tchain_launches.argtypes = [vp, C.POINTER(i32), i32]
    lib.uu3d_op_tchain_xs_pack.restype = C.c_int
    lib.uu3d_op_tchain_xs_pack.argtypes = [vp, i32, i32, i32, vp]
    lib.uu3d_op_tchain_xs_unpack.restype = C.c_int
    lib.uu3d_op_tchain_xs_unpack.argtypes = [vp, i32, i32, i32, vp]
    lib.uu3d_op_train_operand_bytes.restype = sz
    lib.uu3d_op_train_operand_bytes.argtypes = [i32, i32, i32, i32]
    lib.uu3d_op_train_pack.restype = C.c_int
    lib.uu3d_op_train_pack.argtypes = [vp, i32, i32, i32, i32, vp, vp]
    lib.uu3d_op_train_dense.restype = C.c_int
    lib.uu3d_op_train_dense.argtypes = [C.POINTER(Uu3dTrainDenseArgs), vp]
    lib.uu3d_op_train_wgrad.restype = C.c_int
    lib.uu3d_op_train_wgrad.argtypes = [C.POINTER(Uu3dTrainWgradArgs), vp]
    lib.uu3d_op_colsum3.restype = C.c_int
    lib.uu3d_op_colsum3.argtypes = [vp, i32, i32, i32, vp, vp, vp, i32, vp, sz, vp]
    lib.uu3d_op_ln_bwd_ex.restype = C.c_int
    lib.uu3d_op_ln_bwd_ex.argtypes = [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, C.c_float, i32, vp, vp, vp, vp, sz, vp]
    lib.uu3d_op_identity_bwd.restype = C.c_int
    lib.uu3d_op_identity_bwd.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp, vp]
    lib.uu3d_op_scale_rows.restype = C.c_int
    lib.uu3d_op_scale_rows.argtypes = [vp, i32, i32, vp, C.c_float, i32, vp, i32, vp, vp]
    if path is None:
        _lib = lib
    return lib


def check(lib, status, handle=None):
    if status != UU3D_OK:
        detail = lib.uu3d_last_error(handle).decode() if True else ""
        base = lib.uu3d_status_string(status).decode()
        raise Uu3dError(status, f"{base}: {detail}" if detail else base)


def ptr(t):
    """The device (or pinned host) address of a tensor as a ctypes argument; None stays None (a null pointer)."""
    return None if t is None else C.c_void_p(t.data_ptr())
