// uu3d_rotations_api.inc -- the host side of JOINT ROTATIONS (uu3d_rotations.h; include/uu3d.h), a piece of uu3d_api.hip: the rotations
// of any (frames, J, 3) buffer in one launch, and the reset of a live session's slots.  No model and no state: the calls take the joint
// count, like uu3d_fix_bones.  Every guard comes before any HIP call.

int uu3d_joint_rotations(const float* poses, int64_t frames, int32_t J, const int32_t* tree, int32_t depth, const double* rest,
                         const uint8_t* row_mask, float* local, float* global, uint8_t* flags, void* stream) {
    if (J > kBonesMaxJoints) return UU3D_ERR_UNSUPPORTED;
    if (frames < 0 || J < 1 || depth < 0 || depth >= kBonesMaxJoints || frames > ((int64_t)1 << 32)) return UU3D_ERR_INVALID_ARGUMENT;
    if (frames == 0) return UU3D_OK;
    if (!poses || !tree || !rest || !local || (const void*)poses == (const void*)local || (const void*)poses == (const void*)global)
        return UU3D_ERR_INVALID_ARGUMENT;
    if (!bones_aligned(poses, 3) || !bones_aligned(tree, 3) || !bones_aligned(rest, 7) || !bones_aligned(local, 15) || !bones_aligned(global, 15))
        return UU3D_ERR_INVALID_ARGUMENT;
    const int64_t groups = (frames + kRotationWaves - 1) / kRotationWaves;      // (<= 2^30 workgroups)
    hipLaunchKernelGGL(joint_rotations_kernel, dim3((unsigned)groups), dim3(kRotationWaves * kBonesLanes), 0, (hipStream_t)stream, poses,
                       (long)frames, J, tree, depth, rest, row_mask, local, global, flags);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_joint_rotations_reset(int32_t slots, int32_t J, float* local, float* global, uint8_t* flags, const uint8_t* slot_mask, void* stream) {
    if (J > kBonesMaxJoints) return UU3D_ERR_UNSUPPORTED;
    if (slots < 1 || slots > (1 << 20) || J < 1) return UU3D_ERR_INVALID_ARGUMENT;
    if (!local || !bones_aligned(local, 15) || !bones_aligned(global, 15)) return UU3D_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(joint_rotations_reset_kernel, dim3((unsigned)slots), dim3(kBonesLanes), 0, (hipStream_t)stream, slot_mask, J, local, global,
                       flags);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}
