// uu3d_world_api.inc -- the host side of WORLD SPACE (uu3d_world.h; include/uu3d.h), a piece of uu3d_api.hip: the one launch.
// No model and no state: the call takes the joint count, like uu3d_joint_rotations.  Every guard comes before any HIP call.

int uu3d_camera_to_world(const float* poses, float* poses_out, const float* roots, const uint8_t* root_state, float* roots_out, int64_t rows,
                         int32_t J, const int32_t* row_track, int32_t num_tracks, const double* extrinsics, void* stream) {
    if (rows < 0 || J < 1 || num_tracks < 1 || rows > (INT64_MAX >> 4) / ((int64_t)J + 1) ||
        (rows * ((int64_t)J + 1) + 255) / 256 > INT32_MAX)
        return UU3D_ERR_INVALID_ARGUMENT;
    if (rows == 0) return UU3D_OK;
    const bool with_poses = poses || poses_out, with_roots = roots || root_state || roots_out;
    if (!extrinsics || (!with_poses && !with_roots)) return UU3D_ERR_INVALID_ARGUMENT;
    if (with_poses && (!poses || !poses_out)) return UU3D_ERR_INVALID_ARGUMENT;      // the pair and the trio: null together or not at all
    if (with_roots && (!roots || !root_state || !roots_out)) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)poses & 3) != 0 || ((uintptr_t)poses_out & 3) != 0 || ((uintptr_t)roots & 3) != 0 || ((uintptr_t)roots_out & 3) != 0 ||
        ((uintptr_t)extrinsics & 7) != 0 || ((uintptr_t)row_track & 3) != 0)
        return UU3D_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(camera_to_world_kernel, dim3((unsigned)((rows * ((int64_t)J + 1) + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       poses, poses_out, roots, root_state, roots_out, (long)rows, J, row_track, num_tracks, extrinsics);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}
