// uu3d_view_calibrate_api.inc -- the host side of WHERE THE CAMERAS STAND (uu3d_view_calibrate.h; include/uu3d.h), a piece of
// uu3d_api.hip: the launches.  No model and no state.  Every guard comes before any HIP call.

// One workgroup per (chunk of kCalibrateChunk rows, view); the int32 terms of a view keep rows below 2^31.
static int calibrate_shape(int32_t views, int64_t rows, int32_t J, int32_t min_joints) {
    if (views > kViewsMax || J > kRootMaxJoints) return UU3D_ERR_UNSUPPORTED;
    if (views < 1 || J < 1 || rows < 1 || rows > INT32_MAX || min_joints < 2) return UU3D_ERR_INVALID_ARGUMENT;
    return UU3D_OK;
}

int64_t uu3d_view_calibrate_chunks(int64_t rows) {
    return rows < 1 || rows > INT32_MAX ? 0 : (rows + kCalibrateChunk - 1) / kCalibrateChunk;
}

int uu3d_view_moment_sums(const float* poses, const float* kp2d, const uint8_t* joint_flags, int32_t views, int64_t rows, int32_t J,
                          int32_t min_joints, double* partial, void* stream) {
    const int shape = calibrate_shape(views, rows, J, min_joints);
    if (shape != UU3D_OK) return shape;
    if (!poses || !kp2d || !partial) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)poses & 3) != 0 || ((uintptr_t)kp2d & 7) != 0 || ((uintptr_t)partial & 7) != 0) return UU3D_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(view_moment_sums_kernel, dim3((unsigned)uu3d_view_calibrate_chunks(rows), (unsigned)views), dim3(kCalibrateLanes), 0,
                       (hipStream_t)stream, poses, kp2d, joint_flags, (long)rows, J, min_joints, partial);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_view_position_sums(const float* poses, const float* kp2d, const uint8_t* joint_flags, int32_t views, int64_t rows, int32_t J,
                            const double* intrinsics, int32_t min_joints, const double* pose, double* partial, void* stream) {
    const int shape = calibrate_shape(views, rows, J, min_joints);
    if (shape != UU3D_OK) return shape;
    if (!poses || !kp2d || !intrinsics || !pose || !partial) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)poses & 3) != 0 || ((uintptr_t)kp2d & 7) != 0 || ((uintptr_t)intrinsics & 7) != 0 || ((uintptr_t)pose & 7) != 0 ||
        ((uintptr_t)partial & 7) != 0)
        return UU3D_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(view_position_sums_kernel, dim3((unsigned)uu3d_view_calibrate_chunks(rows), (unsigned)views), dim3(kCalibrateLanes), 0,
                       (hipStream_t)stream, poses, kp2d, joint_flags, (long)rows, J, intrinsics, min_joints, pose, partial);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_solve_view_pose(const double* partial, int32_t views, int64_t chunks, int32_t stage, int32_t min_terms, const double* pose_in,
                         double* pose_out, int32_t* terms, void* stream) {
    if (views > kViewsMax) return UU3D_ERR_UNSUPPORTED;
    if (views < 1 || chunks < 1 || chunks > INT32_MAX / kCalibrateChunk + 1 || (stage != 0 && stage != 1) || min_terms < 1)
        return UU3D_ERR_INVALID_ARGUMENT;
    if (!partial || !pose_out || !terms || (stage == 1 && (!pose_in || pose_in == pose_out))) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)partial & 7) != 0 || ((uintptr_t)pose_in & 7) != 0 || ((uintptr_t)pose_out & 7) != 0 || ((uintptr_t)terms & 3) != 0)
        return UU3D_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(solve_view_pose_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, partial, views, (long)chunks, stage, min_terms, pose_in,
                       pose_out, terms);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}
