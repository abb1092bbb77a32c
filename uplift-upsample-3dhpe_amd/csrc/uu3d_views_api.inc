// uu3d_views_api.inc -- the host side of SEVERAL VIEWS (uu3d_views.h; include/uu3d.h), a piece of uu3d_api.hip: the two launches.
// No model and no state: the calls take the view and joint counts.  Every guard comes before any HIP call.

static int views_shape(int32_t views, int64_t rows, int32_t J, int32_t min_joints, int64_t lanes_per_row) {
    if (views > kViewsMax || J > kRootMaxJoints) return UU3D_ERR_UNSUPPORTED;
    if (views < 1 || J < 1 || rows < 0 || min_joints < 2 || rows > (INT64_MAX >> 8) / J || (rows * lanes_per_row + 255) / 256 > INT32_MAX)
        return UU3D_ERR_INVALID_ARGUMENT;
    return UU3D_OK;
}

int uu3d_fuse_views(const float* poses, const float* kp2d, const uint8_t* joint_flags, int32_t views, int64_t rows, int32_t J, int32_t min_joints,
                    float* fused, uint8_t* view_count, uint8_t* sees, void* stream) {
    const int shape = views_shape(views, rows, J, min_joints, J);
    if (shape != UU3D_OK) return shape;
    if (rows == 0) return UU3D_OK;
    if (!poses || !kp2d || !fused || !view_count || !sees || (const void*)poses == (const void*)fused) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)poses & 3) != 0 || ((uintptr_t)kp2d & 7) != 0 || ((uintptr_t)fused & 3) != 0) return UU3D_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(fuse_views_kernel, dim3((unsigned)((rows * J + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       poses, kp2d, joint_flags, views, (long)rows, J, min_joints, fused, view_count, sees);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_solve_view_roots(const float* fused, const float* kp2d, const uint8_t* joint_flags, int32_t views, int64_t rows, int32_t J,
                          const double* cameras, int32_t min_joints, double* roots, uint8_t* solved, void* stream) {
    const int shape = views_shape(views, rows, J, min_joints, 1);
    if (shape != UU3D_OK) return shape;
    if (rows == 0) return UU3D_OK;
    if (!fused || !kp2d || !cameras || !roots || !solved) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)fused & 3) != 0 || ((uintptr_t)kp2d & 7) != 0 || ((uintptr_t)cameras & 7) != 0 || ((uintptr_t)roots & 7) != 0)
        return UU3D_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(solve_view_roots_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       fused, kp2d, joint_flags, views, (long)rows, J, cameras, min_joints, roots, solved);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}
