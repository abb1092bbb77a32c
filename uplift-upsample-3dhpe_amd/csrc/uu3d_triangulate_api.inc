// uu3d_triangulate_api.inc -- the host side of WHERE RAYS MEET (uu3d_triangulate.h; include/uu3d.h), a piece of uu3d_api.hip: the two
// launches.  No model and no state.  Every guard comes before any HIP call.

// rows * J lanes in blocks of 256; J beyond kRootMaxJoints is unsupported, everything else out of range is invalid.
static int triangulate_shape(int64_t rows, int32_t J) {
    if (J > kRootMaxJoints) return UU3D_ERR_UNSUPPORTED;
    if (J < 1 || rows < 0 || rows > (INT64_MAX >> 8) / J || (rows * J + 255) / 256 > INT32_MAX) return UU3D_ERR_INVALID_ARGUMENT;
    return UU3D_OK;
}

int uu3d_triangulate_joints(const float* kp2d, const uint8_t* joint_flags, const uint8_t* sees, int32_t views, int64_t rows, int32_t J,
                            const double* cameras, int32_t min_views, double max_residual, double* points, uint8_t* count, void* stream) {
    if (views > kViewsMax) return UU3D_ERR_UNSUPPORTED;
    const int shape = triangulate_shape(rows, J);
    if (shape != UU3D_OK) return shape;
    if (views < 1 || min_views < kTriangulateMinViews || min_views > kViewsMax) return UU3D_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(max_residual) || !(max_residual > 0.0)) return UU3D_ERR_INVALID_ARGUMENT;
    if (rows == 0) return UU3D_OK;
    if (!kp2d || !sees || !cameras || !points || !count) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)kp2d & 7) != 0 || ((uintptr_t)cameras & 7) != 0 || ((uintptr_t)points & 7) != 0) return UU3D_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(triangulate_joints_kernel, dim3((unsigned)((rows * J + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       kp2d, joint_flags, sees, views, (long)rows, J, cameras, min_views, max_residual, points, count);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_place_joints(const float* fused, const double* points, const uint8_t* count, int64_t rows, int32_t J, int32_t root, float* placed,
                      uint8_t* joint_views, void* stream) {
    const int shape = triangulate_shape(rows, J);
    if (shape != UU3D_OK) return shape;
    if (root < 0 || root >= J) return UU3D_ERR_INVALID_ARGUMENT;
    if (rows == 0) return UU3D_OK;
    if (!fused || !points || !count || !placed || !joint_views || (const void*)fused == (const void*)placed) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)fused & 3) != 0 || ((uintptr_t)points & 7) != 0 || ((uintptr_t)placed & 3) != 0) return UU3D_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(place_joints_kernel, dim3((unsigned)((rows * J + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       fused, points, count, (long)rows, J, root, placed, joint_views);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}
