// uu3d_undistort_api.inc -- the host side of LENS DISTORTION (uu3d_undistort.h; include/uu3d.h), a piece of uu3d_api.hip: the one launch.
// No model and no state.  Every guard comes before any HIP call.

int uu3d_undistort_points(const float* in, float* out, int64_t rows, int32_t points_per_row, const int32_t* row_track, int32_t num_tracks,
                          const double* cameras, void* stream) {
    if (rows < 0 || points_per_row < 1 || num_tracks < 1 || rows > (INT64_MAX >> 4) / points_per_row ||
        (rows * points_per_row + 255) / 256 > INT32_MAX)
        return UU3D_ERR_INVALID_ARGUMENT;
    if (rows == 0) return UU3D_OK;
    if (!in || !out || !cameras || (const void*)in == (const void*)out) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)in & 7) != 0 || ((uintptr_t)out & 7) != 0 || ((uintptr_t)cameras & 7) != 0 || ((uintptr_t)row_track & 3) != 0)
        return UU3D_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(undistort_points_kernel, dim3((unsigned)((rows * points_per_row + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       in, out, (long)rows, points_per_row, row_track, num_tracks, cameras);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}
