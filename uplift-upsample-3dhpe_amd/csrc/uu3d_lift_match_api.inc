// uu3d_lift_match_api.inc -- the host side of WHO IS WHO WITHOUT A WORLD (uu3d_lift_match.h; include/uu3d.h), a piece of uu3d_api.hip: the
// launch.  No model and no state.  Every guard comes before any HIP call; view_of is HOST memory, so its order is a guard too.

int uu3d_lift_pair_sums(const float* poses, const float* kp2d, const uint8_t* joint_flags, const int32_t* view_of, int32_t tracks, int64_t frames,
                        int32_t J, int32_t views, int32_t min_joints, double* sums, int32_t* terms, void* stream) {
    if (J > kRootMaxJoints) return UU3D_ERR_UNSUPPORTED;
    ViewStarts st;
    const int shape = view_starts(view_of, tracks, views, &st);
    if (shape != UU3D_OK) return shape;
    if (J < 1 || frames < 1 || frames > INT32_MAX / J || min_joints < 2) return UU3D_ERR_INVALID_ARGUMENT;      // (the bound of uu3d_view_pair_sums)
    if (!poses || !kp2d || !sums || !terms) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)poses & 3) != 0 || ((uintptr_t)kp2d & 7) != 0 || ((uintptr_t)sums & 7) != 0 || ((uintptr_t)terms & 3) != 0)
        return UU3D_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(lift_pair_sums_kernel, dim3((unsigned)(tracks * (tracks + 1) / 2)), dim3(kMatchLanes), 0, (hipStream_t)stream,
                       poses, kp2d, joint_flags, st, tracks, (int)frames, J, views, min_joints, sums, terms);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}
