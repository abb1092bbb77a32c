// uu3d_view_match_api.inc -- the host side of WHO IS WHO (uu3d_view_match.h; include/uu3d.h), a piece of uu3d_api.hip: the three launches.
// No model and no state.  Every guard comes before any HIP call; view_of is HOST memory, so its order is a guard too.

// view_of (tracks) on the host, ascending, every entry in 0 .. views - 1 -> the first track of every view.
static int view_starts(const int32_t* view_of, int32_t tracks, int32_t views, ViewStarts* st) {
    if (views > kViewsMax || tracks > kMatchMaxTracks) return UU3D_ERR_UNSUPPORTED;
    if (views < 1 || tracks < 1 || !view_of) return UU3D_ERR_INVALID_ARGUMENT;
    int32_t last = 0;
    for (int v = 0; v <= kViewsMax; ++v) st->start[v] = tracks;
    st->start[0] = 0;
    for (int32_t m = 0; m < tracks; ++m) {
        const int32_t v = view_of[m];
        if (v < last || v >= views) return UU3D_ERR_INVALID_ARGUMENT;   // not ascending, or no such view
        for (int32_t u = last + 1; u <= v; ++u) st->start[u] = m;
        last = v;
    }
    return UU3D_OK;
}

int uu3d_view_pair_sums(const float* kp, const uint8_t* joint_flags, const int32_t* view_of, int32_t tracks, int64_t frames, int32_t J,
                        int32_t views, const double* cameras, double* sums, int32_t* terms, void* stream) {
    if (J > kRootMaxJoints) return UU3D_ERR_UNSUPPORTED;
    ViewStarts st;
    const int shape = view_starts(view_of, tracks, views, &st);
    if (shape != UU3D_OK) return shape;
    if (J < 1 || frames < 1 || frames > INT32_MAX / J) return UU3D_ERR_INVALID_ARGUMENT;      // (terms of one pair stay below 2^31)
    if (!kp || !cameras || !sums || !terms) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)kp & 7) != 0 || ((uintptr_t)cameras & 7) != 0 || ((uintptr_t)sums & 7) != 0 || ((uintptr_t)terms & 3) != 0)
        return UU3D_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(view_pair_sums_kernel, dim3((unsigned)(tracks * (tracks + 1) / 2)), dim3(kMatchLanes), 0, (hipStream_t)stream,
                       kp, joint_flags, st, cameras, tracks, (int)frames, J, views, sums, terms);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_group_views(const double* sums, const int32_t* terms, const int32_t* view_of, int32_t tracks, int32_t views, double max_dist,
                     int32_t min_terms, int32_t* person, int32_t* n_persons, int32_t* table, void* stream) {
    ViewStarts st;
    const int shape = view_starts(view_of, tracks, views, &st);
    if (shape != UU3D_OK) return shape;
    if (!(max_dist >= 0.0) || !std::isfinite(max_dist) || min_terms < 1) return UU3D_ERR_INVALID_ARGUMENT;
    if (!sums || !terms || !person || !n_persons || !table) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)sums & 7) != 0 || ((uintptr_t)terms & 3) != 0 || ((uintptr_t)person & 3) != 0 || ((uintptr_t)n_persons & 3) != 0 ||
        ((uintptr_t)table & 3) != 0)
        return UU3D_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(group_views_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, terms, st, tracks, views, max_dist, min_terms, person,
                       n_persons, table);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_gather_view_tracks(const int32_t* src, const float* poses, const float* kp2d, const uint8_t* joint_flags, int32_t views, int32_t persons,
                            int64_t frames, int32_t J, int32_t tracks, float* out_poses, float* out_kp2d, uint8_t* out_flags, void* stream) {
    if (views > kViewsMax || tracks > kMatchMaxTracks || persons > kMatchMaxTracks || J > kRootMaxJoints) return UU3D_ERR_UNSUPPORTED;
    if (views < 1 || tracks < 1 || persons < 1 || J < 1 || frames < 1 || frames > INT32_MAX / J) return UU3D_ERR_INVALID_ARGUMENT;
    if (!src || !poses || !kp2d || !out_poses || !out_kp2d || !out_flags) return UU3D_ERR_INVALID_ARGUMENT;
    if ((const void*)poses == (const void*)out_poses || (const void*)kp2d == (const void*)out_kp2d) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)src & 3) != 0 || ((uintptr_t)poses & 3) != 0 || ((uintptr_t)kp2d & 7) != 0 || ((uintptr_t)out_poses & 3) != 0 ||
        ((uintptr_t)out_kp2d & 7) != 0)
        return UU3D_ERR_INVALID_ARGUMENT;
    const int64_t lanes = (int64_t)views * persons * frames * J;         // at most 8 * 64 * (2^31 - 1): no overflow
    if ((lanes + 255) / 256 > INT32_MAX) return UU3D_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(gather_view_tracks_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       src, poses, kp2d, joint_flags, views, persons, (int)frames, J, tracks, out_poses, out_kp2d, out_flags);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}
