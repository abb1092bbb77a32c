// uu3d_view_align_api.inc -- the host side of ONE CLOCK (uu3d_view_align.h; include/uu3d.h), a piece of uu3d_api.hip: the launches.
// No model and no state.  Every guard comes before any HIP call; view_of and first_row are HOST memory, so their order is a guard too.

// The reference view = the first non-empty view, and its number of tracks.
static void align_reference(const ViewStarts& st, int32_t views, int* ref_view, int* n_ref) {
    int r = 0;
    while (r + 1 < views && st.start[r + 1] <= st.start[r]) ++r;
    *ref_view = r;
    *n_ref = st.start[r + 1] - st.start[r];
}

static int align_shape(const int32_t* view_of, int32_t tracks, int32_t views, int32_t max_lag, ViewStarts* st) {
    if (max_lag > kAlignMaxLag) return UU3D_ERR_UNSUPPORTED;
    const int shape = view_starts(view_of, tracks, views, st);
    if (shape != UU3D_OK) return shape;
    return max_lag < 1 ? UU3D_ERR_INVALID_ARGUMENT : UU3D_OK;
}

size_t uu3d_view_lag_scratch_bytes(int64_t rows, int32_t J) {
    if (rows < 1 || J < 1 || J > kRootMaxJoints || rows > INT64_MAX / (32 * (int64_t)J)) return 0;
    return (view_lag_used_offset(rows, J) + (size_t)rows * (size_t)J + 7) & ~(size_t)7;
}

int uu3d_view_lag_sums(const float* kp, const uint8_t* joint_flags, const int32_t* view_of, const int64_t* first_row, int32_t tracks, int32_t J,
                       int32_t views, const double* cameras, int32_t max_lag, void* scratch, double* sums, int32_t* terms, void* stream) {
    if (J > kRootMaxJoints) return UU3D_ERR_UNSUPPORTED;
    ViewStarts st;
    const int shape = align_shape(view_of, tracks, views, max_lag, &st);
    if (shape != UU3D_OK) return shape;
    if (J < 1 || !first_row || first_row[0] < 0) return UU3D_ERR_INVALID_ARGUMENT;
    TrackRows rows;
    int64_t longest = 0;
    for (int32_t m = 0; m <= kMatchMaxTracks; ++m) rows.first[m] = 0;
    rows.first[0] = (long)first_row[0];
    for (int32_t m = 0; m < tracks; ++m) {
        if (first_row[m + 1] <= first_row[m]) return UU3D_ERR_INVALID_ARGUMENT;                // every track has a frame
        const int64_t frames = first_row[m + 1] - first_row[m];
        if (frames > INT32_MAX / J) return UU3D_ERR_INVALID_ARGUMENT;                          // (terms of one reduction stay below 2^31)
        if (frames > longest) longest = frames;
        rows.first[m + 1] = (long)first_row[m + 1];
    }
    if (first_row[tracks] > INT64_MAX / (32 * (int64_t)J)) return UU3D_ERR_INVALID_ARGUMENT;
    if (!kp || !cameras || !scratch || !sums || !terms) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)kp & 7) != 0 || ((uintptr_t)cameras & 7) != 0 || ((uintptr_t)scratch & 7) != 0 || ((uintptr_t)sums & 7) != 0 ||
        ((uintptr_t)terms & 3) != 0)
        return UU3D_ERR_INVALID_ARGUMENT;
    int ref_view, n_ref;
    align_reference(st, views, &ref_view, &n_ref);
    double* rays = (double*)scratch;
    uint8_t* used = (uint8_t*)scratch + view_lag_used_offset(first_row[tracks], J);
    hipLaunchKernelGGL(view_lag_rays_kernel, dim3((unsigned)((longest * J + 255) / 256), (unsigned)tracks), dim3(256), 0, (hipStream_t)stream,
                       kp, joint_flags, st, rows, cameras, J, views, rays, used);
    hipLaunchKernelGGL(view_lag_sums_kernel, dim3((unsigned)(2 * max_lag + 1), (unsigned)tracks, (unsigned)n_ref), dim3(kMatchLanes), 0,
                       (hipStream_t)stream, rays, used, st, rows, cameras, tracks, J, views, n_ref, ref_view, max_lag, sums, terms);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_view_offsets(const double* sums, const int32_t* terms, const int32_t* view_of, int32_t tracks, int32_t views, int32_t max_lag,
                      int32_t min_terms, int32_t same_index, int32_t* offset, int32_t* state, double* score, void* stream) {
    ViewStarts st;
    const int shape = align_shape(view_of, tracks, views, max_lag, &st);
    if (shape != UU3D_OK) return shape;
    if (min_terms < 1) return UU3D_ERR_INVALID_ARGUMENT;
    int ref_view, n_ref;
    align_reference(st, views, &ref_view, &n_ref);
    if (same_index != 0)
        for (int32_t v = 0; v < views; ++v) {
            const int nb = st.start[v + 1] - st.start[v];
            if (nb > 0 && nb != n_ref) return UU3D_ERR_INVALID_ARGUMENT;                       // the same index needs the same counts
        }
    if (!sums || !terms || !offset || !state || !score) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)sums & 7) != 0 || ((uintptr_t)terms & 3) != 0 || ((uintptr_t)offset & 3) != 0 || ((uintptr_t)state & 3) != 0 ||
        ((uintptr_t)score & 7) != 0)
        return UU3D_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(view_offsets_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, terms, st, tracks, views, n_ref, ref_view, max_lag,
                       min_terms, same_index, offset, state, score);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}
