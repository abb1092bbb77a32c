// uu3d_stream_views_api.inc -- the host side of LIVE SEVERAL VIEWS (uu3d_stream_views.h; include/uu3d.h), a piece of uu3d_api.hip behind
// uu3d_stream_api.inc, whose root checks (stream_root_resolve) it uses: the launch of a push and the reset.  No model: the calls take the
// view, person and joint counts.  Every guard comes before any HIP call.

namespace {
// views and persons of a call and its state block: UU3D_OK, or what is wrong (V beyond 8: UU3D_ERR_UNSUPPORTED)
int stream_views_resolve(const int32_t views, const int32_t persons, const void* state, ViewsStateLayout& L) {
    if (views > kViewsMax) return UU3D_ERR_UNSUPPORTED;
    if (views < 1 || persons < 1 || (int64_t)views * persons > (1 << 20)) return UU3D_ERR_INVALID_ARGUMENT;
    if (!state || ((uintptr_t)state & 255) != 0) return UU3D_ERR_INVALID_ARGUMENT;
    L = views_state_layout(persons);
    return UU3D_OK;
}
}  // namespace

size_t uu3d_stream_views_bytes(int32_t views, int32_t persons) {
    if (views < 1 || views > kViewsMax || persons < 1 || (int64_t)views * persons > (1 << 20)) return 0;
    return views_state_layout(persons).bytes;
}

int uu3d_stream_views(int32_t views, int32_t persons, int32_t J, int32_t lookahead, void* views_state, const void* root_state, const int32_t* frames,
                      const uint8_t* active, const uint8_t* fresh, const float* view_poses, const double* cameras, int32_t min_joints, float* poses,
                      uint8_t* fresh_out, float* roots, uint8_t* root_state_out, uint8_t* view_count, int32_t* person_frames, uint8_t* person_active,
                      void* stream) {
    ViewsStateLayout L;
    RootRingLayout R;
    if (const int st = stream_views_resolve(views, persons, views_state, L)) return st;
    if (const int st = stream_root_resolve(views * persons, J, lookahead, root_state, R)) return st;
    if (!frames || !active || !fresh || !view_poses || !cameras || !poses || !fresh_out || !roots || !root_state_out || !view_count || !person_frames ||
        !person_active || min_joints < 2 || (const void*)view_poses == (const void*)poses)
        return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)frames & 3) != 0 || ((uintptr_t)view_poses & 3) != 0 || ((uintptr_t)cameras & 7) != 0 || ((uintptr_t)poses & 3) != 0 ||
        ((uintptr_t)roots & 3) != 0 || ((uintptr_t)person_frames & 3) != 0)
        return UU3D_ERR_INVALID_ARGUMENT;
    char* b = (char*)views_state;
    const char* ring = (const char*)root_state;
    hipLaunchKernelGGL(stream_views_kernel, dim3((unsigned)persons), dim3(64), 0, (hipStream_t)stream, views, persons, J, R.W, frames, active, fresh,
                       view_poses, (const float*)(ring + R.off_kp), (const uint8_t*)(ring + R.off_used), cameras, min_joints, (double*)(b + L.off_held),
                       (uint8_t*)(b + L.off_last), (int32_t*)(b + L.off_ticks), poses, fresh_out, roots, root_state_out, view_count, person_frames,
                       person_active);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_stream_views_reset(int32_t views, int32_t persons, void* views_state, const uint8_t* slot_mask, void* stream) {
    ViewsStateLayout L;
    if (const int st = stream_views_resolve(views, persons, views_state, L)) return st;
    char* b = (char*)views_state;
    hipLaunchKernelGGL(stream_views_reset_kernel, dim3((unsigned)((persons + 255) / 256)), dim3(256), 0, (hipStream_t)stream, slot_mask, views, persons,
                       (double*)(b + L.off_held), (uint8_t*)(b + L.off_last), (int32_t*)(b + L.off_ticks));
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}
