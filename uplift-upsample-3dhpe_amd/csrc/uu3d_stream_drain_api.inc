// uu3d_stream_drain_api.inc -- the host side of LIVE TRACKS: END OF A TRACK (uu3d_stream_drain.h; include/uu3d.h), a piece of uu3d_api.hip
// behind uu3d_stream_api.inc, whose prologue (stream_resolve), parameters (stream_params) and root checks (stream_root_resolve) it uses:
// the drain state, the commit of a drain tick, the root solve without filing, the scatter into the result rows, the reset.
namespace {
bool drain_slots_ok(const int32_t slots) { return slots >= 1 && slots <= (1 << 20); }
}  // namespace

size_t uu3d_stream_drain_bytes(int32_t slots) {
    return drain_slots_ok(slots) ? drain_layout(slots).bytes : 0;
}

int uu3d_stream_drain_layout(int32_t slots, uu3d_stream_drain_state_layout* out) {
    if (!out || !drain_slots_ok(slots)) return UU3D_ERR_INVALID_ARGUMENT;
    const DrainLayout D = drain_layout(slots);
    out->drained_offset = (int64_t)D.off_drained; out->virtual_frames_offset = (int64_t)D.off_virtual; out->ticked_offset = (int64_t)D.off_ticked;
    out->bytes = (int64_t)D.bytes;
    return UU3D_OK;
}

int uu3d_stream_drain_commit(uu3d_model* m, const uu3d_stream_config* s, const void* state, void* drain_state, const uint8_t* chosen,
                             const void* valid_state, int32_t* rows, uint8_t* stride_mask, uint8_t* fresh, void* stream) {
    if (!m) return UU3D_ERR_INVALID_ARGUMENT;
    StreamCall c;
    if (const int st = stream_resolve(m, s, nullptr, nullptr, state, kStreamState, "uu3d_stream_drain_commit", c)) return st;
    if (valid_state) if (const int st = stream_valid_check(m, "uu3d_stream_drain_commit")) return st;
    if (!drain_state || ((uintptr_t)drain_state & 255) != 0) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_stream_drain_commit: drain_state must be a 256-byte aligned block");
    if (!chosen || !rows || !stride_mask || !fresh) return fail(m, UU3D_ERR_INVALID_ARGUMENT, "uu3d_stream_drain_commit: null buffer");
    const StreamParams p = stream_params(m, s, c.L);
    const DrainLayout D = drain_layout(s->slots);
    char* d = (char*)drain_state;
    hipLaunchKernelGGL(stream_drain_commit_kernel, dim3(s->slots), dim3(256), 0, (hipStream_t)stream, p, chosen, (const int32_t*)(c.base + c.L.off_frames),
                       (int32_t*)(d + D.off_drained), (int32_t*)(d + D.off_virtual), (uint8_t*)(d + D.off_ticked), rows, stride_mask, fresh,
                       (const uint8_t*)valid_state);
    return launched(m, "uu3d_stream_drain_commit");
}

int uu3d_stream_root_drain(int32_t slots, int32_t J, int32_t lookahead, void* root_state, const void* drain_state, const uint8_t* chosen,
                           const uint8_t* fresh, const float* poses, const double* cameras, int32_t min_joints, float* roots, uint8_t* root_state_out,
                           void* stream) {
    RootRingLayout L;
    if (const int st = stream_root_resolve(slots, J, lookahead, root_state, L)) return st;
    if (!drain_state || ((uintptr_t)drain_state & 255) != 0) return UU3D_ERR_INVALID_ARGUMENT;
    if (!chosen || !fresh || !poses || !cameras || !roots || !root_state_out || min_joints < 2) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)poses & 3) != 0 || ((uintptr_t)cameras & 7) != 0 || ((uintptr_t)roots & 3) != 0) return UU3D_ERR_INVALID_ARGUMENT;
    char* b = (char*)root_state;
    const DrainLayout D = drain_layout(slots);
    hipLaunchKernelGGL(stream_root_drain_kernel, dim3((unsigned)((slots + 63) / 64)), dim3(64), 0, (hipStream_t)stream, slots, J, L.W,
                       (const int32_t*)((const char*)drain_state + D.off_virtual), chosen, fresh, poses, cameras, min_joints, (double*)(b + L.off_held),
                       (const float*)(b + L.off_kp), (const uint8_t*)(b + L.off_used), (uint8_t*)(b + L.off_last), roots, root_state_out);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_stream_drain_file(int32_t slots, int32_t lookahead, const void* drain_state, int32_t num_buffers, const float* const* src,
                           const int32_t* widths, float* const* dst, const uint8_t* fresh, uint8_t* fresh_rows, const uint8_t* root_state,
                           uint8_t* root_state_rows, void* stream) {
    if (!drain_slots_ok(slots) || lookahead < 1 || lookahead > (1 << 24) || num_buffers < 1 || num_buffers > kDrainFileBuffers) return UU3D_ERR_INVALID_ARGUMENT;
    if (!drain_state || ((uintptr_t)drain_state & 255) != 0 || !src || !widths || !dst || !fresh || !fresh_rows) return UU3D_ERR_INVALID_ARGUMENT;
    if ((root_state == nullptr) != (root_state_rows == nullptr)) return UU3D_ERR_INVALID_ARGUMENT;
    DrainFileParams f{};
    for (int b = 0; b < num_buffers; ++b) {
        if (!src[b] || !dst[b] || widths[b] < 1 || widths[b] > (1 << 20) || ((uintptr_t)src[b] & 3) != 0 || ((uintptr_t)dst[b] & 3) != 0 ||
            (const void*)src[b] == (const void*)dst[b])
            return UU3D_ERR_INVALID_ARGUMENT;
        f.src[b] = src[b]; f.dst[b] = dst[b]; f.width[b] = widths[b];
    }
    f.byte_src[0] = fresh; f.byte_dst[0] = fresh_rows; f.byte_src[1] = root_state; f.byte_dst[1] = root_state_rows;
    const DrainLayout D = drain_layout(slots);
    const char* d = (const char*)drain_state;
    hipLaunchKernelGGL(stream_drain_file_kernel, dim3((unsigned)slots), dim3(256), 0, (hipStream_t)stream, f, lookahead,
                       (const int32_t*)(d + D.off_drained), (const uint8_t*)(d + D.off_ticked));
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_stream_drain_reset(int32_t slots, void* drain_state, const uint8_t* slot_mask, void* stream) {
    if (!drain_slots_ok(slots) || !drain_state || ((uintptr_t)drain_state & 255) != 0) return UU3D_ERR_INVALID_ARGUMENT;
    const DrainLayout D = drain_layout(slots);
    char* d = (char*)drain_state;
    hipLaunchKernelGGL(stream_drain_reset_kernel, blocks_of(slots), dim3(256), 0, (hipStream_t)stream, slot_mask, slots, (int32_t*)(d + D.off_drained),
                       (int32_t*)(d + D.off_virtual), (uint8_t*)(d + D.off_ticked));
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}
