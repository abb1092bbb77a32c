// uu3d_bones_api.inc -- the host side of CONSTANT BONE LENGTHS (uu3d_bones.h; include/uu3d.h), a piece of uu3d_api.hip: the lengths of
// finished tracks and their fix (one launch each) and the live form of a session (its state block, one launch per push, the reset).  No
// model: the calls take the joint count, like uu3d_solve_roots and uu3d_one_euro_tracks, and run on any buffers.  Every guard comes
// before any HIP call.
namespace {
bool bones_aligned(const void* p, const uintptr_t mask) { return ((uintptr_t)p & mask) == 0; }
// slots, joints and tree tables of a live call: UU3D_OK, or what is wrong (J beyond kBonesMaxJoints: UU3D_ERR_UNSUPPORTED)
int stream_bones_resolve(const int32_t slots, const int32_t J, const void* state, BonesLayout& L) {
    if (J > kBonesMaxJoints) return UU3D_ERR_UNSUPPORTED;
    if (slots < 1 || slots > (1 << 20) || J < 1) return UU3D_ERR_INVALID_ARGUMENT;
    if (!state || !bones_aligned(state, 255)) return UU3D_ERR_INVALID_ARGUMENT;
    L = bones_layout(slots, J);
    return UU3D_OK;
}
}  // namespace

int uu3d_bone_lengths(const float* poses, int64_t rows, int32_t J, const int32_t* parents, const int64_t* track_start, const int64_t* track_len,
                      int32_t num_tracks, double* lengths, int64_t* counts, void* stream) {
    if (J > kBonesMaxJoints) return UU3D_ERR_UNSUPPORTED;
    if (rows < 0 || J < 1 || num_tracks < 0 || num_tracks > (1 << 20) || rows > ((int64_t)1 << 40)) return UU3D_ERR_INVALID_ARGUMENT;
    if (rows == 0 || num_tracks == 0) return UU3D_OK;
    if (!poses || !parents || !track_start || !track_len || !lengths) return UU3D_ERR_INVALID_ARGUMENT;
    if (!bones_aligned(poses, 3) || !bones_aligned(parents, 3) || !bones_aligned(track_start, 7) || !bones_aligned(track_len, 7) ||
        !bones_aligned(lengths, 7) || !bones_aligned(counts, 7))
        return UU3D_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(bone_lengths_kernel, dim3((unsigned)num_tracks, (unsigned)((J + kBonesLanes - 1) / kBonesLanes)), dim3(kBonesLanes), 0,
                       (hipStream_t)stream, poses, (long)rows, J, parents, track_start, track_len, lengths, counts);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_fix_bones(const float* in, float* out, int64_t rows, int32_t J, const int32_t* parents, const int32_t* paths, int32_t depth,
                   const int32_t* row_track, int32_t num_tracks, const double* lengths, void* stream) {
    if (J > kBonesMaxJoints) return UU3D_ERR_UNSUPPORTED;
    if (rows < 0 || J < 1 || depth < 1 || depth > kBonesMaxJoints || num_tracks < 1 || num_tracks > (1 << 20) || rows > ((int64_t)1 << 32))
        return UU3D_ERR_INVALID_ARGUMENT;
    if (rows == 0) return UU3D_OK;
    if (!in || !out || !parents || !paths || !lengths || (const void*)in == (const void*)out) return UU3D_ERR_INVALID_ARGUMENT;
    if (!bones_aligned(in, 3) || !bones_aligned(out, 3) || !bones_aligned(parents, 3) || !bones_aligned(paths, 3) || !bones_aligned(row_track, 3) ||
        !bones_aligned(lengths, 7))
        return UU3D_ERR_INVALID_ARGUMENT;
    const int64_t lanes = rows * J;                                      // (<= 2^38: the grid stays below 2^31 workgroups)
    hipLaunchKernelGGL(fix_bones_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, out, (long)rows, J, parents,
                       paths, depth, row_track, num_tracks, lengths);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

size_t uu3d_stream_bones_bytes(int32_t slots, int32_t J) {
    if (slots < 1 || slots > (1 << 20) || J < 1 || J > kBonesMaxJoints) return 0;
    return bones_layout(slots, J).bytes;
}

int uu3d_stream_bones(int32_t slots, int32_t J, void* bones_state, const int32_t* parents, const int32_t* paths, int32_t depth,
                      const uint8_t* active, const uint8_t* fresh, const float* poses, const double* given_lengths, float* out,
                      double* lengths_out, void* stream) {
    BonesLayout L;
    if (const int st = stream_bones_resolve(slots, J, bones_state, L)) return st;
    if (depth < 1 || depth > kBonesMaxJoints) return UU3D_ERR_INVALID_ARGUMENT;
    if (!parents || !paths || !active || !fresh || !poses || !out || (const void*)poses == (const void*)out) return UU3D_ERR_INVALID_ARGUMENT;
    if (!bones_aligned(parents, 3) || !bones_aligned(paths, 3) || !bones_aligned(poses, 3) || !bones_aligned(out, 3) ||
        !bones_aligned(given_lengths, 7) || !bones_aligned(lengths_out, 7))
        return UU3D_ERR_INVALID_ARGUMENT;
    char* b = (char*)bones_state;
    hipLaunchKernelGGL(stream_bones_kernel, dim3((unsigned)slots), dim3(kBonesLanes), 0, (hipStream_t)stream, J, parents, paths, depth, active, fresh,
                       poses, given_lengths, (double*)(b + L.off_sum), (int32_t*)(b + L.off_count), out, lengths_out);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_stream_bones_reset(int32_t slots, int32_t J, void* bones_state, const uint8_t* slot_mask, void* stream) {
    BonesLayout L;
    if (const int st = stream_bones_resolve(slots, J, bones_state, L)) return st;
    char* b = (char*)bones_state;
    hipLaunchKernelGGL(stream_bones_reset_kernel, dim3((unsigned)slots), dim3(kBonesLanes), 0, (hipStream_t)stream, slot_mask, J,
                       (double*)(b + L.off_sum), (int32_t*)(b + L.off_count));
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}
