// uu3d_smooth_api.inc -- the host side of STEADY OUTPUT (uu3d_smooth.h; include/uu3d.h), a piece of uu3d_api.hip: the One-Euro filter over
// finished tracks (one launch) and the live filter of a session (its state block, one launch per push, the reset).  No model: the calls
// take the channel count, like uu3d_solve_roots and uu3d_stream_root, and run on any buffers.
namespace {
bool smooth_finite(const double v) { return v - v == 0.0; }
// the filter (min_cutoff > 0, beta >= 0, d_cutoff > 0), all finite
bool one_euro_params_ok(const double min_cutoff, const double beta, const double d_cutoff) {
    return smooth_finite(min_cutoff) && smooth_finite(beta) && smooth_finite(d_cutoff) && min_cutoff > 0.0 && beta >= 0.0 && d_cutoff > 0.0;
}
// slots and channels of a live call: UU3D_OK, or what is wrong (C beyond kSmoothMaxChannels: UU3D_ERR_UNSUPPORTED)
int stream_one_euro_resolve(const int32_t slots, const int32_t C, const int32_t lookahead, const void* state, OneEuroLayout& L) {
    if (C > kSmoothMaxChannels) return UU3D_ERR_UNSUPPORTED;
    if (slots < 1 || slots > (1 << 20) || C < 1 || lookahead < 0 || lookahead > (1 << 24)) return UU3D_ERR_INVALID_ARGUMENT;
    if (!state || ((uintptr_t)state & 255) != 0) return UU3D_ERR_INVALID_ARGUMENT;
    L = one_euro_layout(slots, C);
    return UU3D_OK;
}
}  // namespace

int uu3d_one_euro_tracks(const float* in, float* out, int64_t rows, int32_t C, const int64_t* track_start, const int64_t* track_len,
                         const double* rates, int32_t num_tracks, const uint8_t* state, double min_cutoff, double beta, double d_cutoff,
                         void* stream) {
    if (C > kSmoothMaxChannels) return UU3D_ERR_UNSUPPORTED;
    if (rows < 0 || C < 1 || num_tracks < 0 || num_tracks > (1 << 20) || rows > (INT64_MAX >> 4) / C) return UU3D_ERR_INVALID_ARGUMENT;
    if (!one_euro_params_ok(min_cutoff, beta, d_cutoff)) return UU3D_ERR_INVALID_ARGUMENT;
    if (rows == 0 || num_tracks == 0) return UU3D_OK;
    if (!in || !out || !track_start || !track_len || !rates || (const void*)in == (const void*)out) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)in & 3) != 0 || ((uintptr_t)out & 3) != 0 || ((uintptr_t)track_start & 7) != 0 || ((uintptr_t)track_len & 7) != 0 ||
        ((uintptr_t)rates & 7) != 0)
        return UU3D_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(one_euro_tracks_kernel, dim3((unsigned)num_tracks, (unsigned)((C + kSmoothLanes - 1) / kSmoothLanes)), dim3(kSmoothLanes), 0,
                       (hipStream_t)stream, in, out, (long)rows, C, track_start, track_len, rates, state, min_cutoff, beta, d_cutoff);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

// The zero-lag form: the arguments, the checks (in their order) and the grid of uu3d_one_euro_tracks, which stays as it is; the other kernel.
int uu3d_one_euro_tracks_two_pass(const float* in, float* out, int64_t rows, int32_t C, const int64_t* track_start, const int64_t* track_len,
                                  const double* rates, int32_t num_tracks, const uint8_t* state, double min_cutoff, double beta, double d_cutoff,
                                  void* stream) {
    if (C > kSmoothMaxChannels) return UU3D_ERR_UNSUPPORTED;
    if (rows < 0 || C < 1 || num_tracks < 0 || num_tracks > (1 << 20) || rows > (INT64_MAX >> 4) / C) return UU3D_ERR_INVALID_ARGUMENT;
    if (!one_euro_params_ok(min_cutoff, beta, d_cutoff)) return UU3D_ERR_INVALID_ARGUMENT;
    if (rows == 0 || num_tracks == 0) return UU3D_OK;
    if (!in || !out || !track_start || !track_len || !rates || (const void*)in == (const void*)out) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)in & 3) != 0 || ((uintptr_t)out & 3) != 0 || ((uintptr_t)track_start & 7) != 0 || ((uintptr_t)track_len & 7) != 0 ||
        ((uintptr_t)rates & 7) != 0)
        return UU3D_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(one_euro_tracks_two_pass_kernel, dim3((unsigned)num_tracks, (unsigned)((C + kSmoothLanes - 1) / kSmoothLanes)),
                       dim3(kSmoothLanes), 0, (hipStream_t)stream, in, out, (long)rows, C, track_start, track_len, rates, state, min_cutoff, beta,
                       d_cutoff);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

size_t uu3d_stream_one_euro_bytes(int32_t slots, int32_t C) {
    if (slots < 1 || slots > (1 << 20) || C < 1 || C > kSmoothMaxChannels) return 0;
    return one_euro_layout(slots, C).bytes;
}

int uu3d_stream_one_euro(int32_t slots, int32_t C, int32_t lookahead, void* filter_state, const int32_t* frames, const uint8_t* active,
                         const uint8_t* fresh, const float* values, const uint8_t* state, double rate, double min_cutoff, double beta,
                         double d_cutoff, float* out, void* stream) {
    OneEuroLayout L;
    if (const int st = stream_one_euro_resolve(slots, C, lookahead, filter_state, L)) return st;
    if (!frames || !active || !fresh || !values || !out || (const void*)values == (const void*)out) return UU3D_ERR_INVALID_ARGUMENT;
    if (((uintptr_t)frames & 3) != 0 || ((uintptr_t)values & 3) != 0 || ((uintptr_t)out & 3) != 0) return UU3D_ERR_INVALID_ARGUMENT;
    if (!one_euro_params_ok(min_cutoff, beta, d_cutoff) || !smooth_finite(rate) || !(rate > 0.0)) return UU3D_ERR_INVALID_ARGUMENT;
    char* b = (char*)filter_state;
    hipLaunchKernelGGL(stream_one_euro_kernel, dim3((unsigned)slots), dim3(kSmoothLanes), 0, (hipStream_t)stream, C, lookahead, frames, active, fresh,
                       values, state, rate, min_cutoff, beta, d_cutoff, (double*)(b + L.off_xh), (double*)(b + L.off_dxh), (int32_t*)(b + L.off_last),
                       (uint8_t*)(b + L.off_taken), out);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_stream_one_euro_reset(int32_t slots, int32_t C, void* filter_state, const uint8_t* slot_mask, void* stream) {
    OneEuroLayout L;
    if (const int st = stream_one_euro_resolve(slots, C, 0, filter_state, L)) return st;
    char* b = (char*)filter_state;
    hipLaunchKernelGGL(stream_one_euro_reset_kernel, dim3((unsigned)slots), dim3(256), 0, (hipStream_t)stream, slot_mask, C, (double*)(b + L.off_xh),
                       (double*)(b + L.off_dxh), (int32_t*)(b + L.off_last), (uint8_t*)(b + L.off_taken));
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}
