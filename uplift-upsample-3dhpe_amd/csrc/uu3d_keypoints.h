// uu3d_keypoints.h -- ANY SKELETON (include/uu3d.h; predict.predict_tracks(keypoints=M), stream.StreamSession(keypoints=M)): the joints a
// detector emits (COCO-17, BODY_25, ...) -> the joints the model was trained on, one affine map applied on the device in front of
// everything else that looks at a track (uu3d_repair_joints, the kernels of uu3d_tracks.h, the stage of a live tick).  One launch, one
// lane per (frame, model joint), one 8-byte store of the coordinate pair and one byte of the joint's flag; every element has one writer
// and is a function of inputs that nobody writes: bitwise repeatable, no atomics.  The table is packed and range-checked on the host
// (keypoint_map_pack); the kernel trusts it.
#pragma once
#include "uu3d_tracks.h"

namespace uu3d {

static constexpr int kKeypointSources = 8;                              // the table's fixed stride: sources per model joint

// The device-resident table of a map onto J model joints, three planes back to back (the f64 plane first: the block is 8-byte aligned):
//     w   (J, 8) f64 at 0          src (J, 8) i32 at 64 J, -1 for an unused entry          n (J) i32 at 96 J
struct KeypointTable { const double* w; const int32_t* src; const int32_t* n; };
__host__ __device__ inline size_t keypoint_table_bytes(const long J) { return ((size_t)J * 100 + 7) / 8 * 8; }
__host__ __device__ inline KeypointTable keypoint_table(const void* base, const long J)
{
    const char* b = static_cast<const char*>(base);
    return KeypointTable{reinterpret_cast<const double*>(b), reinterpret_cast<const int32_t*>(b + (size_t)J * 64),
                         reinterpret_cast<const int32_t*>(b + (size_t)J * 96)};
}

// w[0] * (double)x[0] + w[1] * (double)x[1] + ... in float64, left to right, every product and every sum rounded (no fused multiply-add),
// rounded once to float32 -- numpy's own expression (predict.map_keypoints_host), the discipline of resample_mix.  One term of it:
__device__ __forceinline__ double keypoint_add_term(const double acc, const double w, const float x, const bool first)
{
#pragma clang fp contract(off)
    const double term = w * (double)x;
    return first ? term : acc + term;
}
// ... and its one rounding.  A NaN result is stored as THE quiet NaN 0x7fc00000: which NaN an invalid sum (Inf - Inf) makes differs
// between processors, and host and device must agree.
__device__ __forceinline__ float keypoint_round(const double acc)
{
    const float r = (float)acc;
    return (__float_as_uint(r) & 0x7fffffffu) > 0x7f800000u ? __uint_as_float(0x7fc00000u) : r;
}

// out (frames, J, 2) and, with flags, flags_out (frames, J): lane p = frame * J + j.  Only the listed sources are read.  flags_in
// (frames, inputs) u8 or nullptr; with flags a source is OBSERVED when its byte is non-zero and both coordinates are finite, the model
// joint is observed iff every one of its sources is, and an unobserved joint is written as zeros with flag 0.  Without flags the
// expression alone: a NaN source gives a NaN joint.
static __global__ void __launch_bounds__(256)
map_keypoints_kernel(const KeypointTable map, const int inputs, const int J, const float* __restrict__ src, const uint8_t* __restrict__ flags_in,
                     const long frames, float* __restrict__ out, uint8_t* __restrict__ flags_out)
{
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= frames * J) return;
    const long f = p / J;
    const int j = (int)(p - f * J);
    const int n = map.n[j];
    double ax = 0.0, ay = 0.0;
    bool observed = true;
    for (int k = 0; k < n; ++k) {
        const long s = f * inputs + map.src[j * kKeypointSources + k];
        const double w = map.w[j * kKeypointSources + k];
        const float2 v = *reinterpret_cast<const float2*>(src + s * 2);
        ax = keypoint_add_term(ax, w, v.x, k == 0);
        ay = keypoint_add_term(ay, w, v.y, k == 0);
        if (flags_in != nullptr) observed = observed && flags_in[s] != 0 && finite_pair(v);
    }
    const float2 r = observed ? make_float2(keypoint_round(ax), keypoint_round(ay)) : make_float2(0.f, 0.f);
    *reinterpret_cast<float2*>(out + p * 2) = r;
    if (flags_out != nullptr) flags_out[p] = observed ? 1 : 0;
}

// The host half: a map given as (J, 8) planes -- sources[j * 8 + k] for k < counts[j], anything behind -- checked and written into `out`
// in the table's layout.  nullptr = fine, else what is wrong.  What the kernel relies on is checked HERE: 1 <= counts[j] <= 8 and every
// listed source in [0, inputs); and the rule's own terms: sources of a joint distinct, weights finite and non-zero, summing to 1 within 1e-12.
inline const char* keypoint_map_pack(const int inputs, const int J, const int32_t* counts, const int32_t* sources, const double* weights, void* out)
{
    char* b = static_cast<char*>(out);
    double* w = reinterpret_cast<double*>(b);
    int32_t* s = reinterpret_cast<int32_t*>(b + (size_t)J * 64);
    int32_t* n = reinterpret_cast<int32_t*>(b + (size_t)J * 96);
    for (int j = 0; j < J; ++j) {
        if (counts[j] < 1 || counts[j] > kKeypointSources) return "every model joint needs 1 to 8 sources";
        double sum = 0.0;
        for (int k = 0; k < kKeypointSources; ++k) {
            const bool used = k < counts[j];
            const int32_t idx = used ? sources[j * kKeypointSources + k] : -1;
            const double wk = used ? weights[j * kKeypointSources + k] : 0.0;
            if (used) {
                if (idx < 0 || idx >= inputs) return "a source index is outside [0, inputs)";
                for (int q = 0; q < k; ++q) if (s[j * kKeypointSources + q] == idx) return "the sources of a model joint must be distinct";
                if (!std::isfinite(wk) || wk == 0.0) return "weights must be finite and non-zero";
                sum += wk;
            }
            s[j * kKeypointSources + k] = idx;
            w[j * kKeypointSources + k] = wk;
        }
        if (!(std::fabs(sum - 1.0) <= 1e-12)) return "the weights of a model joint must sum to 1";
        n[j] = counts[j];
    }
    return nullptr;
}

}  // namespace uu3d
