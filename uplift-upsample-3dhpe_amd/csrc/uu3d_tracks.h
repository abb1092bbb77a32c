// uu3d_tracks.h -- the front and the back of predict.predict_tracks (include/uu3d.h, "YOUR OWN 2D TRACKS"): pixel coordinates of the
// caller's keypoint tracks -> the pose table the window gather reads, and the central predictions of the forwarded windows -> one 3D pose
// per frame of every track; resample_tracks_kernel is the front for tracks at another frame rate, assemble_tracks_cubic_kernel the back with
// a C1 cubic between the predicted frames in place of the line.  All four: one launch for all tracks of
// a call, one thread per 16 bytes of the flattened output, every output element written by exactly one thread from inputs nobody writes
// (bitwise repeatable; the in-place form of the first kernel reads only what the same thread overwrites).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace uu3d {

// h36m.normalize_screen_coordinates (common/dataset/camera.py:15-20: X / w * 2 - [1, h / w]) on float32 coordinates, in numpy's types
// and order: the quotient and the doubling in float32 (w rounded to float32), then the subtraction of the float64 list [1, h / w] in
// float64, rounded once to float32 when it is stored.
__device__ __forceinline__ float2 normalize_pair(const float2 p, const float wf, const double h_over_w)
{
    const float x = __fdiv_rn(p.x, wf) * 2.0f, y = __fdiv_rn(p.y, wf) * 2.0f;
    return make_float2((float)((double)x - 1.0), (float)((double)y - h_over_w));
}

// Neither coordinate is NaN or +-Inf (the exponent bits: no floating-point compare a compiler flag could fold away).
__device__ __forceinline__ bool finite_pair(const float2 p)
{
    return (__float_as_uint(p.x) & 0x7f800000u) != 0x7f800000u && (__float_as_uint(p.y) & 0x7f800000u) != 0x7f800000u;
}

// Which source row a table row takes.  key_stride == 0: its own.  key_stride > 0: src holds only the frames 0, key_stride, 2 key_stride, ...
// of every track back to back (track t from row src_start[t]); frame f of track t (table row track_start[t] + f) takes source row
// src_start[t] + f / key_stride when f % key_stride == 0.  kTrackRowNotGiven: a frame between two keyframes; kTrackRowBad: a track id or a
// source row out of range.  One statement for normalize_tracks_kernel and track_valid_kernel.
static constexpr long kTrackRowNotGiven = -1, kTrackRowBad = -2;
__device__ __forceinline__ long track_source_row(const long row, const long src_rows, const int32_t* __restrict__ row_track, const int num_tracks,
                                                 const int64_t* __restrict__ track_start, const int64_t* __restrict__ src_start, const int key_stride)
{
    const int t = row_track[row];
    if (t < 0 || t >= num_tracks) return kTrackRowBad;
    long srow = row;
    if (key_stride > 0) {
        const long f = row - track_start[t];
        if (f < 0) return kTrackRowBad;
        if (f % key_stride != 0) return kTrackRowNotGiven;
        srow = src_start[t] + f / key_stride;
    }
    return (srow < 0 || srow >= src_rows) ? kTrackRowBad : srow;
}

// table (rows, J, 2): row r belongs to track row_track[r] and takes the source row track_source_row names: normalised with res (T, 2)
// float64 = (w, h) per track, or copied as it is (res == nullptr; src == table allowed when key_stride == 0).  A row that is not given is
// zero; a track id or a source row out of range writes NaN instead of reading out of bounds.  valid (rows) u8 or nullptr: a row whose byte
// is 0 (a missing frame, track_valid_kernel) is written as zeros whatever its source holds.
static __global__ void __launch_bounds__(256)
normalize_tracks_kernel(const float* src, const long src_rows, float* table, const long rows, const int J, const int32_t* __restrict__ row_track,
                        const int num_tracks, const double* __restrict__ res, const int64_t* __restrict__ track_start,
                        const int64_t* __restrict__ src_start, const int key_stride, const uint8_t* __restrict__ valid)
{
    const long pairs = rows * J;
    const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * 2;         // two (x, y) pairs = one 16-byte store
    if (p0 >= pairs) return;
    float2 v[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const long p = (p0 + e < pairs) ? p0 + e : p0;
        const long row = p / J;
        const int j = (int)(p - row * J);
        const float nan = __builtin_nanf("");
        v[e] = make_float2(nan, nan);
        const long srow = track_source_row(row, src_rows, row_track, num_tracks, track_start, src_start, key_stride);
        if (srow == kTrackRowBad) continue;
        if (srow == kTrackRowNotGiven || (valid != nullptr && valid[row] == 0)) { v[e] = make_float2(0.f, 0.f); continue; }
        const int t = row_track[row];
        const float2 x = *reinterpret_cast<const float2*>(src + (srow * J + j) * 2);
        v[e] = (res != nullptr) ? normalize_pair(x, (float)res[2 * t], res[2 * t + 1] / res[2 * t]) : x;
    }
    if (p0 + 1 < pairs) *reinterpret_cast<float4*>(table + p0 * 2) = make_float4(v[0].x, v[0].y, v[1].x, v[1].y);
    else *reinterpret_cast<float2*>(table + p0 * 2) = v[0];
}

// MISSED DETECTIONS: valid_out[row] = the frame of table row `row` is a real observation -- its source row's byte of valid_in (src_rows, or
// nullptr = all given as valid) is non-zero AND all 2 J coordinates of the source row are finite.  A row that is not given (between two
// keyframes) and a row out of range keep 1: they behave as without validity (zeros / NaN).  One wave per table row, four rows per
// workgroup; lane 0 writes the row's byte.  It runs BEFORE normalize_tracks_kernel on the same stream and only reads src, so the
// in-place form (src == table) sees the caller's coordinates, not rows that are already rewritten.
static __global__ void __launch_bounds__(256)
track_valid_kernel(const float* __restrict__ src, const long src_rows, const long rows, const int J, const int32_t* __restrict__ row_track,
                   const int num_tracks, const int64_t* __restrict__ track_start, const int64_t* __restrict__ src_start, const int key_stride,
                   const uint8_t* __restrict__ valid_in, uint8_t* __restrict__ valid_out)
{
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                             // (whole waves leave: `row` is uniform in a wave)
    const long srow = track_source_row(row, src_rows, row_track, num_tracks, track_start, src_start, key_stride);
    bool ok = true;
    if (srow >= 0) {
        for (int j = lane; j < J; j += 64) {
            const float2 x = *reinterpret_cast<const float2*>(src + (srow * J + j) * 2);
            ok = ok && finite_pair(x);
        }
        ok = __all(ok) != 0 && (valid_in == nullptr || valid_in[srow] != 0);
    }
    if (lane == 0) valid_out[row] = ok ? 1 : 0;
}

// ANY FRAME RATE (predict.resample_plan): table row `row` -- a frame of the model's time grid -- is source row left[row] where
// left == right, else the two source rows mixed with weight[row] in float64.  One source pair as the table takes it: normalised with the
// track's (w, h), or as it is.
__device__ __forceinline__ float2 resample_source_pair(const float* src, const long srow, const int J, const int j, const bool normalise, const float wf,
                                                       const double h_over_w)
{
    const float2 x = *reinterpret_cast<const float2*>(src + (srow * J + j) * 2);
    return normalise ? normalize_pair(x, wf, h_over_w) : x;
}

// a * (1.0 - w) + b * w in float64: two products and one sum, each rounded (no fused multiply-add), then rounded to float32 -- numpy's
// own expression (evaluation.interpolate_between_keyframes), so that a numpy restatement gives the same bits.
__device__ __forceinline__ float resample_mix(const float a, const float b, const double w)
{
#pragma clang fp contract(off)
    const double pa = (double)a * (1.0 - w);
    const double pb = (double)b * w;
    return (float)(pa + pb);
}

// table (rows, J, 2) from src (src_rows, J, 2), never in place: one thread per two (x, y) pairs = one 16-byte store.  A track id or a
// plan row out of range writes NaN instead of reading out of bounds; a row whose byte of valid (rows, or nullptr) is 0 is written as
// zeros.  Where left == right the right row is not read.
static __global__ void __launch_bounds__(256)
resample_tracks_kernel(const float* __restrict__ src, const long src_rows, float* __restrict__ table, const long rows, const int J,
                       const int32_t* __restrict__ row_track, const int num_tracks, const double* __restrict__ res, const int64_t* __restrict__ left,
                       const int64_t* __restrict__ right, const double* __restrict__ weight, const uint8_t* __restrict__ valid)
{
    const long pairs = rows * J;
    const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * 2;
    if (p0 >= pairs) return;
    float2 v[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const long p = (p0 + e < pairs) ? p0 + e : p0;
        const long row = p / J;
        const int j = (int)(p - row * J);
        const float nan = __builtin_nanf("");
        v[e] = make_float2(nan, nan);
        const int t = row_track[row];
        const long l = left[row], r = right[row];
        if (t < 0 || t >= num_tracks || l < 0 || l >= src_rows || r < 0 || r >= src_rows) continue;
        if (valid != nullptr && valid[row] == 0) { v[e] = make_float2(0.f, 0.f); continue; }
        const bool normalise = res != nullptr;
        const float wf = normalise ? (float)res[2 * t] : 1.0f;
        const double h_over_w = normalise ? res[2 * t + 1] / res[2 * t] : 1.0;
        const float2 a = resample_source_pair(src, l, J, j, normalise, wf, h_over_w);
        v[e] = a;
        if (l == r) continue;
        const float2 b = resample_source_pair(src, r, J, j, normalise, wf, h_over_w);
        const double w = weight[row];
        v[e] = make_float2(resample_mix(a.x, b.x, w), resample_mix(a.y, b.y, w));
    }
    if (p0 + 1 < pairs) *reinterpret_cast<float4*>(table + p0 * 2) = make_float4(v[0].x, v[0].y, v[1].x, v[1].y);
    else *reinterpret_cast<float2*>(table + p0 * 2) = v[0];
}

// valid_out[row] = the model frame of table row `row` is a real observation: its left source row is valid (valid_in (src_rows) non-zero,
// nullptr = all) with all 2 J coordinates finite, and where left != right the right one too.  A row whose plan or track id is out of range
// keeps 1: it behaves as without validity (NaN).  One wave per table row, four rows per workgroup, lane 0 writes the byte, as
// track_valid_kernel; it runs before resample_tracks_kernel on the same stream.
static __global__ void __launch_bounds__(256)
resample_valid_kernel(const float* __restrict__ src, const long src_rows, const long rows, const int J, const int32_t* __restrict__ row_track,
                      const int num_tracks, const int64_t* __restrict__ left, const int64_t* __restrict__ right,
                      const uint8_t* __restrict__ valid_in, uint8_t* __restrict__ valid_out)
{
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                             // (whole waves leave: `row` is uniform in a wave)
    const int t = row_track[row];
    const long l = left[row], r = right[row];
    bool ok = true;
    if (t >= 0 && t < num_tracks && l >= 0 && l < src_rows && r >= 0 && r < src_rows) {
        for (int j = lane; j < J; j += 64) {
            ok = ok && finite_pair(*reinterpret_cast<const float2*>(src + (l * J + j) * 2));
            if (l != r) ok = ok && finite_pair(*reinterpret_cast<const float2*>(src + (r * J + j) * 2));
        }
        ok = __all(ok) != 0 && (valid_in == nullptr || (valid_in[l] != 0 && (l == r || valid_in[r] != 0)));
    }
    if (lane == 0) valid_out[row] = ok ? 1 : 0;
}

// The prediction of one window: the plain central prediction, or its mean with the un-flipped mirrored one (eval.py:163-166: x negated,
// joints permuted by AUGM_FLIP_KEYPOINT_ORDER, (a + b) / 2 in float32 -- eval._unflip).
__device__ __forceinline__ float window_prediction(const float* __restrict__ plain, const float* __restrict__ flipped, const int32_t* __restrict__ order,
                                                   const long row, const int J, const int j, const int c)
{
    const float p = plain[(row * J + j) * 3 + c];
    if (flipped == nullptr) return p;
    float q = flipped[(row * J + order[j]) * 3 + c];
    if (c == 0) q = q * -1.0f;
    return (p + q) / 2.0f;
}

// Coordinate c of joint j of frame f by the plan of evaluation.keyframe_plan: the prediction of window left[f] where left == right (a
// predicted frame, or a frame behind its track's last predicted one), else evaluation.interpolate_between_keyframes' own expression
// pred[left] * (1.0 - w) + pred[right] * w in float64, rounded to float32 as numpy stores it into the float32 array (resample_mix).  A row
// outside [0, num_windows) gives NaN.
__device__ __forceinline__ float frame_value(const float* __restrict__ plain, const float* __restrict__ flipped, const int32_t* __restrict__ order,
                                             const long num_windows, const long l, const long r, const double w, const int J, const int j, const int c)
{
    if (l < 0 || l >= num_windows || r < 0 || r >= num_windows) return __builtin_nanf("");
    const float a = window_prediction(plain, flipped, order, l, J, j, c);
    if (l == r) return a;
    return resample_mix(a, window_prediction(plain, flipped, order, r, J, j, c), w);
}

// out (frames, J, 3), flattened: one thread per four consecutive floats.  root >= 0: the frame's root joint is subtracted in float32
// (that joint comes out exactly 0).
static __global__ void __launch_bounds__(256)
assemble_tracks_kernel(const float* __restrict__ plain, const float* __restrict__ flipped, const long num_windows, const int32_t* __restrict__ order,
                       const int32_t* __restrict__ left, const int32_t* __restrict__ right, const double* __restrict__ weight, const long frames,
                       const int J, const int root, float* __restrict__ out)
{
    const long per = (long)J * 3, total = frames * per;
    const long e0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (e0 >= total) return;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long e = (e0 + k < total) ? e0 + k : e0;
        const long f = e / per;
        const int r = (int)(e - f * per), j = r / 3, c = r - j * 3;
        const long l = left[f], rr = right[f];
        const double w = weight[f];
        v[k] = frame_value(plain, flipped, order, num_windows, l, rr, w, J, j, c);
        if (root >= 0) v[k] = v[k] - frame_value(plain, flipped, order, num_windows, l, rr, w, J, root, c);
    }
    if (e0 + 4 <= total) *reinterpret_cast<float4*>(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
    else for (int k = 0; e0 + k < total; ++k) out[e0 + k] = v[k];
}

// C1 MOTION BETWEEN KEYFRAMES (predict_tracks(interpolation="cubic")): the cubic Hermite segment from p1 (weight 0) to p2 (weight 1) with
// Catmull-Rom tangents over equally spaced keyframes -- half the difference of the two neighbours, or the segment's own difference
// where the outer keyframe p0 / p3 does not exist.  All in float64 on the float32 predictions, every operation rounded (no fused
// multiply-add), in the order of evaluation.interpolate_cubic_host, rounded once to float32: a numpy restatement gives the same bits.
__device__ __forceinline__ float hermite_mix(const float p0, const float p1, const float p2, const float p3, const bool has0, const bool has3,
                                             const double t)
{
#pragma clang fp contract(off)
    const double P1 = (double)p1, P2 = (double)p2;
    const double m1 = has0 ? (P2 - (double)p0) * 0.5 : P2 - P1;
    const double m2 = has3 ? ((double)p3 - P1) * 0.5 : P2 - P1;
    const double t2 = t * t;
    const double t3 = t2 * t;
    const double h01 = 3.0 * t2 - 2.0 * t3;
    const double h00 = 1.0 - h01;
    const double h11 = t3 - t2;
    const double h10 = (h11 - t2) + t;
    return (float)(((h00 * P1 + h01 * P2) + h10 * m1) + h11 * m2);
}

// Coordinate c of joint j of frame f by the plan of evaluation.keyframe_plan_cubic: the prediction of window l where l == r (frame_value's
// own bits; b and a are not looked at), else hermite_mix of the windows b, l, r, a -- b / a == -1: no such keyframe.  l or r outside
// [0, num_windows), or b / a outside [-1, num_windows) where they count, gives NaN; nothing is read then.
__device__ __forceinline__ float frame_value_cubic(const float* __restrict__ plain, const float* __restrict__ flipped, const int32_t* __restrict__ order,
                                                   const long num_windows, const long b, const long l, const long r, const long a, const double w,
                                                   const int J, const int j, const int c)
{
    if (l < 0 || l >= num_windows || r < 0 || r >= num_windows) return __builtin_nanf("");
    const float p1 = window_prediction(plain, flipped, order, l, J, j, c);
    if (l == r) return p1;
    if (b < -1 || b >= num_windows || a < -1 || a >= num_windows) return __builtin_nanf("");
    const float p2 = window_prediction(plain, flipped, order, r, J, j, c);
    const float p0 = (b >= 0) ? window_prediction(plain, flipped, order, b, J, j, c) : p1;
    const float p3 = (a >= 0) ? window_prediction(plain, flipped, order, a, J, j, c) : p2;
    return hermite_mix(p0, p1, p2, p3, b >= 0, a >= 0, w);
}

// assemble_tracks_kernel with the cubic rule: out (frames, J, 3), flattened, one thread per four consecutive floats; before / left /
// right / after (frames) i32, weight (frames) f64.  root >= 0: the frame's root joint -- its own interpolated float32 value -- is subtracted
// in float32 (that joint comes out exactly 0).
static __global__ void __launch_bounds__(256)
assemble_tracks_cubic_kernel(const float* __restrict__ plain, const float* __restrict__ flipped, const long num_windows,
                             const int32_t* __restrict__ order, const int32_t* __restrict__ before, const int32_t* __restrict__ left,
                             const int32_t* __restrict__ right, const int32_t* __restrict__ after, const double* __restrict__ weight,
                             const long frames, const int J, const int root, float* __restrict__ out)
{
    const long per = (long)J * 3, total = frames * per;
    const long e0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (e0 >= total) return;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long e = (e0 + k < total) ? e0 + k : e0;
        const long f = e / per;
        const int r = (int)(e - f * per), j = r / 3, c = r - j * 3;
        const long b = before[f], l = left[f], rr = right[f], a = after[f];
        const double w = weight[f];
        v[k] = frame_value_cubic(plain, flipped, order, num_windows, b, l, rr, a, w, J, j, c);
        if (root >= 0) v[k] = v[k] - frame_value_cubic(plain, flipped, order, num_windows, b, l, rr, a, w, J, root, c);
    }
    if (e0 + 4 <= total) *reinterpret_cast<float4*>(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
    else for (int k = 0; e0 + k < total; ++k) out[e0 + k] = v[k];
}

}  // namespace uu3d
