// uu3d_undistort.h -- LENS DISTORTION (include/uu3d.h; predict.undistort_points, predict.predict_tracks(camera=Camera(distortion=...)),
// stream.StreamSession(camera=Camera(distortion=...))): the pixel a detector saw through a lens with radial and tangential distortion ->
// the pixel an ideal pinhole with the same intrinsics would have seen, on the device, in front of everything else that looks at a track
// (uu3d_map_keypoints included: an affine joint map does not commute with distortion).  One launch, one lane per point, one 8-byte load and
// one 8-byte store; no LDS, no atomics; every element has one writer and is a function of inputs that nobody writes: bitwise repeatable.
#pragma once
#include "uu3d_root.h"

namespace uu3d {

static constexpr int kUndistortIterations = 20;                         // Camera.ITERATIONS: a constant of the rule, no early exit
static constexpr int kUndistortCamera = 10;                             // doubles per camera: fx, fy, cx, cy, k1, k2, p1, p2, k3, tol

// One point, every operation rounded once in float64 (no fused multiply-add), one final rounding to float32: the statements of
// predict.undistort_points_host, one for one.  cam = (fx, fy, cx, cy, k1, k2, p1, p2, k3, tol); OpenCV's Brown-Conrady order.
// A point that is not ACCEPTED -- a non-finite input, a camera that is not usable, or a re-distortion residual above tol pixels (an
// observation outside the region where the model can be inverted) -- is (NaN, NaN).
__device__ __forceinline__ float2 undistort_point(const float2 uv, const double* __restrict__ cam)
{
#pragma clang fp contract(off)
    const float nan = __uint_as_float(0x7fc00000u);
    const float2 lost = make_float2(nan, nan);
    const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3];
    const double k1 = cam[4], k2 = cam[5], p1 = cam[6], p2 = cam[7], k3 = cam[8], tol = cam[9];
    if (!finite_double(fx) || !finite_double(fy) || !finite_double(cx) || !finite_double(cy) || !(fx > 0.0) || !(fy > 0.0)) return lost;
    if (!finite_pair(uv)) return lost;
    const double x0 = ((double)uv.x - cx) / fx;
    const double y0 = ((double)uv.y - cy) / fy;
    double x = x0, y = y0;
    for (int i = 0; i < kUndistortIterations; ++i) {
        const double r2 = x * x + y * y;
        const double ic = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2);
        const double dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
        const double dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
        x = (x0 - dx) * ic;
        y = (y0 - dy) * ic;
    }
    // the acceptance check: the forward model on (x, y) must land on the observation
    const double r2 = x * x + y * y;
    const double rad = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
    const double dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
    const double dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
    const double xd = x * rad + dx;
    const double yd = y * rad + dy;
    const double ex = fabs(xd - x0) * fx;
    const double ey = fabs(yd - y0) * fy;
    if (!finite_double(x) || !finite_double(y) || !(ex <= tol) || !(ey <= tol)) return lost;
    const float2 r = make_float2((float)(fx * x + cx), (float)(fy * y + cy));
    return finite_pair(r) ? r : lost;
}

// out (rows, points, 2): lane p = row * points + point takes the camera of its row's track.  row_track (rows) i32 or nullptr (every row
// takes camera 0); cameras (num_tracks, 10) f64.  A track id out of range: (NaN, NaN), nothing read out of bounds (solve_roots_kernel's
// conventions).
static __global__ void __launch_bounds__(256)
undistort_points_kernel(const float* __restrict__ in, float* __restrict__ out, const long rows, const int points, const int32_t* __restrict__ row_track,
                        const int num_tracks, const double* __restrict__ cameras)
{
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= rows * points) return;
    const int t = row_track != nullptr ? row_track[p / points] : 0;
    const float nan = __uint_as_float(0x7fc00000u);
    float2 r = make_float2(nan, nan);
    if (t >= 0 && t < num_tracks)
        r = undistort_point(*reinterpret_cast<const float2*>(in + p * 2), cameras + kUndistortCamera * (long)t);
    *reinterpret_cast<float2*>(out + p * 2) = r;
}

}  // namespace uu3d
