// uu3d_world.h -- WORLD SPACE (include/uu3d.h; predict.camera_to_world, predict.predict_tracks(camera=Camera(..., orientation=, translation=)),
// stream.StreamSession(camera=Camera(..., orientation=...))): root-relative poses and roots in the camera's own space -> the same scene in
// world axes, X_world = qrot(q, X_cam) + t, the convention of h36m.camera_to_world.  Poses are rotated only (they stay root-relative), a
// solved or held root is rotated and translated, a root without a state stays zeros.  One launch, one lane per (row, point) -- the points of
// a row are its J joints and, as point J, its root --, one 12-byte load and one 12-byte store; no LDS, no atomics; every element has one
// writer, and a lane reads its own element before it writes it, so the outputs may be the inputs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace uu3d {

static constexpr int kWorldExtrinsics = 7;                              // doubles per camera: the unit quaternion (w, x, y, z), then t

struct WorldTrio { float a, b, c; };                                    // 12 bytes, 4-byte aligned: what a lane loads and stores

// One point, every operation rounded once in float64 (no fused multiply-add), one final rounding to float32: the statements of
// predict.camera_to_world_host, one for one.  ext = (w, x, y, z, tx, ty, tz); `place`: add t (a root), else rotate only (a joint).
__device__ __forceinline__ WorldTrio world_point(const WorldTrio v, const double* __restrict__ ext, const bool place)
{
#pragma clang fp contract(off)
    const double w = ext[0], x = ext[1], y = ext[2], z = ext[3];
    const double a = (double)v.a, b = (double)v.b, c = (double)v.c;
    const double uv0 = y * c - z * b;
    const double uv1 = z * a - x * c;
    const double uv2 = x * b - y * a;
    const double uuv0 = y * uv2 - z * uv1;
    const double uuv1 = z * uv0 - x * uv2;
    const double uuv2 = x * uv1 - y * uv0;
    double r0 = a + 2.0 * (w * uv0 + uuv0);
    double r1 = b + 2.0 * (w * uv1 + uuv1);
    double r2 = c + 2.0 * (w * uv2 + uuv2);
    if (place) {
        r0 = r0 + ext[4];
        r1 = r1 + ext[5];
        r2 = r2 + ext[6];
    }
    WorldTrio r;
    r.a = (float)r0;
    r.b = (float)r1;
    r.c = (float)r2;
    return r;
}

// Lane p = row * (joints + 1) + point.  point < joints: poses[row][point] -> poses_out (nothing when poses is null); point == joints:
// roots[row] -> roots_out, zeros when root_state[row] == 0 (nothing when roots is null).  row_track (rows) i32 or nullptr (every row takes
// camera 0); extrinsics (num_tracks, 7) f64.  A track id out of range: NaN, nothing read out of bounds (undistort_points_kernel's
// convention).  The output pointers may equal the input pointers, so none of the four is __restrict__.
static __global__ void __launch_bounds__(256)
camera_to_world_kernel(const float* poses, float* poses_out, const float* roots, const uint8_t* __restrict__ root_state, float* roots_out,
                       const long rows, const int joints, const int32_t* __restrict__ row_track, const int num_tracks,
                       const double* __restrict__ extrinsics)
{
    const long per = (long)joints + 1;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= rows * per) return;
    const long row = p / per;
    const int point = (int)(p - row * per);
    const bool root = point == joints;
    if (root ? roots == nullptr : poses == nullptr) return;
    const float* in = root ? roots + row * 3 : poses + (row * joints + point) * 3;
    float* out = root ? roots_out + row * 3 : poses_out + (row * joints + point) * 3;
    const int t = row_track != nullptr ? row_track[row] : 0;
    const float nan = __uint_as_float(0x7fc00000u);
    WorldTrio r;
    r.a = r.b = r.c = nan;
    if (t >= 0 && t < num_tracks) {
        if (root && root_state[row] == 0)
            r.a = r.b = r.c = 0.0f;
        else
            r = world_point(*reinterpret_cast<const WorldTrio*>(in), extrinsics + kWorldExtrinsics * (long)t, root);
    }
    *reinterpret_cast<WorldTrio*>(out) = r;
}

}  // namespace uu3d
