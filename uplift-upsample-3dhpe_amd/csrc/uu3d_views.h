// uu3d_views.h -- SEVERAL VIEWS (include/uu3d.h; predict.fuse_views, predict.solve_view_roots, predict.predict_views): V calibrated cameras
// see the same person at the same frames.  Every view's root-relative pose is in world axes already (uu3d_camera_to_world); this file
// joins them to one pose per frame and solves ONE world root from all views' 2D keypoints at once.
//     fuse_views_kernel        per (frame, joint), one lane: the mean over the views that SEE the frame, in float64, one 12-byte store
//     solve_view_roots_kernel  per frame, one lane: the 3x3 normal equations of all seeing views' used joints, solved by cofactors
// View v SEES frame f iff at least min_joints joints are used there; a joint is used iff its flag is set (no flags: every joint) and both
// raw 2D coordinates are finite (solve_root's test in uu3d_root.h).  The buffers are view-major: poses (V, R, J, 3), kp (V, R, J, 2),
// flags (V, R, J).  Every output element has one writer and is a function of inputs that nobody writes: bitwise repeatable.  No LDS, no
// atomics.  The statements are those of predict.fuse_views_host / predict.solve_view_roots_host, one for one.
#pragma once
#include "uu3d_root.h"
#include "uu3d_world.h"

namespace uu3d {

static constexpr int kViewsMax = 8;                                      // V beyond it: UU3D_ERR_UNSUPPORTED
static constexpr double kViewRank = 0x1p-40;                             // det must exceed this share of Hadamard's bound A00 A11 A22
static constexpr int kViewCamera = 16;                                   // doubles per view: fx, fy, cx, cy, then r1, r2, r3 (the camera's axes in world coordinates), then t

// Whether joint `at` (an index into the (V, R, J) planes) is used.
__device__ __forceinline__ bool view_joint_used(const float* __restrict__ kp, const uint8_t* __restrict__ flags, const long at)
{
    if (flags != nullptr && flags[at] == 0) return false;
    return finite_pair(*reinterpret_cast<const float2*>(kp + 2 * at));
}

// Where joint 0 of view v's frame lies in the (.., J) planes -- the offline buffers: `first` = the index of the frame's joint 0 in view 0,
// `step` = R * J.  The live stage has a functor of its own (uu3d_stream_views.h: every view's frame at its own place of a ring).
struct ViewBlocks {
    long first, step;
    __device__ __forceinline__ long operator()(const int v) const { return first + v * step; }
};

// The views among `allowed` (a bit per view) that see their frame, as a bit per view; at(v) = the index of that frame's joint 0.
template <class At>
__device__ __forceinline__ unsigned seeing_views_at(const float* __restrict__ kp, const uint8_t* __restrict__ flags, const At at, const unsigned allowed,
                                                    const int views, const int J, const int min_joints)
{
    unsigned mask = 0;
    for (int v = 0; v < views; ++v) {
        if (((allowed >> v) & 1u) == 0) continue;
        const long first = at(v);
        int n = 0;
        for (int j = 0; j < J; ++j) n += view_joint_used(kp, flags, first + j) ? 1 : 0;
        if (n >= min_joints) mask |= 1u << v;
    }
    return mask;
}

// The views that see a frame, as a bit per view; `first` = the index of the frame's joint 0 in view 0, `step` = R * J.
__device__ __forceinline__ unsigned seeing_views(const float* __restrict__ kp, const uint8_t* __restrict__ flags, const long first, const long step,
                                                 const int views, const int J, const int min_joints)
{
    return seeing_views_at(kp, flags, ViewBlocks{first, step}, (1u << views) - 1u, views, J, min_joints);
}

// Lane p = frame * J + joint.  fused[frame][joint] = (float)(s / (double)n), s the float64 sum of the seeing views' poses in ascending view
// order, n their number; no view sees the frame: the same mean over ALL views, view_count 0.  The lane of joint 0 also writes
// view_count[frame] and sees[v][frame].
static __global__ void __launch_bounds__(256)
fuse_views_kernel(const float* __restrict__ poses, const float* __restrict__ kp, const uint8_t* __restrict__ flags, const int views, const long rows,
                  const int J, const int min_joints, float* __restrict__ fused, uint8_t* __restrict__ view_count, uint8_t* __restrict__ sees)
{
#pragma clang fp contract(off)
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= rows * J) return;
    const long f = p / J;
    const int j = (int)(p - f * J);
    const long step = rows * J;
    const unsigned mask = seeing_views(kp, flags, f * J, step, views, J, min_joints);
    const int seen = __popc(mask);
    const unsigned take = seen > 0 ? mask : (1u << views) - 1u;
    const int n = seen > 0 ? seen : views;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int v = 0; v < views; ++v) {
        if (((take >> v) & 1u) == 0) continue;
        const WorldTrio t = *reinterpret_cast<const WorldTrio*>(poses + (v * step + p) * 3);
        s0 = s0 + (double)t.a;
        s1 = s1 + (double)t.b;
        s2 = s2 + (double)t.c;
    }
    const double nd = (double)n;
    WorldTrio r;
    r.a = (float)(s0 / nd);
    r.b = (float)(s1 / nd);
    r.c = (float)(s2 / nd);
    *reinterpret_cast<WorldTrio*>(fused + p * 3) = r;
    if (j == 0) {
        view_count[f] = (uint8_t)seen;
        for (int v = 0; v < views; ++v) sees[v * rows + f] = (uint8_t)((mask >> v) & 1u);
    }
}

// The solve of one frame: the statements of predict.solve_view_roots_host, one for one, every operation rounded once.  pose (J, 3) f32: the
// fused world pose of the frame; `mask`: the seeing views, at(v) = the index of joint 0 of view v's frame (seeing_views_at); cams
// (views, 16) f64.  -> solved; T = the world root, zeros when not.
template <class At>
__device__ __forceinline__ bool solve_view_root_at(const float* __restrict__ pose, const float* __restrict__ kp, const uint8_t* __restrict__ flags,
                                                   const At at, const unsigned mask, const int views, const int J,
                                                   const double* __restrict__ cams, double T[3])
{
#pragma clang fp contract(off)
    T[0] = T[1] = T[2] = 0.0;
    if (mask == 0) return false;
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    for (int v = 0; v < views; ++v) {
        if (((mask >> v) & 1u) == 0) continue;
        const double* __restrict__ c = cams + kViewCamera * v;
        const double fx = c[0], fy = c[1], cx = c[2], cy = c[3];
        if (!finite_double(fx) || !finite_double(fy) || !finite_double(cx) || !finite_double(cy) || !(fx > 0.0) || !(fy > 0.0)) return false;
        const long first = at(v);
        for (int j = 0; j < J; ++j) {
            const long q = first + j;
            if (!view_joint_used(kp, flags, q)) continue;
            const float2 uv = *reinterpret_cast<const float2*>(kp + 2 * q);
            const double a = ((double)uv.x - cx) / fx;
            const double b = ((double)uv.y - cy) / fy;
            const double n0 = c[4] - a * c[10], n1 = c[5] - a * c[11], n2 = c[6] - a * c[12];
            const double m0 = c[7] - b * c[10], m1 = c[8] - b * c[11], m2 = c[9] - b * c[12];
            const double d0 = c[13] - (double)pose[3 * j], d1 = c[14] - (double)pose[3 * j + 1], d2 = c[15] - (double)pose[3 * j + 2];
            const double e = (n0 * d0 + n1 * d1) + n2 * d2;
            const double g = (m0 * d0 + m1 * d1) + m2 * d2;
            a00 = a00 + (n0 * n0 + m0 * m0);
            a01 = a01 + (n0 * n1 + m0 * m1);
            a02 = a02 + (n0 * n2 + m0 * m2);
            a11 = a11 + (n1 * n1 + m1 * m1);
            a12 = a12 + (n1 * n2 + m1 * m2);
            a22 = a22 + (n2 * n2 + m2 * m2);
            b0 = b0 + (n0 * e + m0 * g);
            b1 = b1 + (n1 * e + m1 * g);
            b2 = b2 + (n2 * e + m2 * g);
        }
    }
    const double c00 = a11 * a22 - a12 * a12;
    const double c01 = a02 * a12 - a01 * a22;
    const double c02 = a01 * a12 - a02 * a11;
    const double c11 = a00 * a22 - a02 * a02;
    const double c12 = a01 * a02 - a00 * a12;
    const double c22 = a00 * a11 - a01 * a01;
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    if (!finite_double(det) || !(det > 0.0)) return false;
    if (!(det > kViewRank * ((a00 * a11) * a22))) return false;         // the rank guard: a rank-deficient system's det is rounding noise
    const double x0 = (c00 * b0 + c01 * b1) + c02 * b2;
    const double x1 = (c01 * b0 + c11 * b1) + c12 * b2;
    const double x2 = (c02 * b0 + c12 * b1) + c22 * b2;
    const double T0 = x0 / det, T1 = x1 / det, T2 = x2 / det;
    if (!finite_double(T0) || !finite_double(T1) || !finite_double(T2)) return false;
    for (int v = 0; v < views; ++v) {                                    // every used joint of every seeing view in front of its camera
        if (((mask >> v) & 1u) == 0) continue;
        const double* __restrict__ c = cams + kViewCamera * v;
        const long first = at(v);
        for (int j = 0; j < J; ++j) {
            if (!view_joint_used(kp, flags, first + j)) continue;
            const double w0 = (T0 + (double)pose[3 * j]) - c[13];
            const double w1 = (T1 + (double)pose[3 * j + 1]) - c[14];
            const double w2 = (T2 + (double)pose[3 * j + 2]) - c[15];
            const double z = (c[10] * w0 + c[11] * w1) + c[12] * w2;
            if (!(z > 0.0)) return false;
        }
    }
    T[0] = T0; T[1] = T1; T[2] = T2;
    return true;
}

// The solve of one frame of the offline buffers; `first` / `step` as in seeing_views.
__device__ __forceinline__ bool solve_view_root(const float* __restrict__ pose, const float* __restrict__ kp, const uint8_t* __restrict__ flags,
                                                const long first, const long step, const int views, const int J,
                                                const double* __restrict__ cams, const int min_joints, double T[3])
{
    const ViewBlocks at{first, step};
    const unsigned mask = seeing_views_at(kp, flags, at, (1u << views) - 1u, views, J, min_joints);
    return solve_view_root_at(pose, kp, flags, at, mask, views, J, cams, T);
}

// roots (rows, 3) f64 and solved (rows) u8: one lane per frame, the shape of solve_roots_kernel.
static __global__ void __launch_bounds__(256)
solve_view_roots_kernel(const float* __restrict__ fused, const float* __restrict__ kp, const uint8_t* __restrict__ flags, const int views,
                        const long rows, const int J, const double* __restrict__ cams, const int min_joints, double* __restrict__ roots,
                        uint8_t* __restrict__ solved)
{
    const long f = (long)blockIdx.x * 256 + threadIdx.x;
    if (f >= rows) return;
    double T[3] = {0.0, 0.0, 0.0};
    const bool ok = solve_view_root(fused + f * J * 3, kp, flags, f * J, rows * J, views, J, cams, min_joints, T);
    roots[f * 3] = T[0];
    roots[f * 3 + 1] = T[1];
    roots[f * 3 + 2] = T[2];
    solved[f] = ok ? 1 : 0;
}

}  // namespace uu3d
