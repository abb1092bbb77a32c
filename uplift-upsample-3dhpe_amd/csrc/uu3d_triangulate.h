// uu3d_triangulate.h -- WHERE RAYS MEET (include/uu3d.h; predict.triangulate_joints, predict.place_joints, predict.predict_views(triangulate=...)):
// the fused pose of SEVERAL VIEWS is still a mean of monocular lifts, so the scale and depth errors all views share stay in it.  Where two or
// more calibrated cameras see the same joint, its world position is fixed by geometry alone; this file places such joints there and leaves
// every other joint to the fused lift.
//     triangulate_joints_kernel  per (frame, joint), one lane: two weighted 3x3 solves per round over the candidate views, the view of the
//                                largest reprojection residual dropped between rounds; X (rows, J, 3) f64 and count (rows, J) u8
//     place_joints_kernel        per (frame, joint), one lane: (float)(X_j - X_root) where both are triangulated, the fused bits elsewhere;
//                                one 12-byte store and one byte
// The buffers are view-major as in uu3d_views.h: kp (V, R, J, 2), flags (V, R, J), sees (V, R) -- the output of uu3d_fuse_views, read
// instead of recounted.  The candidate views of a joint are walked through a bitmask: nothing per lane is indexed by a run-time view number,
// so nothing goes to scratch memory; a view's depth weight is recomputed from the first pass' X by the statements that produced it.  Every
// output element has one writer and is a function of inputs that nobody writes: bitwise repeatable.  No LDS, no atomics.  The statements are
// those of predict.triangulate_joints_host / predict.place_joints_host, one for one.
#pragma once
#include "uu3d_views.h"
#include "uu3d_view_match.h"

namespace uu3d {

static constexpr int kTriangulateMinViews = 2;                           // two lines meet in a point; one does not

// One weighted solve over the views of `cand`: the normal equations of n . (X - t) = 0 and m . (X - t) = 0, every row scaled by q_v = 1.0
// (from == nullptr) or q_v = 1.0 / z_v, z_v the depth of `from` in view v.  `at` = the index of this lane's joint in view 0, `step` = R * J.
// -> accepted (det finite, > 0 and above the share kViewParallel of Hadamard's bound, X finite); X is written either way.
__device__ __forceinline__ bool triangulate_pass(const float* __restrict__ kp, const long at, const long step, const int views, const unsigned cand,
                                                 const double* __restrict__ cams, const double* from, double X[3])
{
#pragma clang fp contract(off)
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    for (int v = 0; v < views; ++v) {
        if (((cand >> v) & 1u) == 0) continue;
        const double* __restrict__ c = cams + kViewCamera * v;
        double q = 1.0;
        if (from != nullptr) {
            const double w0 = from[0] - c[13], w1 = from[1] - c[14], w2 = from[2] - c[15];
            const double z = (c[10] * w0 + c[11] * w1) + c[12] * w2;
            q = 1.0 / z;
        }
        const float2 uv = *reinterpret_cast<const float2*>(kp + 2 * (at + v * step));
        const double a = ((double)uv.x - c[2]) / c[0];
        const double b = ((double)uv.y - c[3]) / c[1];
        const double n0 = (c[4] - a * c[10]) * q, n1 = (c[5] - a * c[11]) * q, n2 = (c[6] - a * c[12]) * q;
        const double m0 = (c[7] - b * c[10]) * q, m1 = (c[8] - b * c[11]) * q, m2 = (c[9] - b * c[12]) * q;
        const double e = (n0 * c[13] + n1 * c[14]) + n2 * c[15];
        const double g = (m0 * c[13] + m1 * c[14]) + m2 * c[15];
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
    const double c00 = a11 * a22 - a12 * a12;
    const double c01 = a02 * a12 - a01 * a22;
    const double c02 = a01 * a12 - a02 * a11;
    const double c11 = a00 * a22 - a02 * a02;
    const double c12 = a01 * a02 - a00 * a12;
    const double c22 = a00 * a11 - a01 * a01;
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    const double x0 = (c00 * b0 + c01 * b1) + c02 * b2;
    const double x1 = (c01 * b0 + c11 * b1) + c12 * b2;
    const double x2 = (c02 * b0 + c12 * b1) + c22 * b2;
    X[0] = x0 / det;
    X[1] = x1 / det;
    X[2] = x2 / det;
    if (!finite_double(det) || !(det > 0.0)) return false;
    if (!(det > kViewParallel * ((a00 * a11) * a22))) return false;      // the rank guard: rays closer than 1e-3 rad carry no distance
    return finite_double(X[0]) && finite_double(X[1]) && finite_double(X[2]);
}

// Whether X lies in front of every camera of `cand`: z_v = (r3_0 w0 + r3_1 w1) + r3_2 w2 > 0 with w = X - t.
__device__ __forceinline__ bool triangulate_in_front(const int views, const unsigned cand, const double* __restrict__ cams, const double X[3])
{
#pragma clang fp contract(off)
    bool ok = true;
    for (int v = 0; v < views; ++v) {
        if (((cand >> v) & 1u) == 0) continue;
        const double* __restrict__ c = cams + kViewCamera * v;
        const double w0 = X[0] - c[13], w1 = X[1] - c[14], w2 = X[2] - c[15];
        const double z = (c[10] * w0 + c[11] * w1) + c[12] * w2;
        ok = ok && (z > 0.0);
    }
    return ok;
}

// Lane p = frame * J + joint.  X[p] and count[p]: the rule of WHERE RAYS MEET; a joint that is not triangulated gets zeros and 0.
static __global__ void __launch_bounds__(256)
triangulate_joints_kernel(const float* __restrict__ kp, const uint8_t* __restrict__ flags, const uint8_t* __restrict__ sees, const int views,
                          const long rows, const int J, const double* __restrict__ cams, const int min_views, const double max_residual,
                          double* __restrict__ X, uint8_t* __restrict__ count)
{
#pragma clang fp contract(off)
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= rows * J) return;
    const long f = p / J;
    const long step = rows * J;
    unsigned cand = 0;
    for (int v = 0; v < views; ++v)
        if (sees[v * rows + f] != 0 && view_joint_used(kp, flags, p + v * step)) cand |= 1u << v;
    double out[3] = {0.0, 0.0, 0.0};
    int n = 0;
    while (__popc(cand) >= min_views) {
        double X1[3], X2[3];
        if (!triangulate_pass(kp, p, step, views, cand, cams, nullptr, X1) || !triangulate_in_front(views, cand, cams, X1)) break;
        if (!triangulate_pass(kp, p, step, views, cand, cams, X1, X2) || !triangulate_in_front(views, cand, cams, X2)) break;
        double worst = -1.0;                                             // the residuals are >= 0: the first candidate always takes it
        int drop = 0;
        for (int v = 0; v < views; ++v) {
            if (((cand >> v) & 1u) == 0) continue;
            const double* __restrict__ c = cams + kViewCamera * v;
            const float2 uv = *reinterpret_cast<const float2*>(kp + 2 * (p + v * step));
            const double w0 = X2[0] - c[13], w1 = X2[1] - c[14], w2 = X2[2] - c[15];
            const double z = (c[10] * w0 + c[11] * w1) + c[12] * w2;
            const double xc = (c[4] * w0 + c[5] * w1) + c[6] * w2;
            const double yc = (c[7] * w0 + c[8] * w1) + c[9] * w2;
            const double du = fabs((c[0] * (xc / z) + c[2]) - (double)uv.x);
            const double dv = fabs((c[1] * (yc / z) + c[3]) - (double)uv.y);
            double rho = du > dv ? du : dv;
            if (du != du || dv != dv) rho = __builtin_huge_val();        // a NaN rejects the view
            if (rho >= worst) { worst = rho; drop = v; }                 // ties: the larger view index
        }
        if (worst <= max_residual) {
            out[0] = X2[0]; out[1] = X2[1]; out[2] = X2[2];
            n = __popc(cand);
            break;
        }
        cand &= ~(1u << drop);
    }
    X[p * 3] = out[0];
    X[p * 3 + 1] = out[1];
    X[p * 3 + 2] = out[2];
    count[p] = (uint8_t)n;
}

// Lane p = frame * J + joint.  Both the joint and the frame's root joint triangulated: (float)(X_j - X_root) per channel, +0.0 for the root
// joint itself, joint_views = count; otherwise the fused pose's bits and 0.
static __global__ void __launch_bounds__(256)
place_joints_kernel(const float* __restrict__ fused, const double* __restrict__ X, const uint8_t* __restrict__ count, const long rows, const int J,
                    const int root, float* __restrict__ placed, uint8_t* __restrict__ joint_views)
{
#pragma clang fp contract(off)
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= rows * J) return;
    const long f = p / J;
    const int j = (int)(p - f * J);
    const long r = f * J + root;
    const uint8_t here = count[p];
    WorldTrio t = *reinterpret_cast<const WorldTrio*>(fused + p * 3);
    const bool take = here > 0 && count[r] > 0;
    if (take) {
        t.a = j == root ? 0.0f : (float)(X[p * 3] - X[r * 3]);
        t.b = j == root ? 0.0f : (float)(X[p * 3 + 1] - X[r * 3 + 1]);
        t.c = j == root ? 0.0f : (float)(X[p * 3 + 2] - X[r * 3 + 2]);
    }
    *reinterpret_cast<WorldTrio*>(placed + p * 3) = t;
    joint_views[p] = take ? here : (uint8_t)0;
}

}  // namespace uu3d
