// uu3d_view_calibrate.h -- WHERE THE CAMERAS STAND (include/uu3d.h; predict.view_moment_sums, predict.view_position_sums,
// predict.solve_view_pose, predict.calibrate_views, predict.predict_views(calibrate=...)): SEVERAL VIEWS needs every camera's extrinsics, and
// nobody who puts two phones on tripods has them.  Every view's lift is the same skeleton in that camera's own axes, so the rotation between
// two cameras is the rotation between their lifts; the rays of both cameras and the lifts' metric size then fix where the second camera
// stands.  This file finds the pose of views 1 .. V - 1 in the space of view 0.
//     view_moment_sums_kernel    per (chunk of 4096 rows, view), one workgroup of 256 lanes: M_v = sum of p_v (x) p_0 over the rows both views
//                                see, 9 sums and the number of rows
//     view_position_sums_kernel  the same grid, behind the rotation: per row the two cameras' 3x3 normal equations with the row's unknown
//                                root eliminated, S (6 sums), g (3 sums) and the number of rows
//     solve_view_pose_kernel     one wave, a view per lane; stage 0: Horn's 4x4 matrix from M_v, cyclic Jacobi with a fixed number of sweeps,
//                                the quaternion; stage 1: S c = g by cofactors, the position.  Two launches of the one kernel.
// Both sum kernels share calibrate_chunk_sums: lane l walks the rows l, l + 256, ... of its chunk, then a fixed tree through LDS, one value
// after the other; the solve adds the chunks in ascending order.  The buffers are view-major as in uu3d_views.h: poses (V, R, J, 3) -- the
// lifts in each camera's own axes, root-relative --, kp (V, R, J, 2), flags (V, R, J).  Float64 on the float32 inputs, every operation rounded
// once (contraction off), sqrt and division correctly rounded.  Every output element has one writer, no atomics, the inputs are only read,
// nothing per lane is indexed by a run-time view number: bitwise repeatable.  The statements are those of predict.view_moment_sums_host /
// predict.view_position_sums_host / predict.solve_view_pose_host, one for one.  lift_moment_products (a term's nine moment products) and
// horn_jacobi (Horn's matrix through the Jacobi sweeps) are shared with uu3d_lift_match.h, which matches tracks by the same lifts.
#pragma once
#include "uu3d_views.h"

namespace uu3d {

static constexpr int kCalibrateChunk = 4096;                             // rows per workgroup; part of the rule's order of summation
static constexpr int kCalibrateLanes = 256;                              // lane l sums the rows l, l + 256, ... of its chunk
static constexpr int kCalibrateSums = 10;                                // doubles per (view, chunk): 9 sums and the number of rows
static constexpr int kCalibrateSweeps = 10;                              // cyclic Jacobi sweeps of the 4x4, no early exit
static constexpr int kCalibratePose = 8;                                 // doubles per view: the quaternion (w, x, y, z), the position, the state
static constexpr double kCalibrateGap = 0x1p-20;                         // the two largest eigenvalues must differ by this share of the largest

// Whether a view sees the row whose joint 0 is `first` in the (V, R, J) planes: at least min_joints used joints.
__device__ __forceinline__ bool view_sees_row(const float* __restrict__ kp, const uint8_t* __restrict__ flags, const long first, const int J,
                                              const int min_joints)
{
    int n = 0;
    for (int j = 0; j < J; ++j) n += view_joint_used(kp, flags, first + j) ? 1 : 0;
    return n >= min_joints;
}

// The chunked reduction both sum kernels share.  Block (c, v): lane l walks the rows c * 4096 + l, + 256, ... below min(rows, (c + 1) * 4096)
// in ascending order; term(row, s) -> whether the row is a term, and its ten values; x_i = x_i + s_i from 0.0.  Then, one value after the
// other, the fixed tree of uu3d_view_pair_sums through LDS; lane 0 writes out[0 .. 9].
template <typename Term>
__device__ __forceinline__ void calibrate_chunk_sums(const long rows, const Term& term, double* __restrict__ lds, double* __restrict__ out)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    const long begin = (long)blockIdx.x * kCalibrateChunk;
    const long end = begin + kCalibrateChunk < rows ? begin + kCalibrateChunk : rows;
    double x[kCalibrateSums];
#pragma unroll
    for (int i = 0; i < kCalibrateSums; ++i) x[i] = 0.0;
    for (long r = begin + lane; r < end; r += kCalibrateLanes) {
        double s[kCalibrateSums];
        if (term(r, s)) {
#pragma unroll
            for (int i = 0; i < kCalibrateSums; ++i) x[i] = x[i] + s[i];
        }
    }
#pragma unroll
    for (int i = 0; i < kCalibrateSums; ++i) {
        lds[lane] = x[i];
        __syncthreads();
        for (int stride = kCalibrateLanes / 2; stride >= 1; stride >>= 1) {      // the fixed tree
            if (lane < stride) lds[lane] = lds[lane] + lds[lane + stride];
            __syncthreads();
        }
        if (lane == 0) out[i] = lds[0];
        __syncthreads();
    }
}

// Ten zeros for a (view, chunk) that holds no sums: view 0, a view the rotation refused.
__device__ __forceinline__ void calibrate_chunk_zeros(double* __restrict__ out)
{
    if (threadIdx.x < kCalibrateSums) out[threadIdx.x] = 0.0;
}

// The nine moment products of one term, shared with WHO IS WHO WITHOUT A WORLD (uu3d_lift_match.h) so that the bits cannot drift: a, b = the
// index of joint 0 of the two lifts in poses; s_ik = 0.0; s_ik = s_ik + p_a[j][i] * p_b[j][k] over ALL J joints ascending (an unobserved
// joint's lift is still read), ik = 00, 01, 02, 10, ..., 22.
__device__ __forceinline__ void lift_moment_products(const float* __restrict__ poses, const long a, const long b, const int J, double s[9])
{
#pragma clang fp contract(off)
    double m00 = 0.0, m01 = 0.0, m02 = 0.0, m10 = 0.0, m11 = 0.0, m12 = 0.0, m20 = 0.0, m21 = 0.0, m22 = 0.0;
    for (int j = 0; j < J; ++j) {
        const WorldTrio p = *reinterpret_cast<const WorldTrio*>(poses + (a + j) * 3);
        const WorldTrio q = *reinterpret_cast<const WorldTrio*>(poses + (b + j) * 3);
        const double p0 = (double)p.a, p1 = (double)p.b, p2 = (double)p.c;
        const double q0 = (double)q.a, q1 = (double)q.b, q2 = (double)q.c;
        m00 = m00 + p0 * q0; m01 = m01 + p0 * q1; m02 = m02 + p0 * q2;
        m10 = m10 + p1 * q0; m11 = m11 + p1 * q1; m12 = m12 + p1 * q2;
        m20 = m20 + p2 * q0; m21 = m21 + p2 * q1; m22 = m22 + p2 * q2;
    }
    s[0] = m00; s[1] = m01; s[2] = m02; s[3] = m10; s[4] = m11; s[5] = m12; s[6] = m20; s[7] = m21; s[8] = m22;
}

// A row of the rotation: the moment products of view v's lift and view 0's, s_9 = 1.
struct ViewMomentTerm {
    const float* __restrict__ poses;
    const float* __restrict__ kp;
    const uint8_t* __restrict__ flags;
    long rows;
    int J, v, min_joints;
    __device__ __forceinline__ bool operator()(const long r, double (&s)[kCalibrateSums]) const
    {
        const long a0 = r * J, av = ((long)v * rows + r) * J;
        if (!view_sees_row(kp, flags, a0, J, min_joints) || !view_sees_row(kp, flags, av, J, min_joints)) return false;
        lift_moment_products(poses, av, a0, J, s);
        s[9] = 1.0;
        return true;
    }
};

// The rotation of WORLD SPACE before its final rounding: the statements of world_point (uu3d_world.h), one for one.
__device__ __forceinline__ void calibrate_turn(const double w, const double x, const double y, const double z, const double a, const double b,
                                               const double c, double r[3])
{
#pragma clang fp contract(off)
    const double uv0 = y * c - z * b;
    const double uv1 = z * a - x * c;
    const double uv2 = x * b - y * a;
    const double uuv0 = y * uv2 - z * uv1;
    const double uuv1 = z * uv0 - x * uv2;
    const double uuv2 = x * uv1 - y * uv0;
    r[0] = a + 2.0 * (w * uv0 + uuv0);
    r[1] = b + 2.0 * (w * uv1 + uuv1);
    r[2] = c + 2.0 * (w * uv2 + uuv2);
}

// The camera of one view as the position sums read it: fx, fy, cx, cy, the quaternion and the axes r1, r2, r3 it gives.
struct CalibrateCamera { double fx, fy, cx, cy, w, x, y, z, ax[9]; };

// One view's normal equations of a row: over its used joints ascending, the root-solve rows of SEVERAL VIEWS with P_j the view's own lift --
// kTurn: rotated by the view's quaternion --: A_ik += (n_i n_k + m_i m_k), B_i += (n_i e + m_i g) with e = n . P_j, g = m . P_j.
template <bool kTurn>
__device__ __forceinline__ void calibrate_normal_sums(const float* __restrict__ poses, const float* __restrict__ kp, const uint8_t* __restrict__ flags,
                                                      const long first, const int J, const CalibrateCamera& c, double A[6], double B[3])
{
#pragma clang fp contract(off)
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    for (int j = 0; j < J; ++j) {
        if (!view_joint_used(kp, flags, first + j)) continue;
        const float2 uv = *reinterpret_cast<const float2*>(kp + 2 * (first + j));
        const WorldTrio p = *reinterpret_cast<const WorldTrio*>(poses + (first + j) * 3);
        const double a = ((double)uv.x - c.cx) / c.fx;
        const double b = ((double)uv.y - c.cy) / c.fy;
        const double n0 = c.ax[0] - a * c.ax[6], n1 = c.ax[1] - a * c.ax[7], n2 = c.ax[2] - a * c.ax[8];
        const double m0 = c.ax[3] - b * c.ax[6], m1 = c.ax[4] - b * c.ax[7], m2 = c.ax[5] - b * c.ax[8];
        double P[3] = {(double)p.a, (double)p.b, (double)p.c};
        if (kTurn) calibrate_turn(c.w, c.x, c.y, c.z, (double)p.a, (double)p.b, (double)p.c, P);
        const double e = (n0 * P[0] + n1 * P[1]) + n2 * P[2];
        const double g = (m0 * P[0] + m1 * P[1]) + m2 * P[2];
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
    A[0] = a00; A[1] = a01; A[2] = a02; A[3] = a11; A[4] = a12; A[5] = a22;
    B[0] = b0; B[1] = b1; B[2] = b2;
}

// A row of the position: both views' normal equations, the row's root eliminated.  s_0 .. s_5 = S_00, 01, 02, 11, 12, 22; s_6 .. s_8 = g;
// s_9 = 1.  A row whose A0 + Av fails the rank guard of uu3d_solve_view_roots is not a term.
struct ViewPositionTerm {
    const float* __restrict__ poses;
    const float* __restrict__ kp;
    const uint8_t* __restrict__ flags;
    long rows;
    int J, v, min_joints;
    CalibrateCamera c0, cv;
    __device__ __forceinline__ bool operator()(const long r, double (&s)[kCalibrateSums]) const
    {
#pragma clang fp contract(off)
        const long first0 = r * J, firstv = ((long)v * rows + r) * J;
        if (!view_sees_row(kp, flags, first0, J, min_joints) || !view_sees_row(kp, flags, firstv, J, min_joints)) return false;
        double A0[6], B0[3], Av[6], Bv[3];
        calibrate_normal_sums<false>(poses, kp, flags, first0, J, c0, A0, B0);
        calibrate_normal_sums<true>(poses, kp, flags, firstv, J, cv, Av, Bv);
        const double a00 = A0[0] + Av[0], a01 = A0[1] + Av[1], a02 = A0[2] + Av[2], a11 = A0[3] + Av[3], a12 = A0[4] + Av[4], a22 = A0[5] + Av[5];
        const double c00 = a11 * a22 - a12 * a12;
        const double c01 = a02 * a12 - a01 * a22;
        const double c02 = a01 * a12 - a02 * a11;
        const double c11 = a00 * a22 - a02 * a02;
        const double c12 = a01 * a02 - a00 * a12;
        const double c22 = a00 * a11 - a01 * a01;
        const double det = (a00 * c00 + a01 * c01) + a02 * c02;
        if (!finite_double(det) || !(det > 0.0)) return false;
        if (!(det > kViewRank * ((a00 * a11) * a22))) return false;
        const double k00 = c00 / det, k01 = c01 / det, k02 = c02 / det, k11 = c11 / det, k12 = c12 / det, k22 = c22 / det;
        // W = Av K, all nine elements (the product of two symmetric matrices is not symmetric)
        const double w00 = (Av[0] * k00 + Av[1] * k01) + Av[2] * k02;
        const double w01 = (Av[0] * k01 + Av[1] * k11) + Av[2] * k12;
        const double w02 = (Av[0] * k02 + Av[1] * k12) + Av[2] * k22;
        const double w10 = (Av[1] * k00 + Av[3] * k01) + Av[4] * k02;
        const double w11 = (Av[1] * k01 + Av[3] * k11) + Av[4] * k12;
        const double w12 = (Av[1] * k02 + Av[3] * k12) + Av[4] * k22;
        const double w20 = (Av[2] * k00 + Av[4] * k01) + Av[5] * k02;
        const double w21 = (Av[2] * k01 + Av[4] * k11) + Av[5] * k12;
        const double w22 = (Av[2] * k02 + Av[4] * k12) + Av[5] * k22;
        s[0] = Av[0] - ((w00 * Av[0] + w01 * Av[1]) + w02 * Av[2]);
        s[1] = Av[1] - ((w00 * Av[1] + w01 * Av[3]) + w02 * Av[4]);
        s[2] = Av[2] - ((w00 * Av[2] + w01 * Av[4]) + w02 * Av[5]);
        s[3] = Av[3] - ((w10 * Av[1] + w11 * Av[3]) + w12 * Av[4]);
        s[4] = Av[4] - ((w10 * Av[2] + w11 * Av[4]) + w12 * Av[5]);
        s[5] = Av[5] - ((w20 * Av[2] + w21 * Av[4]) + w22 * Av[5]);
        const double h0 = B0[0] + Bv[0], h1 = B0[1] + Bv[1], h2 = B0[2] + Bv[2];
        s[6] = Bv[0] - ((w00 * h0 + w01 * h1) + w02 * h2);
        s[7] = Bv[1] - ((w10 * h0 + w11 * h1) + w12 * h2);
        s[8] = Bv[2] - ((w20 * h0 + w21 * h1) + w22 * h2);
        s[9] = 1.0;
        return true;
    }
};

// Block (c, v).  partial (V, C, 10) f64; view 0's blocks hold zeros.
static __global__ void __launch_bounds__(kCalibrateLanes)
view_moment_sums_kernel(const float* __restrict__ poses, const float* __restrict__ kp, const uint8_t* __restrict__ flags, const long rows, const int J,
                        const int min_joints, double* __restrict__ partial)
{
    __shared__ double lds[kCalibrateLanes];
    const int v = (int)blockIdx.y;
    double* out = partial + ((long)v * gridDim.x + blockIdx.x) * kCalibrateSums;
    if (v == 0) {                                                        // (uniform)
        calibrate_chunk_zeros(out);
        return;
    }
    ViewMomentTerm term;
    term.poses = poses; term.kp = kp; term.flags = flags; term.rows = rows; term.J = J; term.v = v; term.min_joints = min_joints;
    calibrate_chunk_sums(rows, term, lds, out);
}

// Block (c, v).  intrinsics (V, 4) f64: fx, fy, cx, cy; pose (V, 8) f64 of solve_view_pose_kernel's stage 0.  View 0, a view whose state is
// not 1 and a view whose intrinsics are not finite with fx, fy > 0 hold zeros.
static __global__ void __launch_bounds__(kCalibrateLanes)
view_position_sums_kernel(const float* __restrict__ poses, const float* __restrict__ kp, const uint8_t* __restrict__ flags, const long rows,
                          const int J, const double* __restrict__ intrinsics, const int min_joints, const double* __restrict__ pose,
                          double* __restrict__ partial)
{
#pragma clang fp contract(off)
    __shared__ double lds[kCalibrateLanes];
    const int v = (int)blockIdx.y;
    double* out = partial + ((long)v * gridDim.x + blockIdx.x) * kCalibrateSums;
    bool live = v != 0 && pose[kCalibratePose * v + 7] == 1.0;
    for (int i = 0; i < 4; ++i) live = live && finite_double(intrinsics[i]) && finite_double(intrinsics[4 * v + i]);
    live = live && intrinsics[0] > 0.0 && intrinsics[1] > 0.0 && intrinsics[4 * v] > 0.0 && intrinsics[4 * v + 1] > 0.0;
    if (!live) {                                                         // (uniform)
        calibrate_chunk_zeros(out);
        return;
    }
    ViewPositionTerm term;
    term.poses = poses; term.kp = kp; term.flags = flags; term.rows = rows; term.J = J; term.v = v; term.min_joints = min_joints;
    term.c0.fx = intrinsics[0]; term.c0.fy = intrinsics[1]; term.c0.cx = intrinsics[2]; term.c0.cy = intrinsics[3];
    term.c0.w = 1.0; term.c0.x = 0.0; term.c0.y = 0.0; term.c0.z = 0.0;
    for (int i = 0; i < 9; ++i) term.c0.ax[i] = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0;
    term.cv.fx = intrinsics[4 * v]; term.cv.fy = intrinsics[4 * v + 1]; term.cv.cx = intrinsics[4 * v + 2]; term.cv.cy = intrinsics[4 * v + 3];
    const double* q = pose + kCalibratePose * v;
    term.cv.w = q[0]; term.cv.x = q[1]; term.cv.y = q[2]; term.cv.z = q[3];
    calibrate_turn(q[0], q[1], q[2], q[3], 1.0, 0.0, 0.0, term.cv.ax);
    calibrate_turn(q[0], q[1], q[2], q[3], 0.0, 1.0, 0.0, term.cv.ax + 3);
    calibrate_turn(q[0], q[1], q[2], q[3], 0.0, 0.0, 1.0, term.cv.ax + 6);
    calibrate_chunk_sums(rows, term, lds, out);
}

// One Jacobi rotation of the symmetric 4x4 in the plane (p, q), r and s the two other indices: the smaller-root tangent of UU3D_JACOBI_ROT
// (uu3d_metrics.h), every operation rounded once; a zero off-diagonal rotates nothing.  v_ip, v_iq: row i of the eigenvector matrix.
#define UU3D_JACOBI_ROT4(bpp, bqq, bpq, brp, brq, bsp, bsq, v0p, v0q, v1p, v1q, v2p, v2q, v3p, v3q)         \
    {                                                                                               \
        const double th = (bqq - bpp) / (2.0 * bpq);                                                \
        const double tt = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));              \
        const double t = (bpq == 0.0) ? 0.0 : tt;                                                   \
        const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;                                       \
        bpp = bpp - t * bpq; bqq = bqq + t * bpq; bpq = 0.0;                                        \
        double x_ = brp, y_ = brq; brp = c * x_ - sn * y_; brq = sn * x_ + c * y_;                  \
        x_ = bsp; y_ = bsq; bsp = c * x_ - sn * y_; bsq = sn * x_ + c * y_;                         \
        x_ = v0p; y_ = v0q; v0p = c * x_ - sn * y_; v0q = sn * x_ + c * y_;                         \
        x_ = v1p; y_ = v1q; v1p = c * x_ - sn * y_; v1q = sn * x_ + c * y_;                         \
        x_ = v2p; y_ = v2q; v2p = c * x_ - sn * y_; v2q = sn * x_ + c * y_;                         \
        x_ = v3p; y_ = v3q; v3p = c * x_ - sn * y_; v3q = sn * x_ + c * y_;                         \
    }

// Horn's symmetric 4x4 matrix from M = sum of p (x) p' (nine doubles M00, M01, ..., M22) -- its largest eigenvector is the quaternion that
// turns the p onto the p' --, then kCalibrateSweeps sweeps of cyclic Jacobi without an early exit: the eigenvalues b00 .. b33 (the diagonal)
// and the eigenvectors, a column each.  Shared by solve_view_pose_kernel and lift_pair_sums_kernel (uu3d_lift_match.h).
struct HornEigen { double b00, b11, b22, b33, v00, v01, v02, v03, v10, v11, v12, v13, v20, v21, v22, v23, v30, v31, v32, v33; };

__device__ __forceinline__ void horn_jacobi(const double m[9], HornEigen& h)
{
#pragma clang fp contract(off)
    const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5], m20 = m[6], m21 = m[7], m22 = m[8];
    double b00 = (m00 + m11) + m22, b01 = m12 - m21, b02 = m20 - m02, b03 = m01 - m10;
    double b11 = (m00 - m11) - m22, b12 = m01 + m10, b13 = m20 + m02;
    double b22 = (m11 - m00) - m22, b23 = m12 + m21;
    double b33 = (m22 - m00) - m11;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v03 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v13 = 0.0;
    double v20 = 0.0, v21 = 0.0, v22 = 1.0, v23 = 0.0, v30 = 0.0, v31 = 0.0, v32 = 0.0, v33 = 1.0;
#pragma unroll 1
    for (int sweep = 0; sweep < kCalibrateSweeps; ++sweep) {
        UU3D_JACOBI_ROT4(b00, b11, b01, b02, b12, b03, b13, v00, v01, v10, v11, v20, v21, v30, v31)
        UU3D_JACOBI_ROT4(b00, b22, b02, b01, b12, b03, b23, v00, v02, v10, v12, v20, v22, v30, v32)
        UU3D_JACOBI_ROT4(b00, b33, b03, b01, b13, b02, b23, v00, v03, v10, v13, v20, v23, v30, v33)
        UU3D_JACOBI_ROT4(b11, b22, b12, b01, b02, b13, b23, v01, v02, v11, v12, v21, v22, v31, v32)
        UU3D_JACOBI_ROT4(b11, b33, b13, b01, b03, b12, b23, v01, v03, v11, v13, v21, v23, v31, v33)
        UU3D_JACOBI_ROT4(b22, b33, b23, b02, b03, b12, b13, v02, v03, v12, v13, v22, v23, v32, v33)
    }
    h.b00 = b00; h.b11 = b11; h.b22 = b22; h.b33 = b33;
    h.v00 = v00; h.v01 = v01; h.v02 = v02; h.v03 = v03; h.v10 = v10; h.v11 = v11; h.v12 = v12; h.v13 = v13;
    h.v20 = v20; h.v21 = v21; h.v22 = v22; h.v23 = v23; h.v30 = v30; h.v31 = v31; h.v32 = v32; h.v33 = v33;
}

// One wave, lane v = view v.  partial (V, C, 10) f64 of one of the sum kernels; the lane adds its chunks in ascending order from 0.0.
// stage 0 (partial = the moment sums; pose_in unused): pose_out[v] = the quaternion that turns view v's axes onto view 0's, zeros, the state;
//     terms[v] = the rows both views see.  View 0: the identity, state 1, terms 0.  A refused view: the identity, state 0.
// stage 1 (partial = the position sums; pose_in = stage 0's rows): pose_out[v] = pose_in[v] with the position S c = g; a view whose state is
//     1 and whose solve is refused gets state 0 and keeps its quaternion; terms[v] = the rows of the position sums.
static __global__ void __launch_bounds__(64)
solve_view_pose_kernel(const double* __restrict__ partial, const int views, const long chunks, const int stage, const int min_terms,
                       const double* __restrict__ pose_in, double* __restrict__ pose_out, int* __restrict__ terms)
{
#pragma clang fp contract(off)
    const int v = threadIdx.x;
    if (v >= views) return;
    double x0 = 0.0, x1 = 0.0, x2 = 0.0, x3 = 0.0, x4 = 0.0, x5 = 0.0, x6 = 0.0, x7 = 0.0, x8 = 0.0, x9 = 0.0;
    for (long c = 0; c < chunks; ++c) {
        const double* __restrict__ p = partial + ((long)v * chunks + c) * kCalibrateSums;
        x0 = x0 + p[0]; x1 = x1 + p[1]; x2 = x2 + p[2]; x3 = x3 + p[3]; x4 = x4 + p[4];
        x5 = x5 + p[5]; x6 = x6 + p[6]; x7 = x7 + p[7]; x8 = x8 + p[8]; x9 = x9 + p[9];
    }
    double* __restrict__ out = pose_out + kCalibratePose * v;
    const int n = (int)x9;                                               // (whole numbers below 2^31: exact)
    terms[v] = n;
    if (stage != 0) {
        const double* __restrict__ in = pose_in + kCalibratePose * v;
        double t0 = in[4], t1 = in[5], t2 = in[6], state = in[7];
        if (v != 0 && state == 1.0) {
            const double a00 = x0, a01 = x1, a02 = x2, a11 = x3, a12 = x4, a22 = x5, b0 = x6, b1 = x7, b2 = x8;
            const double c00 = a11 * a22 - a12 * a12;
            const double c01 = a02 * a12 - a01 * a22;
            const double c02 = a01 * a12 - a02 * a11;
            const double c11 = a00 * a22 - a02 * a02;
            const double c12 = a01 * a02 - a00 * a12;
            const double c22 = a00 * a11 - a01 * a01;
            const double det = (a00 * c00 + a01 * c01) + a02 * c02;
            const double y0 = (c00 * b0 + c01 * b1) + c02 * b2;
            const double y1 = (c01 * b0 + c11 * b1) + c12 * b2;
            const double y2 = (c02 * b0 + c12 * b1) + c22 * b2;
            const double p0 = y0 / det, p1 = y1 / det, p2 = y2 / det;
            bool ok = finite_double(det) && det > 0.0 && det > kViewRank * ((a00 * a11) * a22);
            ok = ok && finite_double(p0) && finite_double(p1) && finite_double(p2);
            t0 = ok ? p0 : 0.0; t1 = ok ? p1 : 0.0; t2 = ok ? p2 : 0.0;
            state = ok ? 1.0 : 0.0;
        }
        out[0] = in[0]; out[1] = in[1]; out[2] = in[2]; out[3] = in[3];
        out[4] = t0; out[5] = t1; out[6] = t2; out[7] = state;
        return;
    }
    double q0 = 1.0, q1 = 0.0, q2 = 0.0, q3 = 0.0, state = 1.0;
    if (v != 0) {
        const double m[9] = {x0, x1, x2, x3, x4, x5, x6, x7, x8};
        HornEigen h;
        horn_jacobi(m, h);
        const double b00 = h.b00, b11 = h.b11, b22 = h.b22, b33 = h.b33;
        const double v00 = h.v00, v01 = h.v01, v02 = h.v02, v03 = h.v03, v10 = h.v10, v11 = h.v11, v12 = h.v12, v13 = h.v13;
        const double v20 = h.v20, v21 = h.v21, v22 = h.v22, v23 = h.v23, v30 = h.v30, v31 = h.v31, v32 = h.v32, v33 = h.v33;
        // the column of the largest eigenvalue, ties to the smaller index; `next` = the largest of the others
        double top = b00, next = -__builtin_huge_val();
        double e0 = v00, e1 = v10, e2 = v20, e3 = v30;
        if (b11 > top) { next = top; top = b11; e0 = v01; e1 = v11; e2 = v21; e3 = v31; } else if (b11 > next) next = b11;
        if (b22 > top) { next = top; top = b22; e0 = v02; e1 = v12; e2 = v22; e3 = v32; } else if (b22 > next) next = b22;
        if (b33 > top) { next = top; top = b33; e0 = v03; e1 = v13; e2 = v23; e3 = v33; } else if (b33 > next) next = b33;
        const double nn = ((e0 * e0 + e1 * e1) + e2 * e2) + e3 * e3;
        const double len = sqrt(nn);
        double u0 = e0 / len, u1 = e1 / len, u2 = e2 / len, u3 = e3 / len;
        if (u0 < 0.0) { u0 = -u0; u1 = -u1; u2 = -u2; u3 = -u3; }
        bool ok = n >= min_terms;
        ok = ok && finite_double(b00) && finite_double(b11) && finite_double(b22) && finite_double(b33);
        ok = ok && finite_double(u0) && finite_double(u1) && finite_double(u2) && finite_double(u3);
        ok = ok && (top - next > kCalibrateGap * fabs(top));             // closer: the lifts do not fix a rotation
        q0 = ok ? u0 : 1.0; q1 = ok ? u1 : 0.0; q2 = ok ? u2 : 0.0; q3 = ok ? u3 : 0.0;
        state = ok ? 1.0 : 0.0;
    }
    out[0] = q0; out[1] = q1; out[2] = q2; out[3] = q3;
    out[4] = 0.0; out[5] = 0.0; out[6] = 0.0; out[7] = state;
}

}  // namespace uu3d
