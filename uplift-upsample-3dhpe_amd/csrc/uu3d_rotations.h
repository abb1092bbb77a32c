// uu3d_rotations.h -- JOINT ROTATIONS (include/uu3d.h; rotations.joint_rotations, predict.predict_tracks(rotations=...),
// stream.StreamSession(rotations=...)): per pose and joint the unit quaternion (w, x, y, z) that turns the joint's rest frame onto the
// pose, relative to its parent's frame -- what a character rig, a game engine or a BVH file takes.
//     joint_rotations_kernel        one wave per frame, lane j owns joint j; the tree is walked level by level from the root outwards and a
//                                   parent's global quaternion reaches its children through LDS
//     joint_rotations_reset_kernel  live: the chosen slots' quaternions are identities again
// The rule is rotations.joint_rotations_host's, statement for statement, in float64 with every operation rounded once in the written
// order (no fused multiply-add, IEEE square root and division, no trigonometry): the device equals the numpy mirror bit for bit.  Every
// output element has one writer, no atomics, the caller's buffers are only read: bitwise repeatable, capturable.
#pragma once
#include "uu3d_bones.h"

namespace uu3d {

static constexpr int kRotationWaves = 4;                                // frames per workgroup: one wave each

struct Quat {
    double w, x, y, z;
};

// a * b (Hamilton), every component summed left to right
__device__ __forceinline__ Quat quat_mul(const Quat a, const Quat b)
{
#pragma clang fp contract(off)
    Quat r;
    r.w = ((a.w * b.w - a.x * b.x) - a.y * b.y) - a.z * b.z;
    r.x = ((a.w * b.x + a.x * b.w) + a.y * b.z) - a.z * b.y;
    r.y = ((a.w * b.y - a.x * b.z) + a.y * b.w) + a.z * b.x;
    r.z = ((a.w * b.z + a.x * b.y) - a.y * b.x) + a.z * b.w;
    return r;
}

// q / |q|,  |q| = sqrt(((w w + x x) + y y) + z z)
__device__ __forceinline__ Quat quat_unit(const Quat q)
{
#pragma clang fp contract(off)
    const double n = sqrt(((q.w * q.w + q.x * q.x) + q.y * q.y) + q.z * q.z);
    Quat r;
    r.w = q.w / n;
    r.x = q.x / n;
    r.y = q.y / n;
    r.z = q.z / n;
    return r;
}

__device__ __forceinline__ double vec_dot(const double a0, const double a1, const double a2, const double b0, const double b1, const double b2)
{
#pragma clang fp contract(off)
    return (a0 * b0 + a1 * b1) + a2 * b2;
}

__device__ __forceinline__ void vec_cross(const double a0, const double a1, const double a2, const double b0, const double b1, const double b2,
                                          double& c0, double& c1, double& c2)
{
#pragma clang fp contract(off)
    c0 = a1 * b2 - a2 * b1;
    c1 = a2 * b0 - a0 * b2;
    c2 = a0 * b1 - a1 * b0;
}

// v' = q v q*:  t = 2 (q.xyz x v);  v' = (v + q.w t) + q.xyz x t
__device__ __forceinline__ void quat_rotate(const Quat q, const double v0, const double v1, const double v2, double& r0, double& r1, double& r2)
{
#pragma clang fp contract(off)
    double t0, t1, t2, u0, u1, u2;
    vec_cross(q.x, q.y, q.z, v0, v1, v2, t0, t1, t2);
    t0 = 2.0 * t0;
    t1 = 2.0 * t1;
    t2 = 2.0 * t2;
    vec_cross(q.x, q.y, q.z, t0, t1, t2, u0, u1, u2);
    r0 = (v0 + q.w * t0) + u0;
    r1 = (v1 + q.w * t1) + u1;
    r2 = (v2 + q.w * t2) + u2;
}

// The shortest arc from a onto b: (|a||b| + a.b, a x b), normalised.  Antiparallel (the scalar part <= 0 and the cross product zero):
// a half turn about (f0, f1, f2) if `given_axis`, else about a x e, e the coordinate axis of a's smallest-magnitude component (ties: the
// lowest index).
__device__ __forceinline__ Quat quat_arc(const double a0, const double a1, const double a2, const double b0, const double b1, const double b2,
                                         const bool given_axis, const double f0, const double f1, const double f2)
{
#pragma clang fp contract(off)
    const double na = sqrt(vec_dot(a0, a1, a2, a0, a1, a2)), nb = sqrt(vec_dot(b0, b1, b2, b0, b1, b2));
    Quat q;
    q.w = na * nb + vec_dot(a0, a1, a2, b0, b1, b2);
    vec_cross(a0, a1, a2, b0, b1, b2, q.x, q.y, q.z);
    if (q.w <= 0.0 && q.x == 0.0 && q.y == 0.0 && q.z == 0.0) {
        q.w = 0.0;
        if (given_axis) {
            q.x = f0;
            q.y = f1;
            q.z = f2;
        } else {
            int k = 0;
            double m = fabs(a0);
            if (fabs(a1) < m) { k = 1; m = fabs(a1); }
            if (fabs(a2) < m) k = 2;
            q.x = k == 0 ? 0.0 : (k == 1 ? -a2 : a1);                    // a x e_k
            q.y = k == 0 ? a2 : (k == 1 ? 0.0 : -a0);
            q.z = k == 0 ? -a1 : (k == 1 ? a0 : 0.0);
        }
    }
    return quat_unit(q);
}

__device__ __forceinline__ bool vec_usable(const double v0, const double v1, const double v2)
{
    return finite_double(v0) && finite_double(v1) && finite_double(v2) && !(v0 == 0.0 && v1 == 0.0 && v2 == 0.0);
}

// poses (frames, J, 3) f32; tree (4, J) i32: parents, primary child, secondary child (-1: none), level (0 for the root); depth: the
// largest level; rest (J, 3) f64 unit directions by child joint; row_mask (frames) u8 or nullptr: a frame whose entry is 0 is not
// touched.  local, global (frames, J, 4) f32 (global may be nullptr), flags (frames, J) u8 or nullptr.  An index out of range counts as
// "no child" / "no parent", a joint whose level is outside [0, depth] gets identities and flag 0: nothing is read or written out of bounds.
static __global__ void __launch_bounds__(kRotationWaves * kBonesLanes)
joint_rotations_kernel(const float* __restrict__ poses, const long frames, const int J, const int32_t* __restrict__ tree, const int depth,
                       const double* __restrict__ rest, const uint8_t* __restrict__ row_mask, float* __restrict__ local,
                       float* __restrict__ global, uint8_t* __restrict__ flags)
{
#pragma clang fp contract(off)
    __shared__ double Qs[kRotationWaves][kBonesLanes][4];
    const int wave = threadIdx.x / kBonesLanes, j = threadIdx.x % kBonesLanes;
    const long f = (long)blockIdx.x * kRotationWaves + wave;
    const bool live = f < frames && j < J && (row_mask == nullptr || row_mask[f] != 0);
    int p = -1, c1 = -1, c2 = -1, level = -1;
    if (live) {
        p = tree[j];
        c1 = tree[J + j];
        c2 = tree[2 * J + j];
        level = tree[3 * J + j];
        if (!bone_parent_ok(j, p, J)) p = -1;
        if (c1 < 0 || c1 >= J || c1 == j) c1 = -1;
        if (c2 < 0 || c2 >= J || c2 == j || c1 < 0) c2 = -1;
    }
    const float* row = poses + f * J * 3;
    const long e = f * J + j;
    if (live && (level < 0 || level > depth)) {
        *(float4*)(local + e * 4) = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
        if (global != nullptr) *(float4*)(global + e * 4) = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
        if (flags != nullptr) flags[e] = 0;
    }
    for (int lvl = 0; lvl <= depth; ++lvl) {
        if (live && level == lvl) {
            Quat par{1.0, 0.0, 0.0, 0.0};
            if (p >= 0) par = Quat{Qs[wave][p][0], Qs[wave][p][1], Qs[wave][p][2], Qs[wave][p][3]};
            Quat q = par, loc{1.0, 0.0, 0.0, 0.0};
            uint8_t flag = 1;
            if (c1 >= 0) {
                double b0, b1, b2;
                const double nb = bone_offset(row, c1, j, b0, b1, b2);
                if (!bone_length_ok(nb)) flag = 0;
                else {
                    double a0, a1, a2;
                    quat_rotate(par, rest[c1 * 3 + 0], rest[c1 * 3 + 1], rest[c1 * 3 + 2], a0, a1, a2);
                    q = quat_unit(quat_mul(quat_arc(a0, a1, a2, b0, b1, b2, false, 0.0, 0.0, 0.0), par));
                    if (c2 >= 0) {
                        const double u0 = b0 / nb, u1 = b1 / nb, u2 = b2 / nb;
                        double s0, s1, s2, t0, t1, t2;
                        quat_rotate(q, rest[c2 * 3 + 0], rest[c2 * 3 + 1], rest[c2 * 3 + 2], s0, s1, s2);
                        bone_offset(row, c2, j, t0, t1, t2);
                        const double ds = vec_dot(s0, s1, s2, u0, u1, u2), dt = vec_dot(t0, t1, t2, u0, u1, u2);
                        s0 = s0 - u0 * ds;
                        s1 = s1 - u1 * ds;
                        s2 = s2 - u2 * ds;
                        t0 = t0 - u0 * dt;
                        t1 = t1 - u1 * dt;
                        t2 = t2 - u2 * dt;
                        if (vec_usable(s0, s1, s2) && vec_usable(t0, t1, t2))
                            q = quat_unit(quat_mul(quat_arc(s0, s1, s2, t0, t1, t2, true, u0, u1, u2), q));
                    }
                    loc = quat_unit(quat_mul(Quat{par.w, -par.x, -par.y, -par.z}, q));
                    // (plain | and & on the comparisons, then four selects: straight-line code, no nest of short-circuit branches)
                    const bool negative = (loc.w < 0.0) | ((loc.w == 0.0) & ((loc.x < 0.0) | ((loc.x == 0.0) & ((loc.y < 0.0) | ((loc.y == 0.0) & (loc.z < 0.0))))));
                    loc.w = negative ? -loc.w : loc.w;
                    loc.x = negative ? -loc.x : loc.x;
                    loc.y = negative ? -loc.y : loc.y;
                    loc.z = negative ? -loc.z : loc.z;
                }
            }
            Qs[wave][j][0] = q.w;
            Qs[wave][j][1] = q.x;
            Qs[wave][j][2] = q.y;
            Qs[wave][j][3] = q.z;
            *(float4*)(local + e * 4) = make_float4((float)loc.w, (float)loc.x, (float)loc.y, (float)loc.z);
            if (global != nullptr) *(float4*)(global + e * 4) = make_float4((float)q.w, (float)q.x, (float)q.y, (float)q.z);
            if (flags != nullptr) flags[e] = flag;
        }
        __syncthreads();
    }
}

// local, global (slots, J, 4) f32 (global may be nullptr), flags (slots, J) u8 or nullptr; slot_mask (slots) u8 or nullptr (every slot):
// the chosen slots hold identities and flags 0.  One wave per slot.
static __global__ void __launch_bounds__(kBonesLanes)
joint_rotations_reset_kernel(const uint8_t* __restrict__ slot_mask, const int J, float* __restrict__ local, float* __restrict__ global,
                             uint8_t* __restrict__ flags)
{
    const int slot = blockIdx.x, j = threadIdx.x;
    if (j >= J || (slot_mask != nullptr && slot_mask[slot] == 0)) return;
    const long e = (long)slot * J + j;
    *(float4*)(local + e * 4) = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
    if (global != nullptr) *(float4*)(global + e * 4) = make_float4(1.0f, 0.0f, 0.0f, 0.0f);
    if (flags != nullptr) flags[e] = 0;
}

}  // namespace uu3d
