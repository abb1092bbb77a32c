// uu3d_root.h -- ABSOLUTE ROOT POSITION (include/uu3d.h; predict.solve_roots, predict.predict_tracks(camera=...)): where the root-relative
// skeleton of every frame must stand in the camera's space so that it projects onto the 2D keypoints it was uplifted from, and the root
// trajectory of a track read at the times of the returned frames.
//     solve_roots_kernel      per given frame, one lane: the normal equations of Tx - a Tz = p, Ty - b Tz = q over the used joints
//     root_scan_kernel        per track, one workgroup: the nearest solved frame at or before / behind every given frame, two segmented scans
//     root_trajectory_kernel  per returned frame, one lane: the solved frame's bits, the mix of its two solved neighbours, or the held end
// Every output element has one writer and is a function of inputs that nobody writes: bitwise repeatable.  The scans are those of
// uu3d_repair.h (kRepairChunk frames per step, the carry in a register); the cost does not depend on the length of a gap.
#pragma once
#include "uu3d_repair.h"

namespace uu3d {

static constexpr int kRootMaxJoints = 64;                               // J beyond it: UU3D_ERR_UNSUPPORTED (the conventions of uu3d_associate.h)

__device__ __forceinline__ bool finite_double(const double x)
{
    return ((unsigned long long)__double_as_longlong(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// The solve of one frame, every product and sum rounded (no fused multiply-add), the sums in ascending joint order: the statements of
// predict.solve_roots_host, one for one.  pose (J, 3) f32, kp (J, 2) f32, flags (J) u8 or nullptr, cam = (fx, fy, cx, cy).
// -> solved; T = the root, zeros when the frame is not solved.
__device__ __forceinline__ bool solve_root(const float* __restrict__ pose, const float* __restrict__ kp, const uint8_t* __restrict__ flags, const int J,
                                           const double* __restrict__ cam, const int min_joints, double T[3])
{
#pragma clang fp contract(off)
    T[0] = T[1] = T[2] = 0.0;
    const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3];
    if (!finite_double(fx) || !finite_double(fy) || !finite_double(cx) || !finite_double(cy) || !(fx > 0.0) || !(fy > 0.0)) return false;
    int n = 0;
    double Sa = 0.0, Sb = 0.0, Sq = 0.0, Sp = 0.0, Sk = 0.0, Sr = 0.0;
    for (int j = 0; j < J; ++j) {
        if (flags != nullptr && flags[j] == 0) continue;
        const float2 uv = *reinterpret_cast<const float2*>(kp + 2 * j);
        if (!finite_pair(uv)) continue;
        const double X = (double)pose[3 * j], Y = (double)pose[3 * j + 1], Z = (double)pose[3 * j + 2];
        const double a = ((double)uv.x - cx) / fx;
        const double b = ((double)uv.y - cy) / fy;
        const double p = a * Z - X;
        const double q = b * Z - Y;
        n += 1;
        Sa = Sa + a;
        Sb = Sb + b;
        Sq = Sq + (a * a + b * b);
        Sp = Sp + p;
        Sk = Sk + q;
        Sr = Sr + (a * p + b * q);
    }
    if (n < min_joints) return false;
    const double nd = (double)n;
    const double den = Sq - (Sa * Sa + Sb * Sb) / nd;
    if (!(den > 0.0)) return false;
    const double num = (Sa * Sp + Sb * Sk) / nd - Sr;
    const double Tz = num / den;
    const double Tx = (Sp + Sa * Tz) / nd;
    const double Ty = (Sk + Sb * Tz) / nd;
    if (!finite_double(Tx) || !finite_double(Ty) || !finite_double(Tz) || !(Tz > 0.0)) return false;
    for (int j = 0; j < J; ++j) {                                        // every used joint in front of the camera
        if (flags != nullptr && flags[j] == 0) continue;
        if (!finite_pair(*reinterpret_cast<const float2*>(kp + 2 * j))) continue;
        if (!((double)pose[3 * j + 2] + Tz > 0.0)) return false;
    }
    T[0] = Tx; T[1] = Ty; T[2] = Tz;
    return true;
}

// roots (frames, 3) f64 and solved (frames) u8: one lane per frame.  row_track (frames) i32 or nullptr (every frame takes camera 0);
// cameras (num_tracks, 4) f64.  A track id out of range: not solved, zeros, nothing read out of bounds.
static __global__ void __launch_bounds__(256)
solve_roots_kernel(const float* __restrict__ poses, const float* __restrict__ kp, const uint8_t* __restrict__ joint_flags, const long frames,
                   const int J, const int32_t* __restrict__ row_track, const int num_tracks, const double* __restrict__ cameras,
                   const int min_joints, double* __restrict__ roots, uint8_t* __restrict__ solved)
{
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= frames) return;
    const int t = row_track != nullptr ? row_track[g] : 0;
    double T[3] = {0.0, 0.0, 0.0};
    bool ok = false;
    if (t >= 0 && t < num_tracks)
        ok = solve_root(poses + g * J * 3, kp + g * J * 2, joint_flags != nullptr ? joint_flags + g * J : nullptr, J, cameras + 4 * (long)t,
                        min_joints, T);
    roots[g * 3] = T[0];
    roots[g * 3 + 1] = T[1];
    roots[g * 3 + 2] = T[2];
    solved[g] = ok ? 1 : 0;
}

// left[g] = the largest g' <= g of the same track with solved[g'] (-1: none); right[g] = the smallest g' > g (kRepairNone: none).  One
// workgroup per track, thread i on frame i of the chunk, the chunks in order with the carry in a register: repair_plan_kernel's two
// scans, the one running backwards made exclusive (a lane takes its right neighbour's inclusive value), so that a position between
// frame g and frame g + 1 finds both of its neighbours at g without a look across the track's end.
static __global__ void __launch_bounds__(kRepairChunk)
root_scan_kernel(const uint8_t* __restrict__ solved, const long frames, const int64_t* __restrict__ track_start, int32_t* __restrict__ left,
                 int32_t* __restrict__ right)
{
    __shared__ int wave_edge[kRepairChunk / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long begin = track_start[blockIdx.x], end = track_start[blockIdx.x + 1];
    begin = begin < 0 ? 0 : (begin > frames ? frames : begin);
    end = end < begin ? begin : (end > frames ? frames : end);

    int carry = -1;
    for (long base = begin; base < end; base += kRepairChunk) {
        const long row = base + tid;
        int v = (row < end && solved[row] != 0) ? (int)row : -1;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(v, d);
            if (lane >= d) v = max(v, o);
        }
        if (lane == 63) wave_edge[wave] = v;
        __syncthreads();
        int before = carry;                                              // everything in front of this wave
#pragma unroll
        for (int w = 0; w < kRepairChunk / 64; ++w) {
            if (w < wave) before = max(before, wave_edge[w]);
            carry = max(carry, wave_edge[w]);
        }
        if (row < end) left[row] = max(v, before);
        __syncthreads();                                                 // (wave_edge is rewritten by the next chunk)
    }

    carry = kRepairNone;
    const long chunks = (end - begin + kRepairChunk - 1) / kRepairChunk;
    for (long c = chunks - 1; c >= 0; --c) {
        const long row = begin + c * kRepairChunk + tid;
        int v = (row < end && solved[row] != 0) ? (int)row : kRepairNone;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_down(v, d);
            if (lane + d < 64) v = min(v, o);
        }
        if (lane == 0) wave_edge[wave] = v;
        __syncthreads();
        const int next = __shfl_down(v, 1);                              // the inclusive value one frame on; lane 63 has none in its wave
        int behind = carry;                                              // everything behind this wave
#pragma unroll
        for (int w = 0; w < kRepairChunk / 64; ++w) {
            if (w > wave) behind = min(behind, wave_edge[w]);
            carry = min(carry, wave_edge[w]);
        }
        if (row < end) right[row] = lane < 63 ? min(next, behind) : behind;
        __syncthreads();
    }
}

// a * (1.0 - w) + b * w on float64 roots: two products and one sum, each rounded, then rounded once to float32 (resample_mix's expression).
__device__ __forceinline__ float root_mix(const double a, const double b, const double w)
{
#pragma clang fp contract(off)
    const double pa = a * (1.0 - w);
    const double pb = b * w;
    return (float)(pa + pb);
}

// Returned frame i sits at given-frame position base[i] + rem[i] / den[i] (base a global row of the given frames, 0 <= rem < den), the
// host's exact plan.  L = left[base], R = right[base]:
//     rem == 0 and L == base: a solved given frame, its bits rounded to float32, state 1
//     L and R exist: root_mix(roots[L], roots[R], double((base - L) den + rem) / double((R - L) den)), state 2
//     only one exists: its root, held, state 2                      neither: zeros, state 0
// A plan row outside [0, frames), den < 1, rem outside [0, den), or a scan entry that does not lie on its side of base inside [0, frames)
// -- scratch the scan did not write because track_start does not cover the row -- gives NaN and state 0 instead of a read out of bounds.
static __global__ void __launch_bounds__(256)
root_trajectory_kernel(const double* __restrict__ roots, const long frames, const int32_t* __restrict__ left, const int32_t* __restrict__ right,
                       const int64_t* __restrict__ base, const int64_t* __restrict__ rem, const int64_t* __restrict__ den, const long out_frames,
                       float* __restrict__ out, uint8_t* __restrict__ state)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= out_frames) return;
    const float nan = __builtin_nanf("");
    float v[3] = {nan, nan, nan};
    uint8_t s = 0;
    const long b = base[i], r0 = rem[i], d = den[i];
    if (b >= 0 && b < frames && d >= 1 && r0 >= 0 && r0 < d) {
        const long L = left[b], R = right[b];
        const bool has_l = L >= 0, has_r = R != kRepairNone;
        if (L >= -1 && L <= b && (!has_r || (R > b && R < frames))) {
            if (has_l && L == b && r0 == 0) {
                for (int c = 0; c < 3; ++c) v[c] = (float)roots[b * 3 + c];
                s = 1;
            } else if (has_l && has_r) {
                const double w = (double)((b - L) * d + r0) / (double)((R - L) * d);
                for (int c = 0; c < 3; ++c) v[c] = root_mix(roots[L * 3 + c], roots[R * 3 + c], w);
                s = 2;
            } else if (has_l || has_r) {
                const long h = has_l ? L : R;
                for (int c = 0; c < 3; ++c) v[c] = (float)roots[h * 3 + c];
                s = 2;
            } else {
                v[0] = v[1] = v[2] = 0.f;
            }
        }
    }
    out[i * 3] = v[0];
    out[i * 3 + 1] = v[1];
    out[i * 3 + 2] = v[2];
    state[i] = s;
}

}  // namespace uu3d
