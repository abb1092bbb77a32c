// uu3d_repair.h -- PER-JOINT MISSED DETECTIONS (include/uu3d.h; predict.predict_tracks(repair_joints=G)): a joint a detector lost for a few
// frames is filled by linear interpolation between the nearest frames where it was seen, on the device, in front of the kernels of
// uu3d_tracks.h.  Three launches on one stream:
//     repair_plan_kernel   per (track, joint): the nearest observed frame at or before / at or after every frame, two segmented scans
//     repair_apply_kernel  per 16 bytes of the repaired source: the fill (resample_mix, the bits of predict.repair_joints_host) and the state
//     repair_flag_kernel   per frame, one wave: the frame flag from the joint states
// Every output element has one writer and is a function of inputs that nobody writes: bitwise repeatable.  The cost does not depend on G.
#pragma once
#include "uu3d_tracks.h"

namespace uu3d {

static constexpr int kRepairChunk = 256;                                // frames per scan step = threads per workgroup
static constexpr int32_t kRepairNone = INT32_MAX;                       // "no observed frame to the right" (rows < 2^31, so never a row); to the left: -1

// Joint p = row * J + j is OBSERVED: its flag (nullptr: none given) is non-zero and both coordinates are finite.
__device__ __forceinline__ bool joint_observed(const float* __restrict__ src, const uint8_t* __restrict__ joint_flags, const long p)
{
    if (joint_flags != nullptr && joint_flags[p] == 0) return false;
    return finite_pair(*reinterpret_cast<const float2*>(src + p * 2));
}

// left[row * J + j] = the largest row' <= row of the same track where joint j is observed (-1: none); right[...] = the smallest
// row' >= row (kRepairNone: none).  An observed joint names itself; for an unobserved one these are the rule's l and r.
// One workgroup per (track, joint), thread i of 256 on frame i of the chunk, the chunks of a track in order with the carry in a register:
// a max-scan of (observed ? row : -1) running forwards, then a min-scan of (observed ? row : kRepairNone) running backwards -- inside a
// wave by __shfl_up / __shfl_down, across the four waves through four words of LDS.  Why per (track, joint) and not per track: a call
// has few tracks (often one), and J workgroups per track is the only parallelism a scan along the frames leaves; the price is that the J
// workgroups of a track each read 8 of every 8 J bytes of the same lines, which they share in L2 (they are neighbours in the grid).
// track_start (num_tracks + 1): track t is rows [track_start[t], track_start[t + 1]), clamped into [0, rows].
static __global__ void __launch_bounds__(kRepairChunk)
repair_plan_kernel(const float* __restrict__ src, const uint8_t* __restrict__ joint_flags, const long rows, const int J,
                   const int64_t* __restrict__ track_start, int32_t* __restrict__ left, int32_t* __restrict__ right)
{
    __shared__ int wave_edge[kRepairChunk / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = blockIdx.x / J, j = blockIdx.x - t * J;
    long begin = track_start[t], end = track_start[t + 1];
    begin = begin < 0 ? 0 : (begin > rows ? rows : begin);
    end = end < begin ? begin : (end > rows ? rows : end);

    int carry = -1;
    for (long base = begin; base < end; base += kRepairChunk) {
        const long row = base + tid;
        int v = (row < end && joint_observed(src, joint_flags, row * J + j)) ? (int)row : -1;
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
        if (row < end) left[row * J + j] = max(v, before);
        __syncthreads();                                                 // (wave_edge is rewritten by the next chunk)
    }

    carry = kRepairNone;
    const long chunks = (end - begin + kRepairChunk - 1) / kRepairChunk;
    for (long c = chunks - 1; c >= 0; --c) {
        const long row = begin + c * kRepairChunk + tid;
        int v = (row < end && joint_observed(src, joint_flags, row * J + j)) ? (int)row : kRepairNone;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_down(v, d);
            if (lane + d < 64) v = min(v, o);
        }
        if (lane == 0) wave_edge[wave] = v;
        __syncthreads();
        int behind = carry;                                              // everything behind this wave
#pragma unroll
        for (int w = 0; w < kRepairChunk / 64; ++w) {
            if (w > wave) behind = min(behind, wave_edge[w]);
            carry = min(carry, wave_edge[w]);
        }
        if (row < end) right[row * J + j] = min(v, behind);
        __syncthreads();
    }
}

// out (rows, J, 2) and state (rows, J): one thread per two joints = one 16-byte store and one 2-byte store.  An observed joint keeps its
// bits (state 1).  An unobserved one with l = left, r = right (max_gap = G):
//     l and r exist and r - l - 1 <= G:  resample_mix(src[l], src[r], double(row - l) / double(r - l)) per coordinate
//     only r exists and r - row <= G:    the bits of src[r]            only l exists and row - l <= G:  the bits of src[l]
// (state 2), else zeros (state 0).  A plan entry that does not lie on its side of the row inside [0, rows) -- scratch the plan launch did
// not write because track_start does not cover the row -- gives NaN and state 0 instead of a read out of bounds.
static __global__ void __launch_bounds__(256)
repair_apply_kernel(const float* __restrict__ src, const uint8_t* __restrict__ joint_flags, const long rows, const int J,
                    const int32_t* __restrict__ left, const int32_t* __restrict__ right, const int max_gap, float* __restrict__ out,
                    uint8_t* __restrict__ state)
{
    const long pairs = rows * J;
    const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * 2;
    if (p0 >= pairs) return;
    float2 v[2];
    uint8_t s[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const long p = (p0 + e < pairs) ? p0 + e : p0;
        const long row = p / J;
        const int j = (int)(p - row * J);
        const float2 x = *reinterpret_cast<const float2*>(src + p * 2);
        v[e] = x;
        s[e] = 1;
        if (joint_observed(src, joint_flags, p)) continue;
        const long l = left[p], r = right[p];
        const bool has_l = l >= 0, has_r = r != kRepairNone;
        const float nan = __builtin_nanf("");
        v[e] = make_float2(nan, nan);
        s[e] = 0;
        if (l < -1 || l >= row || (has_r && (r <= row || r >= rows))) continue;
        v[e] = make_float2(0.f, 0.f);
        const long gap = max_gap;
        if (has_l && has_r) {
            if (r - l - 1 > gap) continue;
            const float2 a = *reinterpret_cast<const float2*>(src + (l * J + j) * 2);
            const float2 b = *reinterpret_cast<const float2*>(src + (r * J + j) * 2);
            const double w = (double)(row - l) / (double)(r - l);
            v[e] = make_float2(resample_mix(a.x, b.x, w), resample_mix(a.y, b.y, w));
        } else if (has_r) {
            if (r - row > gap) continue;
            v[e] = *reinterpret_cast<const float2*>(src + (r * J + j) * 2);
        } else if (has_l) {
            if (row - l > gap) continue;
            v[e] = *reinterpret_cast<const float2*>(src + (l * J + j) * 2);
        } else {
            continue;                                                    // never observed in this track
        }
        s[e] = 2;
    }
    if (p0 + 1 < pairs) {
        *reinterpret_cast<float4*>(out + p0 * 2) = make_float4(v[0].x, v[0].y, v[1].x, v[1].y);
        *reinterpret_cast<uchar2*>(state + p0) = make_uchar2(s[0], s[1]);
    } else {
        *reinterpret_cast<float2*>(out + p0 * 2) = v[0];
        state[p0] = s[0];
    }
}

// frame_valid[row] = the frame is a real observation: at least one joint observed (state 1) and no joint left unrepaired (state 0).  One
// wave per row, four rows per workgroup, lane 0 writes the byte, as track_valid_kernel; it runs after repair_apply_kernel on the same stream.
static __global__ void __launch_bounds__(256)
repair_flag_kernel(const uint8_t* __restrict__ state, const long rows, const int J, uint8_t* __restrict__ frame_valid)
{
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                             // (whole waves leave: `row` is uniform in a wave)
    bool complete = true, seen = false;
    for (int j = lane; j < J; j += 64) {
        const uint8_t s = state[row * J + j];
        complete = complete && s != 0;
        seen = seen || s == 1;
    }
    const bool ok = __all(complete) != 0 && __any(seen) != 0;
    if (lane == 0) frame_valid[row] = ok ? 1 : 0;
}

}  // namespace uu3d
