// uu3d_stream_repair.h -- LIVE PER-JOINT MISSED DETECTIONS (stream.StreamSession(repair_joints=G); include/uu3d.h): the rule of uu3d_repair.h
// run incrementally, one pushed frame per slot and tick.  The session's contract is unchanged -- the pose of frame t - lookahead is the one
// predict_tracks(repair_joints=G) gives on the track cut at t -- so a push may REVISE frames the session has filed already:
//   * coordinates change only for frames t - G .. t (a gap of at most G frames closes at t: held -> interpolated; a joint is seen for the
//     first time at t: unfilled -> held from t); of those the ring keeps the multiples of s_in and the edge frame: K = G / s_in + 2 frames;
//   * an older frame can only go from valid to MISSING (a gap longer than G closes at t: the up to G frames held from its left end become
//     unfillable): a byte of valid_state, no features.
// Two kernels around uu3d_frame_features (over halves * slots * K staged frames):
//   stream_repair_stage_kernel   per slot: file the pushed raw frame and flags in a ring of G + 1 frames, work out the K frames to re-stage
//                                and the far list, write the re-staged frames normalised (normalize_pair) with their mirrored copies
//   stream_commit_repair_kernel  stream_commit_kernel with another filing step: the K staged frames into the ring places and the edge row
//                                that still hold them, the far list into their valid bytes; then the same window (stream_write_window)
// The state a slot needs is bounded (the host mirror, written to be read: stream.LiveRepairHost): the raw coordinates and observed flags of
// frames t - G .. t; per joint the last observation that has left that window (index + 1, 0 = none, and its coordinates); per joint G bits:
// which of the G frames behind that observation have left the window as valid frames -- the ones a long gap turns missing when it closes.
// One workgroup (one wave) per slot, one lane per joint; a slot's state is touched by its own workgroup only.  No atomics, one writer per
// output element, the counters are read on the device: the launches have the same arguments at every tick.
#pragma once
#include "uu3d_stream.h"

namespace uu3d {

static constexpr int kLiveRepairMaxGap = 32;                            // G <= 32: the held-frame bits of a joint are one 32-bit word

// The repair state of a session, caller-allocated like valid_state; all zeros = every slot empty.
struct RepairLayout {
    int W, K;                                                           // frames in the raw ring (G + 1), frames re-staged per slot and tick
    size_t off_raw, off_last_xy, off_last, off_held, off_observed, bytes;
};
inline RepairLayout repair_layout(const int slots, const int J, const int s_in, const int G)
{
    RepairLayout R{};
    R.W = G + 1; R.K = G / s_in + 2;
    R.off_raw = 0;                                                                              // (slots, W, J, 2) f32
    R.off_last_xy = R.off_raw + stream_align((size_t)slots * R.W * J * 2 * sizeof(float));      // (slots, J, 2) f32
    R.off_last = R.off_last_xy + stream_align((size_t)slots * J * 2 * sizeof(float));           // (slots, J) i32: index + 1
    R.off_held = R.off_last + stream_align((size_t)slots * J * sizeof(int32_t));                // (slots, J) u32
    R.off_observed = R.off_held + stream_align((size_t)slots * J * sizeof(uint32_t));           // (slots, W, J) u8
    R.bytes = R.off_observed + stream_align((size_t)slots * R.W * J);
    return R;
}

struct RepairParams { int slots, J, G, W, K, s_in, seq_stride, halves; };

// Joint j of frame f of one slot as the rule of uu3d_repair.h sees it from the frames lo .. newest of the raw ring (frame g at place g % W)
// and the joint's last observation in front of them (last, -1 = none): -> the state (1 observed, 2 filled, 0 neither) and the coordinates
// (zeros for state 0).  lo <= f <= newest.  The fill is resample_mix: the bits of predict.repair_joints_host.
__device__ __forceinline__ int live_repair_joint(const float* __restrict__ raw, const uint8_t* __restrict__ observed, const int last,
                                                 const float2 last_xy, const int W, const int J, const int j, const int f, const int lo,
                                                 const int newest, const int G, float2& out)
{
    if (observed[(f % W) * J + j] != 0) {
        out = *reinterpret_cast<const float2*>(raw + ((size_t)(f % W) * J + j) * 2);
        return 1;
    }
    out = make_float2(0.f, 0.f);
    int l = last, r = -1;
    float2 a = last_xy, b = make_float2(0.f, 0.f);
    for (int g = f - 1; g >= lo; --g)
        if (observed[(g % W) * J + j] != 0) { l = g; a = *reinterpret_cast<const float2*>(raw + ((size_t)(g % W) * J + j) * 2); break; }
    for (int g = f + 1; g <= newest; ++g)
        if (observed[(g % W) * J + j] != 0) { r = g; b = *reinterpret_cast<const float2*>(raw + ((size_t)(g % W) * J + j) * 2); break; }
    if (l >= 0 && r >= 0) {
        if (r - l - 1 > G) return 0;
        const double w = (double)(f - l) / (double)(r - l);
        out = make_float2(resample_mix(a.x, b.x, w), resample_mix(a.y, b.y, w));
    } else if (r >= 0) {
        if (r - f > G) return 0;
        out = b;
    } else if (l >= 0) {
        if (f - l > G) return 0;
        out = a;
    } else return 0;
    return 2;
}

// The k-th frame a slot whose newest frame is t re-stages, -1 = unused: the multiples of s_in in [max(0, t - G), t], oldest first, then the
// edge frame (the newest multiple of the sequence stride) where it lies in that range and is no multiple of s_in.
__device__ __forceinline__ int live_repair_candidate(const RepairParams& p, const int t, const int k)
{
    const int lo = t > p.G ? t - p.G : 0;
    const int first = (lo + p.s_in - 1) / p.s_in * p.s_in;
    const int count = first <= t ? (t - first) / p.s_in + 1 : 0;
    if (k < count) return first + k * p.s_in;
    const int edge = t / p.seq_stride * p.seq_stride;
    return (k == count && edge >= lo && edge % p.s_in != 0) ? edge : -1;
}

// x << s for s in (-64, 64), negative = a right shift
__device__ __forceinline__ uint64_t live_shift(const uint64_t x, const long s)
{
    if (s >= 64 || s <= -64) return 0;
    return s >= 0 ? x << s : x >> -s;
}

// One wave per slot, lane = joint (j = lane, lane + 64, ...).  kp (T, J, 2) raw, joint_flags (T, J) u8 or nullptr, frames (T): the slot's
// counter = the index t of the frame pushed now (stream_commit_repair_kernel advances it).  Outputs per slot: staged (halves * T * K, J, 2),
// stage_frame (T, K) i32 (-1 unused), stage_valid (T, K) u8, far (T, G) i32 (-1 unused), joint_state (T, J) u8 of frame t.  An inactive
// slot changes nothing of its state, stages zeros and marks every entry unused; its joint_state stays.
static __global__ void __launch_bounds__(64)
stream_repair_stage_kernel(const RepairParams p, const float* __restrict__ kp, const double* __restrict__ res, const uint8_t* __restrict__ active,
                           const int32_t* __restrict__ order, const uint8_t* __restrict__ joint_flags, const int32_t* __restrict__ frames,
                           float* raw_all, float* last_xy_all, int32_t* last_all, uint32_t* held_all, uint8_t* observed_all,
                           float* staged, int32_t* __restrict__ stage_frame, uint8_t* __restrict__ stage_valid, int32_t* __restrict__ far,
                           uint8_t* __restrict__ joint_state)
{
    const int slot = blockIdx.x, lane = threadIdx.x;
    const int J = p.J, G = p.G, W = p.W, K = p.K;
    const int t = frames[slot];
    const bool act = active[slot] != 0 && t >= 0 && t < INT32_MAX;                     // (uniform in the workgroup)
    float* raw = raw_all + (size_t)slot * W * J * 2;
    uint8_t* observed = observed_all + (size_t)slot * W * J;
    float* last_xy = last_xy_all + (size_t)slot * J * 2;
    int32_t* last = last_all + (size_t)slot * J;                                        // index + 1
    uint32_t* held = held_all + (size_t)slot * J;
    if (!act) {
        for (int k = lane; k < K; k += 64) { stage_frame[(size_t)slot * K + k] = -1; stage_valid[(size_t)slot * K + k] = 0; }
        for (int i = lane; i < G; i += 64) far[(size_t)slot * G + i] = -1;
        for (int h = 0; h < p.halves; ++h)
            for (int i = lane; i < K * J; i += 64)
                *reinterpret_cast<float2*>(staged + (((size_t)h * p.slots + slot) * K * J + i) * 2) = make_float2(0.f, 0.f);
        return;
    }

    // 1. frame e = t - G - 1 leaves the window: its state under the frames up to t - 1 is final but for the far list.  A joint observed at e
    //    takes e as its last observation; one that is held from its last observation at e notes whether e left as a valid frame.
    const int e = t - G - 1;
    if (e >= 0) {
        bool complete = true, seen = false;
        for (int j = lane; j < J; j += 64) {
            float2 xy;
            const int s = live_repair_joint(raw, observed, last[j] - 1, *reinterpret_cast<const float2*>(last_xy + j * 2), W, J, j, e, e, t - 1, G, xy);
            complete = complete && s != 0;
            seen = seen || s == 1;
        }
        const bool valid_e = __all(complete) != 0 && __any(seen) != 0;
        for (int j = lane; j < J; j += 64) {
            const int l = last[j] - 1;
            if (observed[(e % W) * J + j] != 0) {
                last[j] = e + 1;
                *reinterpret_cast<float2*>(last_xy + j * 2) = *reinterpret_cast<const float2*>(raw + ((size_t)(e % W) * J + j) * 2);
                held[j] = 0;
            } else if (valid_e && l >= 0 && e - l <= G) held[j] |= 1u << (e - l - 1);
        }
    }

    // 2. file the pushed frame (place t % W: the one frame e had)
    for (int j = lane; j < J; j += 64) {
        const float2 x = *reinterpret_cast<const float2*>(kp + ((size_t)slot * J + j) * 2);
        const bool ok = (joint_flags == nullptr || joint_flags[(size_t)slot * J + j] != 0) && finite_pair(x);
        *reinterpret_cast<float2*>(raw + ((size_t)(t % W) * J + j) * 2) = x;
        observed[(t % W) * J + j] = ok ? 1 : 0;
    }

    // 3. the far list: a joint seen at t whose gap is longer than G -- no observation in t - G .. t - 1 and the last one before more than
    //    G + 1 frames back -- turns the frames it was held in missing.  All such frames lie in (l_min, l_min + G], l_min the oldest of
    //    those last observations: a frame further behind a younger one was not valid, the joint of l_min being unfillable there.
    const int lo = t > G ? t - G : 0;
    int l_min = INT32_MAX;
    for (int j = lane; j < J; j += 64) {
        bool closes = observed[(t % W) * J + j] != 0 && last[j] > 0 && t - (last[j] - 1) - 1 > G;
        for (int g = lo; g < t && closes; ++g) closes = observed[(g % W) * J + j] == 0;
        if (closes) l_min = min(l_min, last[j] - 1);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) l_min = min(l_min, __shfl_xor(l_min, d));
    uint32_t far_bits = 0;                                                              // bit i: frame l_min + 1 + i turns missing
    if (l_min != INT32_MAX) {                                                           // (uniform)
        const uint64_t range = G >= 32 ? 0xffffffffull : ((1ull << G) - 1);
        for (int j = lane; j < J; j += 64) {
            bool closes = observed[(t % W) * J + j] != 0 && last[j] > 0 && t - (last[j] - 1) - 1 > G;
            for (int g = lo; g < t && closes; ++g) closes = observed[(g % W) * J + j] == 0;
            if (closes) {
                far_bits |= (uint32_t)(live_shift(held[j], (long)(last[j] - 1) - l_min) & range);
                held[j] = 0;
            }
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) far_bits |= __shfl_xor(far_bits, d);
        for (int j = lane; j < J; j += 64)                                              // those frames are no longer valid for any joint's bits
            if (last[j] > 0) held[j] &= ~(uint32_t)live_shift(far_bits, (long)l_min - (last[j] - 1));
    }
    for (int i = lane; i < G; i += 64) far[(size_t)slot * G + i] = ((far_bits >> i) & 1u) ? l_min + 1 + i : -1;

    // 4. the state of the newest frame, and the K frames to re-stage: normalised where the frame is valid, zeros otherwise
    for (int j = lane; j < J; j += 64) {
        float2 xy;
        joint_state[(size_t)slot * J + j] =
            (uint8_t)live_repair_joint(raw, observed, last[j] - 1, *reinterpret_cast<const float2*>(last_xy + j * 2), W, J, j, t, lo, t, G, xy);
    }
    const float wf = res != nullptr ? (float)res[2 * slot] : 1.f;
    const double h_over_w = res != nullptr ? res[2 * slot + 1] / res[2 * slot] : 1.0;
    for (int k = 0; k < K; ++k) {
        const int f = live_repair_candidate(p, t, k);                                  // (uniform)
        float* plain = staged + ((size_t)slot * K + k) * J * 2;
        bool valid = false;
        if (f >= 0) {
            bool complete = true, seen = false;
            for (int j = lane; j < J; j += 64) {
                float2 xy;
                const int s = live_repair_joint(raw, observed, last[j] - 1, *reinterpret_cast<const float2*>(last_xy + j * 2), W, J, j, f, lo, t, G, xy);
                complete = complete && s != 0;
                seen = seen || s == 1;
                *reinterpret_cast<float2*>(plain + j * 2) = res != nullptr ? normalize_pair(xy, wf, h_over_w) : xy;
            }
            valid = __all(complete) != 0 && __any(seen) != 0;
        }
        if (!valid)
            for (int j = lane; j < J; j += 64) *reinterpret_cast<float2*>(plain + j * 2) = make_float2(0.f, 0.f);
        if (lane == 0) { stage_frame[(size_t)slot * K + k] = f; stage_valid[(size_t)slot * K + k] = valid ? 1 : 0; }
        if (p.halves > 1) {
            __syncthreads();                                                            // the plain copy is written: other lanes read it
            float* flipped = staged + (((size_t)p.slots + slot) * K + k) * J * 2;
            for (int j = lane; j < J; j += 64) {
                float2 v = make_float2(0.f, 0.f);
                if (valid) {
                    const int js = order[j];
                    if (js < 0 || js >= J) v = make_float2(__builtin_nanf(""), __builtin_nanf(""));
                    else { v = *reinterpret_cast<const float2*>(plain + js * 2); v.x = -v.x; }
                }
                *reinterpret_cast<float2*>(flipped + j * 2) = v;
            }
        }
    }
}

// stream_commit_kernel for a session with repair_joints: feats (halves * T * K, d_t) are the features of the staged frames.  Frame f of
// entry k is filed, features and valid byte, in ring place (f / s_in) % cap where that place still holds f -- f is a multiple of s_in and
// f > newest - cap * s_in -- and as the edge row where f is the edge frame of the newest frame; the far list clears the valid bytes of the
// places that still hold its frames.  No two entries share a place: two frames of one place lie cap * s_in apart and only the younger is
// still held.  Then the window of the tick, stream_commit_kernel's own (stream_write_window).
static __global__ void __launch_bounds__(256)
stream_commit_repair_kernel(const StreamParams p, const int K, const int G, const float* __restrict__ feats, const uint8_t* __restrict__ active,
                            int32_t* __restrict__ frames, float* __restrict__ table, const int32_t* __restrict__ stage_frame,
                            const uint8_t* __restrict__ stage_valid, const int32_t* __restrict__ far, int32_t* __restrict__ rows,
                            uint8_t* __restrict__ stride_mask, uint8_t* __restrict__ fresh, uint8_t* valid_state)
{
    const int slot = blockIdx.x, tid = threadIdx.x;
    const int before = frames[slot];
    const bool act = active[slot] != 0 && before >= 0 && before < INT32_MAX;
    __syncthreads();                                                     // every read of the counter is done
    const int len = before + (act ? 1 : 0);
    if (tid == 0 && act) frames[slot] = len;
    if (act) {
        const int edge_frame = before / p.seq_stride * p.seq_stride;
        const long oldest_held = (long)before - (long)p.cap * p.s_in;    // a multiple of s_in is still in its ring place iff it is younger
        const int q = p.dt / 4;
        for (int i = tid; i < K * p.halves * q; i += 256) {
            const int k = i / (p.halves * q), half = (i - k * p.halves * q) / q, c = (i - (k * p.halves + half) * q) * 4;
            const int f = stage_frame[(size_t)slot * K + k];
            if (f < 0 || f > before) continue;
            const float4 v = *reinterpret_cast<const float4*>(feats + (((size_t)half * p.slots + slot) * K + k) * p.dt + c);
            if (f == edge_frame) *reinterpret_cast<float4*>(table + (size_t)stream_edge_row(p, half, slot) * p.dt + c) = v;
            if (f % p.s_in == 0 && f > oldest_held) *reinterpret_cast<float4*>(table + (size_t)stream_ring_row(p, half, slot, f) * p.dt + c) = v;
        }
        for (int i = tid; i < K + G; i += 256) {                          // the valid bytes: the staged frames' own, 0 for the far list
            const bool staged_entry = i < K;
            const int f = staged_entry ? stage_frame[(size_t)slot * K + i] : far[(size_t)slot * G + (i - K)];
            if (f < 0 || f > before) continue;
            const uint8_t b = staged_entry && stage_valid[(size_t)slot * K + i] != 0 ? 1 : 0;
            if (f == edge_frame) valid_state[stream_edge_row(p, 0, slot)] = b;
            if (f % p.s_in == 0 && f > oldest_held) valid_state[stream_ring_row(p, 0, slot, f)] = b;
        }
    }
    __syncthreads();                                                     // the bytes filed above are read below by other threads
    stream_write_window(p, slot, tid, len, act, 0, valid_state, rows, stride_mask, fresh);
}

// slot_mask (T) u8 or nullptr (every slot): the chosen slots forget their last observations and held-frame bits.  The raw ring stays: no
// frame in front of a slot's counter is ever read.
static __global__ void __launch_bounds__(256)
stream_repair_reset_kernel(const uint8_t* __restrict__ slot_mask, const int T, const int J, int32_t* __restrict__ last, uint32_t* __restrict__ held)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)T * J) return;
    if (slot_mask != nullptr && slot_mask[i / J] == 0) return;
    last[i] = 0;
    held[i] = 0;
}

}  // namespace uu3d
