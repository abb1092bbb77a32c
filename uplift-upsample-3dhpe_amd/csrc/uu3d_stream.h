// uu3d_stream.h -- live uplifting (stream.StreamSession; include/uu3d.h, "LIVE TRACKS"): one frame of 2D keypoints per slot and tick in,
// the pose of frame `newest - lookahead` out.  Four small kernels around uu3d_frame_features and uu3d_forward_frames_ex:
//   stream_stage_kernel   pushed pixel frames -> normalised frames and their mirrored copies (normalize_pair of uu3d_tracks.h)
//   stream_commit_kernel  per slot: advance the frame counter, file the new frame's features (edge row, keyframe ring), write this tick's
//                         window as feature-table rows and stride masks (stream_write_window, shared with uu3d_stream_repair.h; window_frame
//                         of uu3d_misc.h: the one statement of the rules)
//   stream_emit_kernel    un-flip / average (window_prediction of uu3d_tracks.h), root shift, fresh slots written, the others held
//   stream_reset_kernel   chosen slots back to zero frames and a zero held pose
// All per-slot state sits in one caller-allocated block (StreamLayout).  No atomics, every output element has one writer, the counters are
// read and advanced on the device: the launches of a tick have the same arguments at every tick and replay from one captured graph.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "uu3d_misc.h"
#include "uu3d_tracks.h"

namespace uu3d {

// The feature table of a session, (rows, d_t) float32: per half (plain, then flipped when flip is on) and slot `cap + 1` rows -- the ring
// of the slot's keyframes (frame k * s_in in ring place k % cap) and, last, its edge row (the newest frame whose index is a multiple of
// the sequence stride: what copy padding behind the end repeats) -- and one last row for the features of an all-zero frame.
//   cap = (lookahead + (N / 2) * seq_stride) / s_in + 1: a window centred on c = newest - lookahead reads frames c - (N / 2) * seq_stride
//   .. newest, lookahead + (N / 2) * seq_stride + 1 consecutive indices, which hold at most `cap` multiples of s_in, and `cap`
//   consecutive multiples never share a ring place.
struct StreamLayout {
    int slots, halves, cap, dt, per_pose;      // per_pose = J * 3
    long table_rows, zero_row;
    size_t off_frames, off_held, off_table, bytes;
};
inline size_t stream_align(size_t v) { return (v + 255) / 256 * 256; }
inline StreamLayout stream_layout(int slots, int N, int J, int dt, int seq_stride, int s_in, int lookahead, int flip)
{
    StreamLayout L{};
    L.slots = slots; L.halves = flip ? 2 : 1; L.dt = dt; L.per_pose = J * 3;
    L.cap = (lookahead + (N / 2) * seq_stride) / s_in + 1;
    L.zero_row = (long)L.halves * slots * (L.cap + 1);
    L.table_rows = L.zero_row + 1;
    L.off_frames = 0;
    L.off_held = stream_align((size_t)slots * sizeof(int32_t));
    L.off_table = L.off_held + stream_align((size_t)slots * L.per_pose * sizeof(float));
    L.bytes = L.off_table + stream_align((size_t)L.table_rows * dt * sizeof(float));
    return L;
}

// What the commit kernel needs to know about the session (passed by value).
struct StreamParams {
    int slots, N, dt, seq_stride, s_in, pred_stride, lookahead, cap, halves, pad_edge;
    int masked_row;        // the row of a token the stride mask drops: -1 (the forward writes the masked token) or the zero row (no strided input)
    int zero_row;
};
__device__ __forceinline__ int stream_ring_row(const StreamParams& p, const int half, const int slot, const int frame)
{
    return (half * p.slots + slot) * (p.cap + 1) + (frame / p.s_in) % p.cap;
}
__device__ __forceinline__ int stream_edge_row(const StreamParams& p, const int half, const int slot)
{
    return (half * p.slots + slot) * (p.cap + 1) + p.cap;
}

// kp (T, J, 2) pixel (or already normalised: res == nullptr) coordinates of this tick -> out (halves * T, J, 2): the normalised frames and,
// behind them, their mirrored copies (joints permuted by `order`, x negated -- gather_windows_kernel's flip).  An inactive slot's frames
// are zeros.  One thread per two (x, y) pairs = one 16-byte store.
// MISSED DETECTIONS (valid_out != nullptr): valid_out[slot] = active && valid_in[slot] (nullptr: 1) && all 2 J coordinates of the slot's row
// are finite; a slot whose frame is missing stages zeros in both halves, like an inactive one.  Every thread re-reads its slot's row of kp
// (which nobody writes); the thread of joint 0 of the plain half writes the slot's byte.
static __global__ void __launch_bounds__(256)
stream_stage_kernel(const float* __restrict__ kp, const double* __restrict__ res, const uint8_t* __restrict__ active,
                    const int32_t* __restrict__ order, const int T, const int J, const int halves, const uint8_t* __restrict__ valid_in,
                    uint8_t* __restrict__ valid_out, float* __restrict__ out)
{
    const long pairs = (long)halves * T * J;
    const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * 2;
    if (p0 >= pairs) return;
    float2 v[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const long p = (p0 + e < pairs) ? p0 + e : p0;
        const int row = (int)(p / J), j = (int)(p - (long)row * J);
        const int half = row / T, t = row - half * T;
        v[e] = make_float2(0.f, 0.f);
        bool real = active[t] != 0;
        if (valid_out != nullptr) {
            real = real && (valid_in == nullptr || valid_in[t] != 0);
            for (int k = 0; k < J && real; ++k) real = finite_pair(*reinterpret_cast<const float2*>(kp + ((long)t * J + k) * 2));
            if (p == p0 + e && half == 0 && j == 0) valid_out[t] = real ? 1 : 0;
        }
        if (!real) continue;
        int js = j;
        if (half != 0) { js = order[j]; if (js < 0 || js >= J) { v[e] = make_float2(__builtin_nanf(""), __builtin_nanf("")); continue; } }
        const float2 x = *reinterpret_cast<const float2*>(kp + ((long)t * J + js) * 2);
        float2 n = (res != nullptr) ? normalize_pair(x, (float)res[2 * t], res[2 * t + 1] / res[2 * t]) : x;
        if (half != 0) n.x = -n.x;
        v[e] = n;
    }
    if (p0 + 1 < pairs) *reinterpret_cast<float4*>(out + p0 * 2) = make_float4(v[0].x, v[0].y, v[1].x, v[1].y);
    else *reinterpret_cast<float2*>(out + p0 * 2) = v[0];
}

// The window of a tick, for stream_commit_kernel, stream_commit_repair_kernel (uu3d_stream_repair.h) and stream_drain_commit_kernel
// (uu3d_stream_drain.h): slot `slot` has `len` frames after this tick (act: it took one).  Writes the slot's rows (halves, N), stride masks
// and fresh byte; valid_state as in stream_commit_kernel.  centre_offset: 0 for a push; a drain tick moves the centre that many frames
// towards the newest frame (0 <= centre_offset <= lookahead, so no frame older than the ring's oldest is read) while `len` stays.
__device__ __forceinline__ void stream_write_window(const StreamParams& p, const int slot, const int tid, const int len, const bool act,
                                                    const int centre_offset, const uint8_t* valid_state, int32_t* __restrict__ rows,
                                                    uint8_t* __restrict__ stride_mask, uint8_t* __restrict__ fresh)
{
    const int centre = len - 1 - p.lookahead + centre_offset;
    const bool is_fresh = act && centre >= 0 && centre % p.pred_stride == 0;
    if (tid == 0) fresh[slot] = is_fresh ? 1 : 0;
    const int oldest = centre - (p.N / 2) * p.seq_stride;               // nothing older is still in the ring for certain
    for (int i = tid; i < p.halves * p.N; i += 256) {
        const int half = i / p.N, n = i - half * p.N;
        const size_t o = ((size_t)half * p.slots + slot) * p.N + n;
        int r = p.masked_row;
        uint8_t sm = 0;
        if (is_fresh) {                                                  // (a slot that is not fresh: an all-masked window, finite and discarded)
            const WindowDesc d{0, centre, p.seq_stride, p.s_in, centre, half};
            const WindowFrame t = window_frame(d, len, p.N, n, p.pad_edge);
            int place = -1;                                              // where the frame the token reads is kept, in half 0 of the table
            if (t.sm && t.have) {
                if (!t.inside && t.src == (len - 1) / p.seq_stride * p.seq_stride) place = stream_edge_row(p, 0, slot);
                else if (t.src % p.s_in == 0 && t.src >= oldest && t.src >= 0 && t.src < len) place = stream_ring_row(p, 0, slot, t.src);
            }
            const bool real = window_token_real(t, place >= 0 ? valid_state : nullptr, place);
            sm = real ? 1 : 0;
            if (!real) r = p.masked_row;
            else if (!t.have) r = p.zero_row;
            else if (place >= 0) r = place + half * p.slots * (p.cap + 1);
            else r = -1;                                                 // no such frame is kept: NaN in the forward, reported by its range check
        }
        rows[o] = r;
        stride_mask[o] = sm;
    }
}

// One workgroup per slot.  feats (halves * T, d_t): the features of this tick's staged frames.  The slot's counter is read by every
// thread of ITS workgroup only, and written by one of them behind a barrier.  Rows written: rows (halves * T, N), stride_mask likewise,
// fresh (T).  The window is the one uu3d_gather_window_frames writes for a video of `frames` frames centred on frames - 1 - lookahead with
// a globally aligned mask; only where its frames live differs (ring place / edge row instead of video_start + frame).
// MISSED DETECTIONS (valid_state != nullptr): valid (T) u8 says whether this tick's frame of a slot is a real observation (stream_stage_kernel's
// valid_out); valid_state (T, cap + 1) u8 keeps that byte per ring place and for the edge row, filed where the features are filed, the same
// for both halves.  A missing frame advances the counter like any other (time passes) and the window applies window_token_real with the
// byte of the place it points to.
static __global__ void __launch_bounds__(256)
stream_commit_kernel(const StreamParams p, const float* __restrict__ feats, const uint8_t* __restrict__ active, int32_t* __restrict__ frames,
                     float* __restrict__ table, int32_t* __restrict__ rows, uint8_t* __restrict__ stride_mask, uint8_t* __restrict__ fresh,
                     const uint8_t* __restrict__ valid, uint8_t* valid_state)
{
    const int slot = blockIdx.x, tid = threadIdx.x;
    const int before = frames[slot];
    const bool act = active[slot] != 0 && before >= 0 && before < INT32_MAX;
    __syncthreads();                                                     // every read of the counter is done
    const int len = before + (act ? 1 : 0);
    if (tid == 0 && act) frames[slot] = len;
    if (act) {                                                           // file the new frame (index `before`)
        const bool edge = before % p.seq_stride == 0, key = before % p.s_in == 0;
        const int q = p.dt / 4;
        for (int i = tid; i < p.halves * q; i += 256) {
            const int half = i / q, c = (i - half * q) * 4;
            const float4 v = *reinterpret_cast<const float4*>(feats + ((size_t)half * p.slots + slot) * p.dt + c);
            if (edge) *reinterpret_cast<float4*>(table + (size_t)stream_edge_row(p, half, slot) * p.dt + c) = v;
            if (key) *reinterpret_cast<float4*>(table + (size_t)stream_ring_row(p, half, slot, before) * p.dt + c) = v;
        }
        if (valid_state != nullptr && tid == 0) {                        // (stream_ring_row / stream_edge_row of half 0 and `slot` = the slot's (cap + 1) bytes)
            const uint8_t b = valid[slot] != 0 ? 1 : 0;
            if (edge) valid_state[stream_edge_row(p, 0, slot)] = b;
            if (key) valid_state[stream_ring_row(p, 0, slot, before)] = b;
        }
    }
    if (valid_state != nullptr) __syncthreads();                         // (uniform: the bytes filed above are read below by other threads)
    stream_write_window(p, slot, tid, len, act, 0, valid_state, rows, stride_mask, fresh);
}

// central (halves * T, J, 3): the forward's central predictions of this tick's windows.  out (T, J, 3) and held (T, J, 3, in the state
// block): a fresh slot takes its new pose (the flipped half un-flipped and averaged in, the root joint subtracted when root >= 0), any other
// slot its held one.  One thread per four consecutive floats.
static __global__ void __launch_bounds__(256)
stream_emit_kernel(const float* __restrict__ central, const int halves, const int32_t* __restrict__ order, const uint8_t* __restrict__ fresh,
                   const int T, const int J, const int root, float* __restrict__ held, float* __restrict__ out)
{
    const long per = (long)J * 3, total = (long)T * per;
    const long e0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (e0 >= total) return;
    const float* flipped = halves > 1 ? central + total : nullptr;
    float v[4];
    bool any_fresh = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long e = (e0 + k < total) ? e0 + k : e0;
        const long t = e / per;
        const int r = (int)(e - t * per), j = r / 3, c = r - j * 3;
        if (fresh[t] != 0) {
            any_fresh = true;
            v[k] = window_prediction(central, flipped, order, t, J, j, c);
            if (root >= 0) v[k] = v[k] - window_prediction(central, flipped, order, t, J, root, c);
        } else v[k] = held[e];
    }
    if (e0 + 4 <= total) {
        *reinterpret_cast<float4*>(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
        if (any_fresh) *reinterpret_cast<float4*>(held + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else for (int k = 0; e0 + k < total; ++k) { out[e0 + k] = v[k]; if (any_fresh) held[e0 + k] = v[k]; }
}

// slot_mask (T) u8 or nullptr (every slot): the chosen slots start again at zero frames with a zero held pose.  Ring and edge rows stay as
// they are: a window never reads a frame its slot's counter has not reached.
static __global__ void __launch_bounds__(256)
stream_reset_kernel(const uint8_t* __restrict__ slot_mask, const int T, const int per_pose, int32_t* __restrict__ frames, float* __restrict__ held)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)T * per_pose) return;
    const int t = (int)(i / per_pose);
    if (slot_mask != nullptr && slot_mask[t] == 0) return;
    held[i] = 0.f;
    if (i - (long)t * per_pose == 0) frames[t] = 0;
}

}  // namespace uu3d
