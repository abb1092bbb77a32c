// uu3d_stream_rate.h -- live tracks at any frame rate (stream.StreamSession(fps=F); include/uu3d.h, "LIVE TRACKS AT ANY FRAME RATE"): one
// SOURCE frame per slot and push in, one pose per slot and push out at the source frame's own time.  With model_fps / fps = a / b in lowest
// terms, model frame k sits at source position k b / a (predict.resample_plan) and is made in the sub-tick after source frame
// ceil(k b / a) was pushed; a sub-tick is the plain session's tick with its stage replaced:
//   stream_source_push_kernel     per slot: advance the source counter, file the raw frame (and its validity byte) in the two-frame ring
//   stream_resample_stage_kernel  per slot: is model frame frames[slot] due?  then the normalised, mixed frame and its mirrored copy
//                                 (normalize_pair / resample_mix of uu3d_tracks.h) and sub_active = 1, else zeros and sub_active = 0
//   stream_file_keyframe_kernel   after stream_emit_kernel: a fresh central pose into the slot's keyframe ring, place (centre / P) % D
//   stream_timed_emit_kernel      once per push: the pose of source frame q = newest - lookahead, read at model position q a / b from the
//                                 piecewise-linear motion through the kept keyframes (evaluation.keyframe_plan_at's rule)
// and, for a session with an output rate of its own (StreamSession(fps=F, out_fps=G)), in place of stream_timed_emit_kernel:
//   stream_timed_emit_multi_kernel  once per push: EVERY output frame that became due at this push, up to R = ceil(G / F) poses per slot
// Both read a pose from the kept keyframes with keyframe_read.  A session with interpolation="cubic" launches
//   stream_timed_emit_cubic_kernel / stream_timed_emit_multi_cubic_kernel
// in their places: the same launches reading through keyframe_read_cubic, the C1 cubic through four kept keyframes.  For either kind of session:
//   stream_rate_reset_kernel      chosen slots: every counter 0 (model, source, output), both held poses 0
// The new state lies behind the plain session's (StreamLayout) in the same caller-allocated block.  No atomics, one writer per output
// element, every counter is read and advanced on the device, all arguments are the same at every push: a sub-tick in which no slot is due
// changes no byte of the state and none of the outputs of the push.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "uu3d_stream.h"
#include "uu3d_tracks.h"

namespace uu3d {

// Behind StreamLayout::bytes: source counters (T) i32; pushed (T) u8 = the slot took a frame at this push; source validity (T, 2) u8 and
// the raw source frames (T, 2, J, 2) f32, frame i of a slot in place i & 1; the keyframe ring (T, D, key_stride) f32, key_stride = J * 3
// rounded up to four floats so that every kept pose starts on 16 bytes; the held output poses (T, J * 3) f32.
struct RateLayout {
    int key_ring, key_stride;
    size_t off_source_frames, off_pushed, off_source_valid, off_source, off_keys, off_out_held, bytes;
};
inline RateLayout rate_layout(const StreamLayout& L, const int J, const int key_ring)
{
    RateLayout R{};
    const size_t T = (size_t)L.slots;
    R.key_ring = key_ring;
    R.key_stride = (L.per_pose + 3) / 4 * 4;
    R.off_source_frames = L.bytes;
    R.off_pushed = R.off_source_frames + stream_align(T * sizeof(int32_t));
    R.off_source_valid = R.off_pushed + stream_align(T);
    R.off_source = R.off_source_valid + stream_align(T * 2);
    R.off_keys = R.off_source + stream_align(T * 2 * J * 2 * sizeof(float));
    R.off_out_held = R.off_keys + stream_align(T * key_ring * R.key_stride * sizeof(float));
    R.bytes = R.off_out_held + stream_align(T * L.per_pose * sizeof(float));
    return R;
}

// Behind RateLayout::bytes, for a session with an output rate of its own: the output counters (T) i32.
inline size_t out_frames_offset(const RateLayout& R) { return R.bytes; }
inline size_t out_layout_bytes(const RateLayout& R, const int slots) { return R.bytes + stream_align((size_t)slots * sizeof(int32_t)); }

struct RateParams {
    int slots, J, halves, per_pose;
    int a, b;              // model_fps / fps in lowest terms; both below 2^20, so every product with a 31-bit counter fits int64 (and float64)
    int lookahead;         // of the session, in SOURCE frames
    int model_lookahead;   // a_m: the lookahead of the sub-ticks, in model frames
    int pred_stride, key_ring, key_stride;
};

// One workgroup of one wave per slot (the slot's counter is read by ITS wave only and written by lane 0 behind a barrier, as
// stream_commit_kernel does).  kp (T, J, 2): the raw frames of this push.  An active slot's frame gets source index `count` and ring place
// count & 1; its validity byte = valid_in (nullptr: 1) && all 2 J coordinates finite -- uu3d_resample_tracks' test of a source row -- when
// track_valid, else 1.  pushed[slot] says whether the slot took a frame.  The two frames of a slot's ring are 8-byte aligned only (J pairs
// each) and neighbouring slots sit in different places: 8-byte stores, one (x, y) pair per lane.
static __global__ void __launch_bounds__(64)
stream_source_push_kernel(const float* __restrict__ kp, const uint8_t* __restrict__ active, const uint8_t* __restrict__ valid_in, const int track_valid,
                          const int J, int32_t* __restrict__ source_frames, uint8_t* __restrict__ pushed, uint8_t* __restrict__ source_valid,
                          float* __restrict__ source)
{
    const int slot = blockIdx.x, lane = threadIdx.x;
    const int count = source_frames[slot];
    const bool act = active[slot] != 0 && count >= 0 && count < INT32_MAX;
    __syncthreads();                                                     // every read of the counter is done
    if (lane == 0) { pushed[slot] = act ? 1 : 0; if (act) source_frames[slot] = count + 1; }
    if (!act) return;                                                    // (uniform in the workgroup)
    const int place = count & 1;
    bool ok = true;
    for (int j = lane; j < J; j += 64) {
        const float2 x = *reinterpret_cast<const float2*>(kp + ((long)slot * J + j) * 2);
        ok = ok && finite_pair(x);
        *reinterpret_cast<float2*>(source + (((long)slot * 2 + place) * J + j) * 2) = x;
    }
    ok = __all(ok) != 0 && (valid_in == nullptr || valid_in[slot] != 0);
    if (lane == 0) source_valid[slot * 2 + place] = (!track_valid || ok) ? 1 : 0;
}

// Which model frame a slot makes in this sub-tick, if any: frame k = frames[slot] (the model counter: the frames made so far) lies at
// source position k b / a between source frames l and r = l + (rem > 0); it is due once r has been pushed.  `gone`: l has already left the
// two-frame ring -- impossible while every push is followed by at least ceil(a / b) sub-ticks; such a frame is staged as NaN and the
// forward's range check reports it.
struct RateDue { bool due, gone; long l, r, rem; };
__device__ __forceinline__ RateDue rate_due(const int source_count, const int model_count, const int a, const int b)
{
    RateDue d{false, false, 0, 0, 0};
    if (source_count < 1 || model_count < 0 || model_count == INT32_MAX) return d;
    const long pos = (long)model_count * b;
    d.l = pos / a;
    d.rem = pos - d.l * a;
    d.r = d.l + (d.rem > 0 ? 1 : 0);
    d.due = d.r <= (long)source_count - 1;
    d.gone = d.due && d.l < (long)source_count - 2;
    return d;
}

// out (halves * T, J, 2) as stream_stage_kernel writes it, from the slots' source rings: where the position is whole the source frame's
// (normalised) bits, else its two neighbours normalised and then mixed in float64 with weight (double) rem / (double) a -- the double
// predict.resample_plan computes.  sub_active[slot] = the slot makes a model frame in this sub-tick: the `active` of the rest of the tick.
// valid_out (nullptr: no missed detections): that frame is a real observation = its left source frame is valid and, where it is mixed from
// two, its right one too (resample_valid_kernel's rule); a missing frame stages zeros in both halves.  A slot that is not due stages
// zeros, like an inactive slot of stream_stage_kernel.  Nothing this kernel reads is written by it; the thread of joint 0 of the plain
// half writes the slot's bytes.  One thread per two (x, y) pairs = one 16-byte store.
static __global__ void __launch_bounds__(256)
stream_resample_stage_kernel(const RateParams p, const int32_t* __restrict__ source_frames, const int32_t* __restrict__ frames,
                             const uint8_t* __restrict__ source_valid, const float* __restrict__ source, const double* __restrict__ res,
                             const int32_t* __restrict__ order, uint8_t* __restrict__ sub_active, uint8_t* __restrict__ valid_out,
                             float* __restrict__ out)
{
    const int T = p.slots, J = p.J;
    const long pairs = (long)p.halves * T * J;
    const long p0 = ((long)blockIdx.x * 256 + threadIdx.x) * 2;
    if (p0 >= pairs) return;
    float2 v[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const long q = (p0 + e < pairs) ? p0 + e : p0;
        const int row = (int)(q / J), j = (int)(q - (long)row * J);
        const int half = row / T, t = row - half * T;
        v[e] = make_float2(0.f, 0.f);
        const RateDue d = rate_due(source_frames[t], frames[t], p.a, p.b);
        bool real = d.due;
        if (valid_out != nullptr && d.due && !d.gone)
            real = source_valid[t * 2 + (int)(d.l & 1)] != 0 && (d.rem == 0 || source_valid[t * 2 + (int)(d.r & 1)] != 0);
        if (q == p0 + e && half == 0 && j == 0) {
            sub_active[t] = d.due ? 1 : 0;
            if (valid_out != nullptr) valid_out[t] = real ? 1 : 0;
        }
        if (!real) continue;
        int js = j;
        if (half != 0) js = order[j];
        if (d.gone || js < 0 || js >= J) { v[e] = make_float2(__builtin_nanf(""), __builtin_nanf("")); continue; }
        const bool normalise = res != nullptr;
        const float wf = normalise ? (float)res[2 * t] : 1.0f;
        const double h_over_w = normalise ? res[2 * t + 1] / res[2 * t] : 1.0;
        float2 n = resample_source_pair(source, (long)t * 2 + (d.l & 1), J, js, normalise, wf, h_over_w);
        if (d.rem > 0) {
            const float2 b = resample_source_pair(source, (long)t * 2 + (d.r & 1), J, js, normalise, wf, h_over_w);
            const double w = (double)d.rem / (double)p.a;
            n = make_float2(resample_mix(n.x, b.x, w), resample_mix(n.y, b.y, w));
        }
        if (half != 0) n.x = -n.x;
        v[e] = n;
    }
    if (p0 + 1 < pairs) *reinterpret_cast<float4*>(out + p0 * 2) = make_float4(v[0].x, v[0].y, v[1].x, v[1].y);
    else *reinterpret_cast<float2*>(out + p0 * 2) = v[0];
}

// After stream_emit_kernel: held (T, J * 3) holds the pose a fresh slot has just emitted, of centre frames[slot] - 1 - model_lookahead (a
// multiple of the prediction stride P).  It is filed in the slot's keyframe ring, place (centre / P) % D.  One thread per four floats of a
// kept pose = one 16-byte store (the floats behind J * 3 are zeros).
static __global__ void __launch_bounds__(256)
stream_file_keyframe_kernel(const RateParams p, const int32_t* __restrict__ frames, const uint8_t* __restrict__ fresh, const float* __restrict__ held,
                            float* __restrict__ keys)
{
    const int quads = p.key_stride / 4;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)p.slots * quads) return;
    const int t = (int)(i / quads), c = (int)(i - (long)t * quads) * 4;
    if (fresh[t] == 0) return;
    const int centre = frames[t] - 1 - p.model_lookahead;
    if (centre < 0) return;
    const int place = (centre / p.pred_stride) % p.key_ring;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (c + k < p.per_pose) ? held[(long)t * p.per_pose + c + k] : 0.f;
    *reinterpret_cast<float4*>(keys + ((long)t * p.key_ring + place) * p.key_stride + c) = make_float4(v[0], v[1], v[2], v[3]);
}

// Column `col` of a slot's pose at model position u = num / den, read from the slot's keyframe ring (`ring`: its first float) through the
// piecewise-linear motion through the kept keyframes, P model frames apart (rates.keyframe_bracket on the host): k0 = floor(u / P) P;
// u == k0 gives keyframe k0's bits, anything else resample_mix(k0, k0 + P, w) -- float64, rounded once to float32 -- with
// w = (num - k0 den) / (P den), one float64 division of two integers (keyframe_plan_at's weight).  The place is taken modulo the ring.
__device__ __forceinline__ float keyframe_read(const float* __restrict__ ring, const int key_ring, const int key_stride, const long P, const long num,
                                               const long den, const int col)
{
    const long k0 = num / den / P * P;
    const long off = num - k0 * den;                                      // (u - k0) den, in [0, P den)
    const float a = ring[(k0 / P) % key_ring * key_stride + col];
    if (off == 0) return a;
    const float b = ring[(k0 / P + 1) % key_ring * key_stride + col];
    return resample_mix(a, b, (double)off / (double)(P * den));
}

// Once per push, behind its sub-ticks.  A slot that took a frame at this push (pushed) and whose q = newest source frame - lookahead is
// >= 0 gets the pose at model position u = q a / b (keyframe_read).  The host's plan (rates.rate_plan) guarantees that both keyframes have
// been emitted and are still in the ring.  Any other slot keeps its held pose; fresh_out says which is which.  out (T, J * 3) and
// out_held likewise: one thread per four consecutive floats, as stream_emit_kernel.
static __global__ void __launch_bounds__(256)
stream_timed_emit_kernel(const RateParams p, const int32_t* __restrict__ source_frames, const uint8_t* __restrict__ pushed,
                         const float* __restrict__ keys, float* __restrict__ out_held, float* __restrict__ out, uint8_t* __restrict__ fresh_out)
{
    const long per = p.per_pose, total = (long)p.slots * per;
    const long e0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (e0 >= total) return;
    float v[4];
    bool any_fresh = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long e = (e0 + k < total) ? e0 + k : e0;
        const long t = e / per;
        const int r = (int)(e - t * per);
        const long q = (long)source_frames[t] - 1 - p.lookahead;
        const bool is_fresh = pushed[t] != 0 && q >= 0;
        if (e == e0 + k && r == 0) fresh_out[t] = is_fresh ? 1 : 0;
        if (!is_fresh) { v[k] = out_held[e]; continue; }
        any_fresh = true;
        v[k] = keyframe_read(keys + t * p.key_ring * p.key_stride, p.key_ring, p.key_stride, p.pred_stride, q * p.a, p.b, r);
    }
    if (e0 + 4 <= total) {
        *reinterpret_cast<float4*>(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
        if (any_fresh) *reinterpret_cast<float4*>(out_held + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else for (int k = 0; e0 + k < total; ++k) { out[e0 + k] = v[k]; if (any_fresh) out_held[e0 + k] = v[k]; }
}

// The output rate of a session, next to RateParams: G / F = c / d and model_fps / G = un / ud, both in lowest terms with terms below 2^20
// (every product with a 31-bit counter fits int64); max_out = R = ceil(c / d), the most poses one push returns.
struct OutParams { int c, d, un, ud, max_out; };

// Once per push, behind its sub-ticks, in place of stream_timed_emit_kernel.  One workgroup per slot: the slot's output counter is read by
// that workgroup only and advanced by lane 0 behind a barrier (the discipline of stream_source_push_kernel).  A slot that took a frame
// at this push and whose q = newest source frame - lookahead is >= 0 has, after the push, emitted every output frame i <= hi =
// floor(q c / d): the frames whose time i / G is not later than q / F.  n = hi + 1 - out_frames[slot], clamped to [0, R], of them are new;
// any other slot has n = 0.  Row r < n of poses (T, R, J * 3) is output frame i = out_frames[slot] + r, read at model position
// u = i un / ud (keyframe_read).  The host's plan (rates.rate_plan) guarantees that both keyframes of every due frame have been emitted
// and are still in the ring; the place is taken modulo the ring whatever the counters hold.  Rows r >= n are zeros; count[slot] = n.  The counter stops at INT32_MAX instead of wrapping.
// A slot's R rows are R * J * 3 consecutive floats, 16-byte aligned only where slot * R * J * 3 is a multiple of four: the workgroup walks
// the 16-byte quads of poses that overlap its rows, stores a quad that lies wholly inside them at once and the floats of a quad it shares
// with a neighbouring slot one by one -- every element has one writer.
static __global__ void __launch_bounds__(256)
stream_timed_emit_multi_kernel(const RateParams p, const OutParams o, const int32_t* __restrict__ source_frames, const uint8_t* __restrict__ pushed,
                               const float* __restrict__ keys, int32_t* __restrict__ out_frames, float* __restrict__ poses, int32_t* __restrict__ count)
{
    const int slot = blockIdx.x;
    const long done = out_frames[slot];
    const long q = (long)source_frames[slot] - 1 - p.lookahead;
    long n = 0;
    if (pushed[slot] != 0 && q >= 0 && done >= 0) {
        n = q * o.c / o.d + 1 - done;
        n = n < 0 ? 0 : (n > o.max_out ? o.max_out : n);
        if (n > (long)INT32_MAX - done) n = (long)INT32_MAX - done;
    }
    __syncthreads();                                                     // every read of the counter is done
    if (threadIdx.x == 0) { out_frames[slot] = (int32_t)(done + n); count[slot] = (int32_t)n; }
    const long per = p.per_pose;
    const long start = (long)slot * o.max_out * per, end = start + (long)o.max_out * per;
    const float* ring = keys + (long)slot * p.key_ring * p.key_stride;
    for (long quad = start / 4 + threadIdx.x; quad * 4 < end; quad += 256) {
        const long e0 = quad * 4;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = 0.f;
            const long rel = e0 + k - start;
            if (rel < 0 || e0 + k >= end) continue;
            const long r = rel / per;
            if (r >= n) continue;
            v[k] = keyframe_read(ring, p.key_ring, p.key_stride, p.pred_stride, (done + r) * o.un, o.ud, (int)(rel - r * per));
        }
        if (e0 >= start && e0 + 4 <= end) *reinterpret_cast<float4*>(poses + e0) = make_float4(v[0], v[1], v[2], v[3]);
        else for (int k = 0; k < 4; ++k) if (e0 + k >= start && e0 + k < end) poses[e0 + k] = v[k];
    }
}

// LIVE C1 MOTION (StreamSession(fps=F, interpolation="cubic")): keyframe_read with the C1 cubic through the kept keyframes in place of the
// line (rates.push_plan_cubic on the host; evaluation.interpolate_cubic_host is the rule).  u == k0 gives keyframe k0's bits as before;
// anything else hermite_mix (uu3d_tracks.h: float64, no contraction, rounded once) of the four ring places (k0 / P - 1) .. (k0 / P + 2)
// modulo the ring with keyframe_read's own weight.  A slot's first segment (k0 < P) has no keyframe in front: its place is not read -- it
// may hold a pose of the slot's previous track -- and the tangent at k0 is the segment's own difference.  A live track has no last
// segment: k0 + 2 P always counts, and the host's plan (rates.rate_plan(interpolation="cubic")) guarantees that it has been emitted and
// that k0 - P is still in the ring.
__device__ __forceinline__ float keyframe_read_cubic(const float* __restrict__ ring, const int key_ring, const int key_stride, const long P,
                                                     const long num, const long den, const int col)
{
    const long k0 = num / den / P * P;
    const long off = num - k0 * den;                                      // (u - k0) den, in [0, P den)
    const long i1 = k0 / P;
    const float p1 = ring[i1 % key_ring * key_stride + col];
    if (off == 0) return p1;
    const bool has0 = k0 >= P;                                            // (then i1 >= 1: the place below is not negative)
    const float p0 = has0 ? ring[(i1 - 1) % key_ring * key_stride + col] : p1;
    const float p2 = ring[(i1 + 1) % key_ring * key_stride + col];
    const float p3 = ring[(i1 + 2) % key_ring * key_stride + col];
    return hermite_mix(p0, p1, p2, p3, has0, true, (double)off / (double)(P * den));
}

// stream_timed_emit_kernel with keyframe_read_cubic: the same arguments, the same held pose and fresh_out, one thread per four
// consecutive floats.
static __global__ void __launch_bounds__(256)
stream_timed_emit_cubic_kernel(const RateParams p, const int32_t* __restrict__ source_frames, const uint8_t* __restrict__ pushed,
                               const float* __restrict__ keys, float* __restrict__ out_held, float* __restrict__ out, uint8_t* __restrict__ fresh_out)
{
    const long per = p.per_pose, total = (long)p.slots * per;
    const long e0 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (e0 >= total) return;
    float v[4];
    bool any_fresh = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long e = (e0 + k < total) ? e0 + k : e0;
        const long t = e / per;
        const int r = (int)(e - t * per);
        const long q = (long)source_frames[t] - 1 - p.lookahead;
        const bool is_fresh = pushed[t] != 0 && q >= 0;
        if (e == e0 + k && r == 0) fresh_out[t] = is_fresh ? 1 : 0;
        if (!is_fresh) { v[k] = out_held[e]; continue; }
        any_fresh = true;
        v[k] = keyframe_read_cubic(keys + t * p.key_ring * p.key_stride, p.key_ring, p.key_stride, p.pred_stride, q * p.a, p.b, r);
    }
    if (e0 + 4 <= total) {
        *reinterpret_cast<float4*>(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
        if (any_fresh) *reinterpret_cast<float4*>(out_held + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else for (int k = 0; e0 + k < total; ++k) { out[e0 + k] = v[k]; if (any_fresh) out_held[e0 + k] = v[k]; }
}

// stream_timed_emit_multi_kernel with keyframe_read_cubic: the same arguments, one workgroup per slot, the same counter discipline (read
// by the slot's workgroup, advanced by lane 0 behind the barrier, stopped at INT32_MAX), the same zero rows behind count and the same walk
// over the 16-byte quads of the slot's rows.
static __global__ void __launch_bounds__(256)
stream_timed_emit_multi_cubic_kernel(const RateParams p, const OutParams o, const int32_t* __restrict__ source_frames, const uint8_t* __restrict__ pushed,
                                     const float* __restrict__ keys, int32_t* __restrict__ out_frames, float* __restrict__ poses,
                                     int32_t* __restrict__ count)
{
    const int slot = blockIdx.x;
    const long done = out_frames[slot];
    const long q = (long)source_frames[slot] - 1 - p.lookahead;
    long n = 0;
    if (pushed[slot] != 0 && q >= 0 && done >= 0) {
        n = q * o.c / o.d + 1 - done;
        n = n < 0 ? 0 : (n > o.max_out ? o.max_out : n);
        if (n > (long)INT32_MAX - done) n = (long)INT32_MAX - done;
    }
    __syncthreads();                                                     // every read of the counter is done
    if (threadIdx.x == 0) { out_frames[slot] = (int32_t)(done + n); count[slot] = (int32_t)n; }
    const long per = p.per_pose;
    const long start = (long)slot * o.max_out * per, end = start + (long)o.max_out * per;
    const float* ring = keys + (long)slot * p.key_ring * p.key_stride;
    for (long quad = start / 4 + threadIdx.x; quad * 4 < end; quad += 256) {
        const long e0 = quad * 4;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = 0.f;
            const long rel = e0 + k - start;
            if (rel < 0 || e0 + k >= end) continue;
            const long r = rel / per;
            if (r >= n) continue;
            v[k] = keyframe_read_cubic(ring, p.key_ring, p.key_stride, p.pred_stride, (done + r) * o.un, o.ud, (int)(rel - r * per));
        }
        if (e0 >= start && e0 + 4 <= end) *reinterpret_cast<float4*>(poses + e0) = make_float4(v[0], v[1], v[2], v[3]);
        else for (int k = 0; k < 4; ++k) if (e0 + k >= start && e0 + k < end) poses[e0 + k] = v[k];
    }
}

// slot_mask (T) u8 or nullptr (every slot): the chosen slots start a new track -- the model counter and the sub-ticks' held pose (what
// stream_reset_kernel zeroes in a plain session), the source counter, the pushed byte and the held output pose go back to 0, and with
// out_frames (nullptr: the session has no output rate) the output counter.  The rings stay: nothing reads a source frame or a keyframe
// its slot's counters have not reached.  One thread per float of a held pose; the thread of a slot's first float writes its counters.
static __global__ void __launch_bounds__(256)
stream_rate_reset_kernel(const uint8_t* __restrict__ slot_mask, const int T, const int per_pose, int32_t* __restrict__ frames, float* __restrict__ held,
                         int32_t* __restrict__ source_frames, uint8_t* __restrict__ pushed, float* __restrict__ out_held, int32_t* __restrict__ out_frames)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)T * per_pose) return;
    const int t = (int)(i / per_pose);
    if (slot_mask != nullptr && slot_mask[t] == 0) return;
    held[i] = 0.f;
    out_held[i] = 0.f;
    if (i - (long)t * per_pose != 0) return;
    frames[t] = 0;
    source_frames[t] = 0;
    pushed[t] = 0;
    if (out_frames != nullptr) out_frames[t] = 0;
}

}  // namespace uu3d
