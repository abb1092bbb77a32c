// uu3d_smooth.h -- STEADY OUTPUT (include/uu3d.h; predict.one_euro, predict.predict_tracks(smooth=...), stream.LiveOneEuro,
// stream.StreamSession(smooth=...)): the One-Euro filter (Casiez, Roussel, Vogel 2012) over the poses and roots a call or a session
// returns.  A CHANNEL is one scalar over time; the filter is an exponential smoother whose cut-off rises with the channel's speed.
//     one_euro_tracks_kernel        offline: one lane per (track, channel) walks the track's rows in order -- adjacent lanes are adjacent
//                                   channels of one row, so every step of the walk is one coalesced row read and one row write
//     one_euro_tracks_two_pass_kernel  offline, zero lag: the same lane then walks back over the rows it wrote, in place, in the same launch
//     stream_one_euro_kernel        live: one workgroup per slot, lanes over channels, one sample per fresh pose, the state kept per slot
//     stream_one_euro_reset_kernel  chosen slots: back to no sample taken
// The rule is predict.one_euro_host's, statement for statement, in float64 with every operation rounded (no fused multiply-add, IEEE
// division): the device equals the numpy mirror bit for bit.  Every output and state element has one writer, no atomics, the caller's
// buffers are only read: bitwise repeatable, capturable.  The kernels are latency-bound recurrences (two divisions per sample in the chain).
#pragma once
#include "uu3d_root.h"

namespace uu3d {

static constexpr int kSmoothMaxChannels = 1 << 16;                      // C beyond it: UU3D_ERR_UNSUPPORTED
static constexpr int kSmoothLanes = 64;                                 // one wave: the lanes of a workgroup of both kernels

__device__ __forceinline__ bool finite_float(const float x)
{
    return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
}

// alpha(fc, r) = 1 / (1 + r / (2 pi fc)): the weight of the new sample at cut-off fc (Hz) and sample rate r (Hz)
__device__ __forceinline__ double one_euro_alpha(const double fc, const double r)
{
#pragma clang fp contract(off)
    return 1.0 / (1.0 + r / (6.283185307179586 * fc));
}

// One later sample x of a channel at sample rate r; ad = alpha(d_cutoff, r).  The statements of predict.one_euro_host, one for one.
__device__ __forceinline__ void one_euro_sample(const double x, const double r, const double ad, const double min_cutoff, const double beta,
                                                double& xh, double& dxh)
{
#pragma clang fp contract(off)
    const double dx = (x - xh) * r;
    dxh = ad * dx + (1.0 - ad) * dxh;
    const double a = one_euro_alpha(min_cutoff + beta * fabs(dxh), r);
    xh = a * x + (1.0 - a) * xh;
}

// in, out (rows, C) f32, out != in; track_start, track_len (tracks) i64: the rows of a track; rates (tracks) f64: its sample rate in Hz;
// state: nullptr or (rows) u8, 0 = the row is passed through and takes no sample.  Grid (tracks, ceil(C / 64)): the wave walks ONE track,
// so its trip count is uniform.  A non-finite sample is passed through and touches no state.  The next row is read before this one is
// worked on: the reads do not depend on the recurrence.
static __global__ void __launch_bounds__(kSmoothLanes)
one_euro_tracks_kernel(const float* __restrict__ in, float* __restrict__ out, const long rows, const int C, const int64_t* __restrict__ track_start,
                       const int64_t* __restrict__ track_len, const double* __restrict__ rates, const uint8_t* __restrict__ state,
                       const double min_cutoff, const double beta, const double d_cutoff)
{
    const int c = blockIdx.y * kSmoothLanes + threadIdx.x;
    if (c >= C) return;
    const int track = blockIdx.x;
    long first = track_start[track], n = track_len[track];
    if (first < 0 || n < 1 || first >= rows) return;
    if (n > rows - first) n = rows - first;                              // (nothing is read or written beyond the buffers)
    const double r = rates[track];
    const double ad = one_euro_alpha(d_cutoff, r);                      // (every sample of an offline track is one frame behind the last)
    double xh = 0.0, dxh = 0.0;
    bool taken = false;
    const float* src = in + first * C + c;
    float* dst = out + first * C + c;
    const uint8_t* st = state == nullptr ? nullptr : state + first;
    float v = src[0];
    for (long i = 0; i < n; ++i) {
        const float cur = v;
        if (i + 1 < n) v = src[(i + 1) * C];
        float y = cur;
        if ((st == nullptr || st[i] != 0) && finite_float(cur)) {
            const double x = (double)cur;
            if (!taken) {
                xh = x;
                dxh = 0.0;
                taken = true;
            } else one_euro_sample(x, r, ad, min_cutoff, beta, xh, dxh);
            y = (float)xh;
        }
        dst[i * C] = y;
    }
}

// The zero-lag form (OneEuro(zero_lag=True); offline only): the arguments, the grid and pass 1 of one_euro_tracks_kernel -- a kernel of its
// own, so the causal one stays instruction for instruction what it is.  Behind its forward walk the lane walks BACK from row n - 1 to row
// 0 over the f32 values it wrote to out itself and writes the final value in place: the same walk with the rows taken last to first, the
// same rate, parameters and state bytes, xh / dxh / taken fresh.  Per track the result is reverse(walk(reverse(walk(in)))), bit for bit
// (predict.one_euro_host).  A lane reads back only its own stores, in program order: no barrier, no fence, no scratch buffer, every
// element still has one writer.  in stays read-only (out != in).  The next row -- the one BEFORE this one on the way back -- is read
// before this one is worked on, in both directions.
static __global__ void __launch_bounds__(kSmoothLanes)
one_euro_tracks_two_pass_kernel(const float* __restrict__ in, float* out, const long rows, const int C, const int64_t* __restrict__ track_start,
                                const int64_t* __restrict__ track_len, const double* __restrict__ rates, const uint8_t* __restrict__ state,
                                const double min_cutoff, const double beta, const double d_cutoff)
{
    const int c = blockIdx.y * kSmoothLanes + threadIdx.x;
    if (c >= C) return;
    const int track = blockIdx.x;
    long first = track_start[track], n = track_len[track];
    if (first < 0 || n < 1 || first >= rows) return;
    if (n > rows - first) n = rows - first;                              // (nothing is read or written beyond the buffers)
    const double r = rates[track];
    const double ad = one_euro_alpha(d_cutoff, r);
    const float* src = in + first * C + c;
    float* dst = out + first * C + c;
    const uint8_t* st = state == nullptr ? nullptr : state + first;
    // pass 1: one_euro_tracks_kernel's walk, statement for statement
    double xh = 0.0, dxh = 0.0;
    bool taken = false;
    float v = src[0];
    for (long i = 0; i < n; ++i) {
        const float cur = v;
        if (i + 1 < n) v = src[(i + 1) * C];
        float y = cur;
        if ((st == nullptr || st[i] != 0) && finite_float(cur)) {
            const double x = (double)cur;
            if (!taken) {
                xh = x;
                dxh = 0.0;
                taken = true;
            } else one_euro_sample(x, r, ad, min_cutoff, beta, xh, dxh);
            y = (float)xh;
        }
        dst[i * C] = y;
    }
    // pass 2: the same walk over this lane's own rows of out, last to first, in place
    xh = 0.0;
    dxh = 0.0;
    taken = false;
    v = dst[(n - 1) * C];
    for (long i = n - 1; i >= 0; --i) {
        const float cur = v;
        if (i > 0) v = dst[(i - 1) * C];
        if ((st == nullptr || st[i] != 0) && finite_float(cur)) {
            const double x = (double)cur;
            if (!taken) {
                xh = x;
                dxh = 0.0;
                taken = true;
            } else one_euro_sample(x, r, ad, min_cutoff, beta, xh, dxh);
            dst[i * C] = (float)xh;
        }
    }
}

// The state block of a live filter, per slot and channel: xh and dxh (f64), the frame index of the channel's last sample (i32) and
// whether it has taken one (u8).  All of it per channel: a channel whose sample was not finite took none, so its next n is its own.
struct OneEuroLayout {
    size_t off_xh, off_dxh, off_last, off_taken, bytes;
};
inline size_t one_euro_align(size_t v) { return (v + 255) / 256 * 256; }
inline OneEuroLayout one_euro_layout(const int slots, const int C)
{
    OneEuroLayout L{};
    const size_t e = (size_t)slots * (size_t)C;
    L.off_xh = 0;
    L.off_dxh = one_euro_align(e * sizeof(double));
    L.off_last = L.off_dxh + one_euro_align(e * sizeof(double));
    L.off_taken = L.off_last + one_euro_align(e * sizeof(int32_t));
    L.bytes = L.off_taken + one_euro_align(e);
    return L;
}

// One workgroup per slot, lanes over channels (C beyond the workgroup: each lane loops).  frames (T) i32: the slot's frame counter AFTER
// this push; the fresh value belongs to frame f = frames - 1 - lookahead.  active, fresh (T) u8; values (T, C) f32: what the push returns,
// only read; state: nullptr or (T) u8, 0 = the slot's values are passed through.
//   an active slot whose value is fresh: per channel one sample with n = f - last (anything below 1 counts as 1) at rate / n -- the first
//       one is taken as given; a non-finite value, or the whole row with state 0, is passed through and touches nothing.
//   any other slot returns the channel's xh rounded once, zeros before its first sample.
static __global__ void __launch_bounds__(kSmoothLanes)
stream_one_euro_kernel(const int C, const int lookahead, const int32_t* __restrict__ frames, const uint8_t* __restrict__ active,
                       const uint8_t* __restrict__ fresh, const float* __restrict__ values, const uint8_t* __restrict__ state, const double rate,
                       const double min_cutoff, const double beta, const double d_cutoff, double* __restrict__ xh_all, double* __restrict__ dxh_all,
                       int32_t* __restrict__ last_all, uint8_t* __restrict__ taken_all, float* __restrict__ out)
{
#pragma clang fp contract(off)
    const int slot = blockIdx.x;
    const int count = frames[slot];
    const bool sample = active[slot] != 0 && fresh[slot] != 0 && count >= 1;
    const bool pass = state != nullptr && state[slot] == 0;
    const int f = count - 1 - lookahead;
    const long base = (long)slot * C;
    for (int c = threadIdx.x; c < C; c += kSmoothLanes) {
        const long e = base + c;
        const bool taken = taken_all[e] != 0;
        if (!sample) {
            out[e] = taken ? (float)xh_all[e] : 0.f;
            continue;
        }
        const float v = values[e];
        if (pass || !finite_float(v)) {
            out[e] = v;
            continue;
        }
        const double x = (double)v;
        double xh = x, dxh = 0.0;
        if (taken) {
            long n = (long)f - (long)last_all[e];
            if (n < 1) n = 1;
            const double r = rate / (double)n;
            xh = xh_all[e];
            dxh = dxh_all[e];
            one_euro_sample(x, r, one_euro_alpha(d_cutoff, r), min_cutoff, beta, xh, dxh);
        }
        xh_all[e] = xh;
        dxh_all[e] = dxh;
        last_all[e] = f;
        taken_all[e] = 1;
        out[e] = (float)xh;
    }
}

// slot_mask (T) u8 or nullptr (every slot): the chosen slots have taken no sample, zeros.  One workgroup per slot.
static __global__ void __launch_bounds__(256)
stream_one_euro_reset_kernel(const uint8_t* __restrict__ slot_mask, const int C, double* __restrict__ xh_all, double* __restrict__ dxh_all,
                             int32_t* __restrict__ last_all, uint8_t* __restrict__ taken_all)
{
    const int slot = blockIdx.x;
    if (slot_mask != nullptr && slot_mask[slot] == 0) return;            // (uniform in the workgroup)
    const long base = (long)slot * C;
    for (int c = threadIdx.x; c < C; c += 256) {
        xh_all[base + c] = 0.0;
        dxh_all[base + c] = 0.0;
        last_all[base + c] = 0;
        taken_all[base + c] = 0;
    }
}

}  // namespace uu3d
