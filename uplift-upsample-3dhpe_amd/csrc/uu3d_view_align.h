// uu3d_view_align.h -- ONE CLOCK (include/uu3d.h; predict.view_lag_sums, predict.view_offsets, predict.align_views,
// predict.predict_views(align=...)): V calibrated cameras were started by hand, so frame f of one is not frame f of another.  The squared
// distance between the lines through two cameras and the same joint's pixels (WHO IS WHO, PAIR SUMS) is smallest when the two frames were
// taken at the same instant; this file sums it for every track of the reference view, every track of a later view and every lag in
// -L .. L, and takes the best lag per view.
//     view_lag_rays_kernel  per (track, frame, joint), one lane: the joint's ray in world axes, three f64, and whether it is used -- once,
//                           not 2L + 1 times
//     view_lag_sums_kernel  per (p, q, lag), one workgroup of 256 lanes: the lanes run over p's frames, each frame's joints in ascending
//                           order, then the fixed tree through LDS; one writer per element
//     view_offsets_kernel   one wave: the lags over the lanes, per view the smallest (score, |l|, l) by a butterfly of exact comparisons
// Float64 on the float32 inputs, every operation rounded once (contraction off).  The per-joint expression is view_line_term of
// uu3d_view_match.h, the order of summation that of PAIR SUMS: at lag 0 on tracks of equal length the bits of uu3d_view_pair_sums.  No
// atomics.  The statements are those of predict.view_lag_sums_host / predict.view_offsets_host, one for one.
#pragma once
#include "uu3d_view_match.h"

namespace uu3d {

static constexpr int kAlignMaxLag = 512;                                 // L beyond it: UU3D_ERR_UNSUPPORTED

// Track m holds rows first[m] .. first[m + 1] - 1 of kp.  By value: the host has checked it (strictly ascending, frames * J < 2^31).
struct TrackRows { long first[kMatchMaxTracks + 1]; };

// scratch: rays (rows, J, 3) f64, then used (rows, J) u8.
__host__ __device__ __forceinline__ size_t view_lag_used_offset(const long rows, const int J) { return (size_t)rows * (size_t)J * 3 * sizeof(double); }

// Block (x, m): lanes x * 256 .. of track m's frames * J joints.
static __global__ void __launch_bounds__(256)
view_lag_rays_kernel(const float* __restrict__ kp, const uint8_t* __restrict__ flags, const ViewStarts st, const TrackRows rows, const double* __restrict__ cams,
                     const int J, const int views, double* __restrict__ rays, uint8_t* __restrict__ used)
{
#pragma clang fp contract(off)
    const int m = blockIdx.y;
    const long first = rows.first[m];
    const long count = (rows.first[m + 1] - first) * J;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const long at = first * J + i;
    const double* c = cams + kViewCamera * view_of_track(st, views, m);
    double cam[13], d[3];
    for (int k = 0; k < 13; ++k) cam[k] = c[k];
    view_ray(*reinterpret_cast<const float2*>(kp + 2 * at), cam, d);
    rays[3 * at] = d[0];
    rays[3 * at + 1] = d[1];
    rays[3 * at + 2] = d[2];
    used[at] = view_joint_used(kp, flags, at) ? (uint8_t)1 : (uint8_t)0;
}

// Block (x, q, p): lag l = x - L of reference track p < n_ref against track q.  sums / terms (n_ref, M, 2L + 1).
static __global__ void __launch_bounds__(kMatchLanes)
view_lag_sums_kernel(const double* __restrict__ rays, const uint8_t* __restrict__ used, const ViewStarts st, const TrackRows rows, const double* __restrict__ cams,
                     const int M, const int J, const int views, const int n_ref, const int ref_view, const int L, double* __restrict__ sums,
                     int* __restrict__ terms)
{
#pragma clang fp contract(off)
    __shared__ double xs[kMatchLanes];
    __shared__ int ns[kMatchLanes];
    const int lane = threadIdx.x;
    const int p = blockIdx.z, q = blockIdx.y, l = (int)blockIdx.x - L;
    if (p >= n_ref || q >= M || l > L) return;
    const long out = ((long)p * M + q) * (2 * L + 1) + blockIdx.x;
    bool live = q >= n_ref;                                              // (the columns of the reference view hold zeros)
    double o[3] = {0.0, 0.0, 0.0};
    if (live) {
        const int w = view_of_track(st, views, q);
        for (int i = 0; i < 3; ++i) o[i] = cams[kViewCamera * w + 13 + i] - cams[kViewCamera * ref_view + 13 + i];
        const double oo = (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2];
        live = finite_double(oo) && oo > 0.0;                            // coincident cameras: no terms
    }
    if (!live) {
        if (lane == 0) { sums[out] = 0.0; terms[out] = 0; }
        return;
    }
    const long fp = rows.first[p], fq = rows.first[q];
    const int Tp = (int)(rows.first[p + 1] - fp), Tq = (int)(rows.first[q + 1] - fq);
    double x = 0.0;
    int n = 0;
    for (int f = lane; f < Tp; f += kMatchLanes) {
        const int g = f - l;                                             // (|l| <= 512 and f < 2^31 / J: no overflow)
        double s = 0.0;
        if (g >= 0 && g < Tq) {
            const long ap = (fp + f) * J, aq = (fq + g) * J;
            for (int j = 0; j < J; ++j) {
                if (used[ap + j] == 0 || used[aq + j] == 0) continue;
                const double* rp = rays + 3 * (ap + j);
                const double* rq = rays + 3 * (aq + j);
                const double dp[3] = {rp[0], rp[1], rp[2]}, dq[3] = {rq[0], rq[1], rq[2]};
                double e;
                if (view_line_term(dp, dq, o, &e)) {
                    s = s + e;
                    n += 1;
                }
            }
        }
        x = x + s;
    }
    xs[lane] = x;
    ns[lane] = n;
    __syncthreads();
    for (int stride = kMatchLanes / 2; stride >= 1; stride >>= 1) {      // the fixed tree
        if (lane < stride) {
            xs[lane] = xs[lane] + xs[lane + stride];
            ns[lane] = ns[lane] + ns[lane + stride];
        }
        __syncthreads();
    }
    if (lane == 0) { sums[out] = xs[0]; terms[out] = ns[0]; }
}

// (score a, lag la) before (score b, lag lb): the smaller score, then the smaller |l|, then the smaller l.  Exact comparisons: a total
// order on distinct lags, so the minimum is one answer whatever the order it is looked for in.
__device__ __forceinline__ bool lag_before(const double a, const int la, const double b, const int lb)
{
    if (a < b) return true;
    if (!(a == b)) return false;
    const int ma = la < 0 ? -la : la, mb = lb < 0 ? -lb : lb;
    return ma < mb || (ma == mb && la < lb);
}

// One wave.  sums / terms (n_ref, M, 2L + 1) -> offset (views) i32, state (views) i32, score (views) f64.  Lane i looks at the lags
// i - L, i + 64 - L, ...; kNoLag marks a lane (or a view) without an allowed lag.
static __global__ void __launch_bounds__(64)
view_offsets_kernel(const double* __restrict__ sums, const int* __restrict__ terms, const ViewStarts st, const int M, const int views, const int n_ref,
                    const int ref_view, const int L, const int min_terms, const int same_index, int* __restrict__ offset, int* __restrict__ state,
                    double* __restrict__ score)
{
#pragma clang fp contract(off)
    constexpr int kNoLag = 2 * kAlignMaxLag;
    const int lane = threadIdx.x;
    const int lags = 2 * L + 1;
    for (int w = 0; w < views; ++w) {
        const int lo = st.start[w], nb = st.start[w + 1] - lo;
        if (w == ref_view || nb <= 0) {                                  // the reference view and empty views
            if (lane == 0) { offset[w] = 0; state[w] = 1; score[w] = 0.0; }
            continue;
        }
        double best = 0.0;
        int bl = kNoLag;
        for (int i = lane; i < lags; i += 64) {
            double S = 0.0;
            long n = 0;
            bool allowed = false;
            for (int p = 0; p < n_ref; ++p) {
                const long row = ((long)p * M) * lags + i;
                int bq = -1;
                double bm = 0.0;
                if (same_index != 0) {
                    const int q = lo + p;                                // (the host has checked nb == n_ref)
                    if (terms[row + (long)q * lags] >= min_terms) bq = q;
                } else {
                    for (int q = lo; q < lo + nb; ++q) {
                        const int t = terms[row + (long)q * lags];
                        if (t < min_terms) continue;
                        const double mean = sums[row + (long)q * lags] / (double)t;
                        if (bq < 0 || mean < bm) { bq = q; bm = mean; }  // strict: ties go to the smaller q
                    }
                }
                if (bq < 0) continue;
                S = S + sums[row + (long)bq * lags];
                n = n + terms[row + (long)bq * lags];
                allowed = true;
            }
            if (!allowed) continue;
            const double sc = S / (double)n;
            if (bl == kNoLag || lag_before(sc, i - L, best, bl)) { best = sc; bl = i - L; }
        }
        for (int step = 32; step >= 1; step >>= 1) {
            const double ob = __shfl_xor(best, step, 64);
            const int ol = __shfl_xor(bl, step, 64);
            if (ol != kNoLag && (bl == kNoLag || lag_before(ob, ol, best, bl))) { best = ob; bl = ol; }
        }
        if (lane == 0) {
            offset[w] = bl == kNoLag ? 0 : bl;
            state[w] = bl == kNoLag ? 0 : 1;
            score[w] = bl == kNoLag ? 0.0 : best;
        }
    }
}

}  // namespace uu3d
