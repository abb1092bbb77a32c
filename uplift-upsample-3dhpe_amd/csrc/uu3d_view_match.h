// uu3d_view_match.h -- WHO IS WHO (include/uu3d.h; predict.view_pair_sums, predict.group_views, predict.gather_view_tracks,
// predict.match_views, predict.predict_views(match=...)): V calibrated cameras follow people on their own, so camera 0's track 2 is camera
// 1's track 0.  Two 2D tracks of different views are the same person iff the rays of their joints meet in space; this file measures that
// for every pair of tracks, groups the tracks to persons and lays the persons' tracks out the way uu3d_views.h reads them.
//     view_pair_sums_kernel      per unordered pair of tracks p <= q, one workgroup of 256 lanes: the lanes run over the frames, each frame's
//                                joints in ascending order, then a fixed tree through LDS; both mirrored elements from one writer
//     group_views_kernel         one wave: the greedy, view-by-view grouping on the (M, M) tables, a person per lane
//     gather_view_tracks_kernel  per (view, person row, joint), one lane: the padded view-major buffers of uu3d_fuse_views
// Float64 on the float32 inputs, every operation rounded once (contraction off).  The order of every sum is fixed by the rule, not by the
// machine: bitwise repeatable.  No atomics.  The statements are those of predict.view_pair_sums_host / predict.group_views_host /
// predict.gather_view_tracks_host, one for one.
#pragma once
#include "uu3d_views.h"

namespace uu3d {

static constexpr int kMatchMaxTracks = 64;                               // M beyond it: UU3D_ERR_UNSUPPORTED (a person or a track per lane of one wave)
static constexpr int kMatchLanes = 256;                                  // lanes of a pair's workgroup; part of the rule: lane l sums frames l, l + 256, ...
// cc > kViewParallel * (pp * qq), i.e. sin^2 of the angle between the two rays > 2^-20: rays closer than about 1e-3 rad carry no distance
// information -- the distance between two nearly parallel lines is a quotient of two roundings.
static constexpr double kViewParallel = 0x1p-20;

// The tracks are view-major: view v holds tracks start[v] .. start[v + 1] - 1, start[views] = M.  By value: the host has checked it.
struct ViewStarts { int start[kViewsMax + 1]; };

__device__ __forceinline__ int view_of_track(const ViewStarts& st, const int views, const int m)
{
    int v = 0;
    while (v + 1 < views && m >= st.start[v + 1]) ++v;
    return v;
}

// The ray of pixel uv in world axes: d_i = (r1_i a + r2_i b) + r3_i with a = (u - cx) / fx, b = (v - cy) / fy; c = a row of view_rows.
__device__ __forceinline__ void view_ray(const float2 uv, const double* __restrict__ c, double d[3])
{
#pragma clang fp contract(off)
    const double a = ((double)uv.x - c[2]) / c[0];
    const double b = ((double)uv.y - c[3]) / c[1];
    d[0] = (c[4] * a + c[7] * b) + c[10];
    d[1] = (c[5] * a + c[8] * b) + c[11];
    d[2] = (c[6] * a + c[9] * b) + c[12];
}

// The per-joint expression of PAIR SUMS, shared with ONE CLOCK (uu3d_view_align.h) so that the bits cannot drift: dp, dq the two rays, o the
// way from the first camera to the second -> whether the term counts, and e = the squared distance between the two lines.
__device__ __forceinline__ bool view_line_term(const double dp[3], const double dq[3], const double o[3], double* e_out)
{
#pragma clang fp contract(off)
    const double c0 = dp[1] * dq[2] - dp[2] * dq[1];
    const double c1 = dp[2] * dq[0] - dp[0] * dq[2];
    const double c2 = dp[0] * dq[1] - dp[1] * dq[0];
    const double cc = (c0 * c0 + c1 * c1) + c2 * c2;
    const double pp = (dp[0] * dp[0] + dp[1] * dp[1]) + dp[2] * dp[2];
    const double qq = (dq[0] * dq[0] + dq[1] * dq[1]) + dq[2] * dq[2];
    const double oc = (o[0] * c0 + o[1] * c1) + o[2] * c2;
    const double e = (oc * oc) / cc;
    *e_out = e;
    return cc > kViewParallel * (pp * qq) && finite_double(e);
}

// Block i = the pair (p, q), p <= q, in row-major order of the upper triangle.  kp (M, T, J, 2) f32, flags (M, T, J) u8 or nullptr,
// cams (views, 16) f64 -> sums (M, M) f64, terms (M, M) i32, both symmetric.
static __global__ void __launch_bounds__(kMatchLanes)
view_pair_sums_kernel(const float* __restrict__ kp, const uint8_t* __restrict__ flags, const ViewStarts st, const double* __restrict__ cams, const int M, const int T, const int J, const int views,
                      double* __restrict__ sums, int* __restrict__ terms)
{
#pragma clang fp contract(off)
    __shared__ double xs[kMatchLanes];
    __shared__ int ns[kMatchLanes];
    const int lane = threadIdx.x;
    int p = 0, left = (int)blockIdx.x;                                   // (uniform: at most M steps)
    while (left >= M - p) { left -= M - p; ++p; }
    const int q = p + left;
    if (p >= M || q >= M) return;
    const int v = view_of_track(st, views, p), w = view_of_track(st, views, q);
    bool live = v != w;                                                  // (the diagonal is a same-view pair)
    double o[3] = {0.0, 0.0, 0.0};
    if (live) {
        for (int i = 0; i < 3; ++i) o[i] = cams[kViewCamera * w + 13 + i] - cams[kViewCamera * v + 13 + i];
        const double oo = (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2];
        live = finite_double(oo) && oo > 0.0;                            // coincident cameras cannot be matched by geometry
    }
    if (!live) {                                                         // zeros, before any loop
        if (lane == 0) {
            sums[(long)p * M + q] = 0.0;
            terms[(long)p * M + q] = 0;
            if (p != q) { sums[(long)q * M + p] = 0.0; terms[(long)q * M + p] = 0; }
        }
        return;
    }
    double cp[kViewCamera], cq[kViewCamera];
    for (int i = 0; i < kViewCamera; ++i) { cp[i] = cams[kViewCamera * v + i]; cq[i] = cams[kViewCamera * w + i]; }
    double x = 0.0;
    int n = 0;
    for (int f = lane; f < T; f += kMatchLanes) {
        const long ap = ((long)p * T + f) * J, aq = ((long)q * T + f) * J;
        double s = 0.0;
        for (int j = 0; j < J; ++j) {
            if (!view_joint_used(kp, flags, ap + j) || !view_joint_used(kp, flags, aq + j)) continue;
            double dp[3], dq[3];
            view_ray(*reinterpret_cast<const float2*>(kp + 2 * (ap + j)), cp, dp);
            view_ray(*reinterpret_cast<const float2*>(kp + 2 * (aq + j)), cq, dq);
            double e;
            if (view_line_term(dp, dq, o, &e)) {
                s = s + e;
                n += 1;
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
    if (lane == 0) {
        sums[(long)p * M + q] = xs[0];
        sums[(long)q * M + p] = xs[0];
        terms[(long)p * M + q] = ns[0];
        terms[(long)q * M + p] = ns[0];
    }
}

// One wave.  sums / terms (M, M) -> person (M), n_persons (1), table (views, M).  Lane k holds person k while a view is
// matched; the smallest (cost, k, b) is found by a butterfly of exact comparisons, which has one answer whatever the order.
static __global__ void __launch_bounds__(64)
group_views_kernel(const double* __restrict__ sums, const int* __restrict__ terms, const ViewStarts st, const int M, const int views,
                   const double max_dist, const int min_terms, int* __restrict__ person, int* __restrict__ n_persons, int* __restrict__ table)
{
#pragma clang fp contract(off)
    __shared__ int tab[kViewsMax][kMatchMaxTracks];                      // the track of person k in view v, or -1
    __shared__ int who[kMatchMaxTracks];                                 // the person of track m
    __shared__ double cost[kMatchMaxTracks * kMatchMaxTracks / 4];       // persons x tracks of one step: P0 + nb <= M, so P0 * nb <= M * M / 4
    const int lane = threadIdx.x;
    for (int v = 0; v < kViewsMax; ++v) tab[v][lane] = -1;
    who[lane] = -1;
    __syncthreads();
    const double limit = max_dist * max_dist;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    int P = 0;                                                           // persons so far (uniform)
    for (int w = 0; w < views; ++w) {
        const int lo = st.start[w], nb = st.start[w + 1] - lo;           // the view's tracks are lo .. lo + nb - 1
        if (nb <= 0) continue;
        const int P0 = P;
        unsigned long long taken = 0;                                    // tracks of view w that found a person (bit b - lo; uniform)
        if (P0 > 0) {
            if (lane < P0) {
                for (int bi = 0; bi < nb; ++bi) {
                    const int b = lo + bi;
                    double S = 0.0;
                    int n = 0;
                    for (int u = 0; u < w; ++u) {                        // the members in ascending order: one per earlier view
                        const int m = tab[u][lane];
                        if (m < 0) continue;
                        const int t = terms[(long)m * M + b];
                        if (t > 0) { S = S + sums[(long)m * M + b]; n += t; }
                    }
                    const double mean = S / (double)n;
                    cost[lane * nb + bi] = (n >= min_terms && n > 0 && mean <= limit) ? mean : inf;
                }
            }
            __syncthreads();
            bool free_k = lane < P0;                                     // person `lane` has no track in view w yet
            const int rounds = P0 < nb ? P0 : nb;
            for (int r = 0; r < rounds; ++r) {
                double best = inf;
                int bb = kMatchMaxTracks, bk = kMatchMaxTracks;
                if (free_k) {
                    for (int bi = 0; bi < nb; ++bi) {
                        if ((taken >> bi) & 1ull) continue;
                        const double c = cost[lane * nb + bi];
                        if (c < best) { best = c; bb = bi; bk = lane; }  // strict: ties go to the smaller b
                    }
                }
                for (int step = 32; step >= 1; step >>= 1) {
                    const double oc = __shfl_xor(best, step, 64);
                    const int ok = __shfl_xor(bk, step, 64), ob = __shfl_xor(bb, step, 64);
                    if (oc < best || (oc == best && ok < bk)) { best = oc; bk = ok; bb = ob; }       // ties go to the smaller k
                }
                if (bk >= kMatchMaxTracks) break;                        // no allowed pair is left (uniform)
                taken |= 1ull << bb;
                if (lane == bk) {
                    free_k = false;
                    tab[w][lane] = lo + bb;
                    who[lo + bb] = lane;
                }
            }
        }
        if (lane == 0) {                                                 // the unmatched tracks become new persons, in ascending track order
            int next = P0;
            for (int bi = 0; bi < nb; ++bi) {
                if ((taken >> bi) & 1ull) continue;
                tab[w][next] = lo + bi;
                who[lo + bi] = next;
                ++next;
            }
        }
        P = P0 + nb - __popcll(taken);
        __syncthreads();
    }
    if (lane < M) person[lane] = who[lane];
    for (int v = 0; v < views; ++v)
        if (lane < M) table[v * M + lane] = tab[v][lane];
    if (lane == 0) n_persons[0] = P;
}

// Lane i = ((v * P + k) * T + f) * J + j.  src (views * P) i32: the track of person k in view v, or -1 (anything outside 0 .. M - 1 counts
// as -1).  poses (M * T, J, 3) f32, kp (M * T, J, 2) f32, flags (M * T, J) u8 or nullptr -> the view-major buffers (views, P * T, J, 3 | 2 | 1);
// an absent block: zero poses, NaN keypoints, flags 0.
static __global__ void __launch_bounds__(256)
gather_view_tracks_kernel(const int* __restrict__ src, const float* __restrict__ poses, const float* __restrict__ kp, const uint8_t* __restrict__ flags,
                          const int views, const int P, const int T, const int J, const int M, float* __restrict__ out_poses,
                          float* __restrict__ out_kp, uint8_t* __restrict__ out_flags)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long per_track = (long)T * J;
    if (i >= (long)views * P * per_track) return;
    const long block = i / per_track, within = i - block * per_track;
    const int m = src[block];
    WorldTrio t;
    t.a = t.b = t.c = 0.0f;
    float2 uv = make_float2(__uint_as_float(0x7fc00000u), __uint_as_float(0x7fc00000u));
    uint8_t flag = 0;
    if (m >= 0 && m < M) {
        const long at = (long)m * per_track + within;
        t = *reinterpret_cast<const WorldTrio*>(poses + at * 3);
        uv = *reinterpret_cast<const float2*>(kp + at * 2);
        flag = flags == nullptr ? (uint8_t)1 : (uint8_t)(flags[at] != 0 ? 1 : 0);
    }
    *reinterpret_cast<WorldTrio*>(out_poses + i * 3) = t;
    *reinterpret_cast<float2*>(out_kp + i * 2) = uv;
    out_flags[i] = flag;
}

}  // namespace uu3d
