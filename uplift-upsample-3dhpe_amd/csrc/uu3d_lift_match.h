// uu3d_lift_match.h -- WHO IS WHO WITHOUT A WORLD (include/uu3d.h; predict.lift_pair_sums, predict.match_lifts,
// predict.predict_views(match=MatchLifts(...))): WHO IS WHO compares pixel rays in world axes, and cameras without extrinsics share no world
// yet.  Every view's lift is the same skeleton in that camera's own axes, so two tracks of different views are the same person iff their
// lifts agree up to ONE rotation over the whole track; Horn's largest eigenvalue gives the residual of that best rotation in closed form.
//     lift_pair_sums_kernel      per unordered pair of tracks p <= q, one workgroup of 256 lanes: the lanes run over the frames both tracks
//                                see, eleven values per frame (the nine moment products of uu3d_view_calibrate.h, the two lifts' squared
//                                size, 1.0), a fixed tree through LDS, one value after the other; lane 0 then runs Horn's matrix through the
//                                Jacobi sweeps of solve_view_pose_kernel and writes both mirrored elements
// uu3d_group_views and uu3d_gather_view_tracks (uu3d_view_match.h) take the tables from here unchanged.  Float64 on the float32 inputs,
// every operation rounded once (contraction off), division correctly rounded.  Every output element has one writer, no atomics, the inputs
// are only read, nothing per lane is indexed by a run-time view or track number: bitwise repeatable.  The statements are those of
// predict.lift_pair_sums_host, one for one.
#pragma once
#include "uu3d_view_calibrate.h"
#include "uu3d_view_match.h"

namespace uu3d {

static constexpr int kLiftPairSums = 11;                                 // doubles per term: nine moment products, the squared size, 1.0

// Block i = the pair (p, q), p <= q, in row-major order of the upper triangle.  poses (M, T, J, 3) f32, kp (M, T, J, 2) f32, flags
// (M, T, J) u8 or nullptr -> sums (M, M) f64, terms (M, M) i32, both symmetric.
static __global__ void __launch_bounds__(kMatchLanes)
lift_pair_sums_kernel(const float* __restrict__ poses, const float* __restrict__ kp, const uint8_t* __restrict__ flags, const ViewStarts st,
                      const int M, const int T, const int J, const int views, const int min_joints, double* __restrict__ sums,
                      int* __restrict__ terms)
{
#pragma clang fp contract(off)
    __shared__ double lds[kMatchLanes];
    const int lane = threadIdx.x;
    int p = 0, left = (int)blockIdx.x;                                   // (uniform: at most M steps)
    while (left >= M - p) { left -= M - p; ++p; }
    const int q = p + left;
    if (p >= M || q >= M) return;
    if (view_of_track(st, views, p) == view_of_track(st, views, q)) {    // a same-view pair or the diagonal: zeros, before any loop
        if (lane == 0) {
            sums[(long)p * M + q] = 0.0;
            terms[(long)p * M + q] = 0;
            if (p != q) { sums[(long)q * M + p] = 0.0; terms[(long)q * M + p] = 0; }
        }
        return;
    }
    double x[kLiftPairSums];
#pragma unroll
    for (int i = 0; i < kLiftPairSums; ++i) x[i] = 0.0;
    for (int f = lane; f < T; f += kMatchLanes) {
        const long ap = ((long)p * T + f) * J, aq = ((long)q * T + f) * J;
        if (!view_sees_row(kp, flags, ap, J, min_joints) || !view_sees_row(kp, flags, aq, J, min_joints)) continue;
        double s[kLiftPairSums];
        lift_moment_products(poses, ap, aq, J, s);
        double e = 0.0;
        for (int j = 0; j < J; ++j) {
            const WorldTrio a = *reinterpret_cast<const WorldTrio*>(poses + (ap + j) * 3);
            const WorldTrio b = *reinterpret_cast<const WorldTrio*>(poses + (aq + j) * 3);
            const double a0 = (double)a.a, a1 = (double)a.b, a2 = (double)a.c;
            const double b0 = (double)b.a, b1 = (double)b.b, b2 = (double)b.c;
            e = e + (((a0 * a0 + a1 * a1) + a2 * a2) + ((b0 * b0 + b1 * b1) + b2 * b2));
        }
        s[9] = e;
        s[10] = 1.0;
#pragma unroll
        for (int i = 0; i < kLiftPairSums; ++i) x[i] = x[i] + s[i];
    }
    double total[kLiftPairSums];                                         // (lane 0's are the sums)
#pragma unroll
    for (int i = 0; i < kLiftPairSums; ++i) {
        lds[lane] = x[i];
        __syncthreads();
        for (int stride = kMatchLanes / 2; stride >= 1; stride >>= 1) {  // the fixed tree
            if (lane < stride) lds[lane] = lds[lane] + lds[lane + stride];
            __syncthreads();
        }
        total[i] = lds[0];
        __syncthreads();
    }
    if (lane != 0) return;
    HornEigen h;
    horn_jacobi(total, h);
    double top = h.b00;
    if (h.b11 > top) top = h.b11;
    if (h.b22 > top) top = h.b22;
    if (h.b33 > top) top = h.b33;
    double S = (total[9] - 2.0 * top) / (double)J;
    if (S < 0.0) S = 0.0;
    int n = (int)total[10];                                              // (whole numbers below 2^31: exact)
    if (!finite_double(top) || !finite_double(S)) { S = 0.0; n = 0; }
    sums[(long)p * M + q] = S;
    sums[(long)q * M + p] = S;
    terms[(long)p * M + q] = n;
    terms[(long)q * M + p] = n;
}

}  // namespace uu3d
