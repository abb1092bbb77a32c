// Evaluation report on the device: per-pose MPJPE / N-MPJPE / P-MPJPE in float64 with the keyframe interpolation
// fused into the load, and the per-action sums of the report.
//
//   evaluation._frame_metrics          -> pose_errors_kernel (one lane per pose)
//   interpolate_between_keyframes      -> the (left, right, weight) plan read by the staging loop; the interpolated pose lives in LDS only
//   h36_action_wise_eval / frame_wise_eval sums -> met_accumulate (ordered, per workgroup) + error_sums_combine_kernel (ordered, one workgroup)
//
// A workgroup is ONE wave.  A tile of up to 64 poses is staged through LDS with coalesced loads (a pose is J*3 contiguous numbers, so a lane
// reading its own pose from memory would touch 64 different lines per load); then lane p walks pose p.  Row strides in LDS are odd numbers of
// 8-byte (prediction) and 4-byte (ground truth) words: conflict-free walks.  Registers hold the two means, the nine cross-covariance sums, the
// norms and the 3x3 factorisation; nothing per joint.
//
// The similarity fit (metrics.py:136-201) needs the SVD A = U S V^T of the 3x3 cross-covariance.  Here: cyclic Jacobi on A^T A (8 sweeps,
// branch-free: a zero off-diagonal element selects the identity rotation) gives V and the squared singular values; the column of the smallest
// one goes last, u1 = A v1 / |A v1|, u2 = A v2 / |A v2| and w = u1 x u2.  Whatever sign LAPACK would give u3 = +-w, the reference's
//     T = V diag(1, 1, sign det(V U^T)) U^T   equals   v1 u1^T + v2 u2^T + det(V) v3 w^T      and
//     trace = s1 + s2 + sign * s3             equals   |A v1| + |A v2| + det(V) (w . A v3),
// so the smallest singular value is never divided by.  A rank-1 covariance (collinear pose) gives 0 / 0 in u2 and takes the raw-prediction
// fallback of evaluation.pmpjpe, as does a pose of zero extent.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kMetLanes = 64;            // poses per tile at most = lanes of the workgroup
constexpr int kMetMaxJoints = 32;        // the valid flags of a pose are one 32-bit mask
constexpr int kMetMaxActions = 63;       // (actions + 1) * 3 table cells, three per lane at most
constexpr int kMetMaxCells = (kMetMaxActions + 1) * 3;
constexpr int kMetMaxGrid = 1536;        // workgroups (and rows of the partial-sums scratch); tiles are dealt round-robin
constexpr int kMetSkip = -2;             // s.act: the pose is not part of the report (not selected, or beyond the end)

struct MetTables {
    double ps[kMetLanes * 6];            // per pose: (sum of errors >= 0, their count) x 3 metrics
    int act[kMetLanes];
    double tab[kMetMaxCells * 2];        // the workgroup's running (sum, count) per (action | all, metric)
};

// A launch gets 64 KiB of LDS without opt-in, static and dynamic together: the tile's dynamic part takes what the 6400 bytes of MetTables leave.
constexpr int kMetLdsBudget = 64 * 1024 - (int)sizeof(MetTables);
static_assert(sizeof(MetTables) == 6400 && kMetLdsBudget + sizeof(MetTables) <= 64 * 1024, "static + dynamic LDS of a launch");

// Adds the tile's per-pose sums into the workgroup's table: cell (a, m) is owned by one lane, which walks the poses in order.
static __device__ __forceinline__ void met_accumulate(MetTables& s, const int n, const int A, const int tid)
{
    const int cells = (A + 1) * 3;
    for (int cell = tid; cell < cells; cell += kMetLanes) {
        const int a = cell / 3, m = cell - a * 3;
        double sum = s.tab[cell * 2], cnt = s.tab[cell * 2 + 1];
        for (int p = 0; p < n; ++p) {
            const int ap = s.act[p];
            const bool take = ap != kMetSkip && (a == A || ap == a);
            sum += take ? s.ps[p * 6 + m * 2] : 0.0;
            cnt += take ? s.ps[p * 6 + m * 2 + 1] : 0.0;
        }
        s.tab[cell * 2] = sum;
        s.tab[cell * 2 + 1] = cnt;
    }
}

static __device__ __forceinline__ void met_tables_begin(MetTables& s, const int A, const int tid)
{
    for (int i = tid; i < (A + 1) * 6; i += kMetLanes) s.tab[i] = 0.0;
}

static __device__ __forceinline__ void met_tables_end(const MetTables& s, const int A, const int tid, double* __restrict__ partial)
{
    const int n = (A + 1) * 6;
    for (int i = tid; i < n; i += kMetLanes) partial[(size_t)blockIdx.x * n + i] = s.tab[i];
}

// One Jacobi rotation of the symmetric 3x3 matrix (diagonal bpp, bqq; element bpq; the two elements brp, brq of the third row) and of the
// eigenvector columns p, q.  t = tan of the rotation angle, the smaller root; bpq == 0 rotates by nothing.
#define UU3D_JACOBI_ROT(bpp, bqq, bpq, brp, brq, v0p, v0q, v1p, v1q, v2p, v2q)                      \
    {                                                                                               \
        const double th = (bqq - bpp) / (2.0 * bpq);                                                \
        const double tt = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));              \
        const double t = (bpq == 0.0) ? 0.0 : tt;                                                   \
        const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;                                       \
        bpp -= t * bpq; bqq += t * bpq; bpq = 0.0;                                                  \
        double x_ = brp, y_ = brq; brp = c * x_ - sn * y_; brq = sn * x_ + c * y_;                  \
        x_ = v0p; y_ = v0q; v0p = c * x_ - sn * y_; v0q = sn * x_ + c * y_;                         \
        x_ = v1p; y_ = v1q; v1p = c * x_ - sn * y_; v1q = sn * x_ + c * y_;                         \
        x_ = v2p; y_ = v2q; v2p = c * x_ - sn * y_; v2q = sn * x_ + c * y_;                         \
    }

#define UU3D_CSWAP(cond, a, b) { const double a_ = a, b_ = b; a = (cond) ? b_ : a_; b = (cond) ? a_ : b_; }

// pred (R, J, 3), gt (P, J, C) of type T (float: the product path; double: poses that exist in float64 only, e.g. the reference's fixtures).
// Pose i = pred[left[i]] * (1 - weight[i]) + pred[right[i]] * weight[i]  (left NULL: row i; weight NULL: pred[left[i]]).
// errors (P, J, 3) or NULL: (mpjpe, nmpjpe, pmpjpe) in metres, -1 at invalid joints and in poses that `select` leaves out.
// partial (gridDim.x, A + 1, 3, 2) or NULL.
template <typename T>
static __global__ void __launch_bounds__(kMetLanes)
pose_errors_kernel(const T* __restrict__ pred, const long R, const int* __restrict__ left, const int* __restrict__ right,
                   const double* __restrict__ weight, const T* __restrict__ gt, const long P, const int J, const int C, const int root,
                   const int ppb, const int gstride, double* __restrict__ errors, const int* __restrict__ actions, const int A,
                   const uint8_t* __restrict__ select, double* __restrict__ partial)
{
    extern __shared__ double met_lds[];
    __shared__ MetTables s;
    const int tid = threadIdx.x;
    const int J3 = J * 3, JC = J * C;
    const int pstride = J3 | 1;                                   // doubles per staged prediction
    double* Pd = met_lds;
    T* Gs = reinterpret_cast<T*>(met_lds + (size_t)ppb * pstride);
    const long tiles = (P + ppb - 1) / ppb;
    const double nan = __builtin_nan("");
    if (partial) met_tables_begin(s, A, tid);

    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long base = tile * ppb;
        const int n = (int)min((long)ppb, P - base);
        __syncthreads();                                          // (the previous tile's stores and sums are done with LDS)
        // ---- stage: predictions (gathered rows, interpolated in float64) and ground truth (one contiguous block) ----
#pragma unroll 4
        for (int idx = tid; idx < n * J3; idx += kMetLanes) {
            const int p = idx / J3, e = idx - p * J3;
            const long pose = base + p;
            double v = 0.0;
            if (!select || select[pose]) {
                const long l = left ? (long)left[pose] : pose;
                const long r = (weight && right) ? (long)right[pose] : l;
                const double w = weight ? weight[pose] : 0.0;
                if (l < 0 || l >= R || r < 0 || r >= R) v = nan;          // a row that does not exist: the pose drops out of every mean
                else if (r == l || w == 0.0) v = (double)pred[l * J3 + e];
                else v = (double)pred[l * J3 + e] * (1.0 - w) + (double)pred[r * J3 + e] * w;     // action_wise_eval.py:94
            }
            Pd[p * pstride + e] = v;
        }
#pragma unroll 4
        for (int idx = tid; idx < n * JC; idx += kMetLanes) {
            const int p = idx / JC, e = idx - p * JC;
            Gs[p * gstride + e] = gt[base * JC + idx];
        }
        __syncthreads();

        // ---- lane p: pose p ----
        const long pose = base + tid;
        const bool live = tid < n && (!select || select[pose]);
        double sum[3] = {0.0, 0.0, 0.0}, cnt[3] = {0.0, 0.0, 0.0};
        if (tid < n) {
            double* Pp = Pd + tid * pstride;
            const T* G = Gs + tid * gstride;
            if (!live) {
                for (int e = 0; e < J3; ++e) Pp[e] = -1.0;
            } else {
                // means over all joints, valid flags
                uint32_t vmask = 0;
                double mp0 = 0, mp1 = 0, mp2 = 0, mg0 = 0, mg1 = 0, mg2 = 0;
                for (int j = 0; j < J; ++j) {
                    mp0 += Pp[j * 3]; mp1 += Pp[j * 3 + 1]; mp2 += Pp[j * 3 + 2];
                    mg0 += (double)G[j * C]; mg1 += (double)G[j * C + 1]; mg2 += (double)G[j * C + 2];
                    const bool ok = C == 4 ? (G[j * C + 3] > (T)0) : true;
                    vmask |= (ok ? 1u : 0u) << j;
                }
                const double rj = (double)J;
                mp0 /= rj; mp1 /= rj; mp2 /= rj; mg0 /= rj; mg1 /= rj; mg2 /= rj;
                const double pr0 = Pp[root * 3], pr1 = Pp[root * 3 + 1], pr2 = Pp[root * 3 + 2];
                const double gr0 = (double)G[root * C], gr1 = (double)G[root * C + 1], gr2 = (double)G[root * C + 2];
                // cross-covariance of the centred poses, their norms; the sums of the optimal scale over valid joints (metrics.py:120-133)
                double a00 = 0, a01 = 0, a02 = 0, a10 = 0, a11 = 0, a12 = 0, a20 = 0, a21 = 0, a22 = 0, nx = 0, ny = 0, num = 0, den = 0;
                for (int j = 0; j < J; ++j) {
                    const double p0 = Pp[j * 3], p1 = Pp[j * 3 + 1], p2 = Pp[j * 3 + 2];
                    const double g0 = (double)G[j * C], g1 = (double)G[j * C + 1], g2 = (double)G[j * C + 2];
                    const double y0 = p0 - mp0, y1 = p1 - mp1, y2 = p2 - mp2, x0 = g0 - mg0, x1 = g1 - mg1, x2 = g2 - mg2;
                    nx += x0 * x0 + x1 * x1 + x2 * x2;
                    ny += y0 * y0 + y1 * y1 + y2 * y2;
                    a00 += x0 * y0; a01 += x0 * y1; a02 += x0 * y2;
                    a10 += x1 * y0; a11 += x1 * y1; a12 += x1 * y2;
                    a20 += x2 * y0; a21 += x2 * y1; a22 += x2 * y2;
                    const double m = (vmask >> j) & 1u ? 1.0 : 0.0;
                    const double dp0 = (p0 - pr0) * m, dp1 = (p1 - pr1) * m, dp2 = (p2 - pr2) * m;
                    num += dp0 * ((g0 - gr0) * m) + dp1 * ((g1 - gr1) * m) + dp2 * ((g2 - gr2) * m);
                    den += dp0 * dp0 + dp1 * dp1 + dp2 * dp2;
                }
                const double s_opt = num / den;                                   // 0 / 0 = NaN as on the host
                const double normX = sqrt(nx), normY = sqrt(ny);
                const double rx = 1.0 / normX, ry = 1.0 / normY;
                a00 = a00 * rx * ry; a01 = a01 * rx * ry; a02 = a02 * rx * ry;
                a10 = a10 * rx * ry; a11 = a11 * rx * ry; a12 = a12 * rx * ry;
                a20 = a20 * rx * ry; a21 = a21 * rx * ry; a22 = a22 * rx * ry;
                // B = A^T A, V = eigenvectors (columns)
                double b00 = a00 * a00 + a10 * a10 + a20 * a20, b11 = a01 * a01 + a11 * a11 + a21 * a21, b22 = a02 * a02 + a12 * a12 + a22 * a22;
                double b01 = a00 * a01 + a10 * a11 + a20 * a21, b02 = a00 * a02 + a10 * a12 + a20 * a22, b12 = a01 * a02 + a11 * a12 + a21 * a22;
                double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;
#pragma unroll 1
                for (int sweep = 0; sweep < 8; ++sweep) {
                    UU3D_JACOBI_ROT(b00, b11, b01, b02, b12, v00, v01, v10, v11, v20, v21)
                    UU3D_JACOBI_ROT(b00, b22, b02, b01, b12, v00, v02, v10, v12, v20, v22)
                    UU3D_JACOBI_ROT(b11, b22, b12, b01, b02, v01, v02, v11, v12, v21, v22)
                }
                // the column of the smallest eigenvalue goes last
                const bool sw0 = b00 < b22;
                UU3D_CSWAP(sw0, b00, b22) UU3D_CSWAP(sw0, v00, v02) UU3D_CSWAP(sw0, v10, v12) UU3D_CSWAP(sw0, v20, v22)
                const bool sw1 = b11 < b22;
                UU3D_CSWAP(sw1, b11, b22) UU3D_CSWAP(sw1, v01, v02) UU3D_CSWAP(sw1, v11, v12) UU3D_CSWAP(sw1, v21, v22)
                // u_i = A v_i / |A v_i| (i = 1, 2), w = u1 x u2
                double u10 = a00 * v00 + a01 * v10 + a02 * v20, u11 = a10 * v00 + a11 * v10 + a12 * v20, u12 = a20 * v00 + a21 * v10 + a22 * v20;
                double u20 = a00 * v01 + a01 * v11 + a02 * v21, u21 = a10 * v01 + a11 * v11 + a12 * v21, u22 = a20 * v01 + a21 * v11 + a22 * v21;
                const double z0 = a00 * v02 + a01 * v12 + a02 * v22, z1 = a10 * v02 + a11 * v12 + a12 * v22, z2 = a20 * v02 + a21 * v12 + a22 * v22;
                const double s1 = sqrt(u10 * u10 + u11 * u11 + u12 * u12), s2 = sqrt(u20 * u20 + u21 * u21 + u22 * u22);
                const double r1 = 1.0 / s1, r2 = 1.0 / s2;
                u10 *= r1; u11 *= r1; u12 *= r1; u20 *= r2; u21 *= r2; u22 *= r2;
                const double w0 = u11 * u22 - u12 * u21, w1 = u12 * u20 - u10 * u22, w2 = u10 * u21 - u11 * u20;
                const double detV = v00 * (v11 * v22 - v12 * v21) - v01 * (v10 * v22 - v12 * v20) + v02 * (v10 * v21 - v11 * v20);
                const double d = detV >= 0.0 ? 1.0 : -1.0;
                const double trace = s1 + s2 + d * (w0 * z0 + w1 * z1 + w2 * z2);
                // T[i][k] = v1[i] u1[k] + v2[i] u2[k] + d v3[i] w[k], scaled by normX * trace / normY  (Z = scale * (p - muY) T + muX)
                const double sc = normX * trace * ry;
                const double t00 = sc * (v00 * u10 + v01 * u20 + d * v02 * w0), t01 = sc * (v00 * u11 + v01 * u21 + d * v02 * w1), t02 = sc * (v00 * u12 + v01 * u22 + d * v02 * w2);
                const double t10 = sc * (v10 * u10 + v11 * u20 + d * v12 * w0), t11 = sc * (v10 * u11 + v11 * u21 + d * v12 * w1), t12 = sc * (v10 * u12 + v11 * u22 + d * v12 * w2);
                const double t20 = sc * (v20 * u10 + v21 * u20 + d * v22 * w0), t21 = sc * (v20 * u11 + v21 * u21 + d * v22 * w1), t22 = sc * (v20 * u12 + v21 * u22 + d * v22 * w2);
                // evaluation.pmpjpe: a pose whose aligned result is not finite keeps its raw prediction
                bool finite = true;
                for (int j = 0; j < J; ++j) {
                    const double y0 = Pp[j * 3] - mp0, y1 = Pp[j * 3 + 1] - mp1, y2 = Pp[j * 3 + 2] - mp2;
                    const double q0 = y0 * t00 + y1 * t10 + y2 * t20 + mg0, q1 = y0 * t01 + y1 * t11 + y2 * t21 + mg1, q2 = y0 * t02 + y1 * t12 + y2 * t22 + mg2;
                    finite = finite && __builtin_isfinite(q0) && __builtin_isfinite(q1) && __builtin_isfinite(q2);
                }
                for (int j = 0; j < J; ++j) {
                    const double p0 = Pp[j * 3], p1 = Pp[j * 3 + 1], p2 = Pp[j * 3 + 2];
                    const double g0 = (double)G[j * C], g1 = (double)G[j * C + 1], g2 = (double)G[j * C + 2];
                    const double dp0 = p0 - pr0, dp1 = p1 - pr1, dp2 = p2 - pr2, dg0 = g0 - gr0, dg1 = g1 - gr1, dg2 = g2 - gr2;
                    const double e0 = dp0 - dg0, e1 = dp1 - dg1, e2 = dp2 - dg2;
                    const double n0 = dp0 * s_opt - dg0, n1 = dp1 * s_opt - dg1, n2 = dp2 * s_opt - dg2;
                    const double y0 = p0 - mp0, y1 = p1 - mp1, y2 = p2 - mp2;
                    const double q0 = finite ? y0 * t00 + y1 * t10 + y2 * t20 + mg0 : p0;
                    const double q1 = finite ? y0 * t01 + y1 * t11 + y2 * t21 + mg1 : p1;
                    const double q2 = finite ? y0 * t02 + y1 * t12 + y2 * t22 + mg2 : p2;
                    const double f0 = q0 - g0, f1 = q1 - g1, f2 = q2 - g2;
                    const bool ok = (vmask >> j) & 1u;
                    const double em = ok ? sqrt(e0 * e0 + e1 * e1 + e2 * e2) : -1.0;
                    const double en = ok ? sqrt(n0 * n0 + n1 * n1 + n2 * n2) : -1.0;
                    const double ep = ok ? sqrt(f0 * f0 + f1 * f1 + f2 * f2) : -1.0;
                    sum[0] += em >= 0.0 ? em : 0.0; cnt[0] += em >= 0.0 ? 1.0 : 0.0;
                    sum[1] += en >= 0.0 ? en : 0.0; cnt[1] += en >= 0.0 ? 1.0 : 0.0;
                    sum[2] += ep >= 0.0 ? ep : 0.0; cnt[2] += ep >= 0.0 ? 1.0 : 0.0;
                    Pp[j * 3] = em; Pp[j * 3 + 1] = en; Pp[j * 3 + 2] = ep;           // (the pose's own slot: read above, never again)
                }
            }
        }
        if (partial) {
#pragma unroll
            for (int m = 0; m < 3; ++m) { s.ps[tid * 6 + m * 2] = sum[m]; s.ps[tid * 6 + m * 2 + 1] = cnt[m]; }
            s.act[tid] = live ? (actions ? actions[pose] : -1) : kMetSkip;
        }
        __syncthreads();
        if (errors) {
#pragma unroll 4
            for (int idx = tid; idx < n * J3; idx += kMetLanes) {
                const int p = idx / J3, e = idx - p * J3;
                errors[base * J3 + idx] = Pd[p * pstride + e];
            }
        }
        if (partial) met_accumulate(s, n, A, tid);
    }
    __syncthreads();
    if (partial) met_tables_end(s, A, tid, partial);
}

// The report sums of an error array (P, J, 3) that is already in memory: lane p sums pose p's entries >= 0, then as above.
// Tiles here are always 64 poses.  pose_errors_kernel takes 64 only while a pose fits 1/64 of the LDS budget (J = 17 in float32 does);
// larger poses are tiled smaller there, the sums then run in another order and agree with this kernel to rounding, not bit for bit.
static __global__ void __launch_bounds__(kMetLanes)
error_sums_kernel(const double* __restrict__ errors, const long P, const int J, const int* __restrict__ actions, const int A,
                  const uint8_t* __restrict__ select, double* __restrict__ partial)
{
    __shared__ MetTables s;
    const int tid = threadIdx.x;
    const int J3 = J * 3;
    const long tiles = (P + kMetLanes - 1) / kMetLanes;
    met_tables_begin(s, A, tid);
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long base = tile * kMetLanes;
        const int n = (int)min((long)kMetLanes, P - base);
        const long pose = base + tid;
        const bool live = tid < n && (!select || select[pose]);
        double sum[3] = {0.0, 0.0, 0.0}, cnt[3] = {0.0, 0.0, 0.0};
        if (live) {
            const double* e = errors + pose * J3;
            for (int j = 0; j < J; ++j) {
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    const double v = e[j * 3 + m];
                    sum[m] += v >= 0.0 ? v : 0.0;
                    cnt[m] += v >= 0.0 ? 1.0 : 0.0;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 3; ++m) { s.ps[tid * 6 + m * 2] = sum[m]; s.ps[tid * 6 + m * 2 + 1] = cnt[m]; }
        s.act[tid] = live ? (actions ? actions[pose] : -1) : kMetSkip;
        __syncthreads();
        met_accumulate(s, n, A, tid);
    }
    __syncthreads();
    met_tables_end(s, A, tid, partial);
}

// out[i] = partial[0][i] + partial[1][i] + ... in workgroup order: the one ordered combine.
static __global__ void __launch_bounds__(64)
error_sums_combine_kernel(const double* __restrict__ partial, const int blocks, const int n, double* __restrict__ out)
{
    for (int i = threadIdx.x; i < n; i += 64) {
        double acc = 0.0;
        for (int b = 0; b < blocks; ++b) acc += partial[(size_t)b * n + i];
        out[i] = acc;
    }
}
