// uu3d_attn_long.h -- exact-f32 softmax attention for the training step over sequences of more than 128 tokens
// (up to ATTN_LONG_MAX_L = 416), head dim 48: a tiled forward that saves per-row softmax statistics and a tiled backward
// that recomputes P from them.  The <= 128-token training kernels (attn_f32_kernel, attn_bwd_mfma_kernel) hold a whole
// sequence's tiles in registers; these walk the other operand in chunks of 64 rows staged through LDS instead.
//
// Arithmetic of the <= 128-token kernels: v_mfma_f32_16x16x4_f32 (exact f32), logits = fma(QK^T, 1/sqrt(d_h), madd) with
// madd = (1 - mask) * -1e9 (finite) and -inf only on the zero padding past L, exp as exp2 of a prescaled argument.
// Statistics are the row max m and the row sum l = sum exp(v - m), kept SEPARATELY (float2 {m, l} per (sequence, head,
// query) row, [B][H][L]): in a sequence whose keys are all masked every logit rounds to exactly -1e9, v - m is exactly 0 and
// P exactly uniform, as in the other kernels; exp(v - LSE) with an LSE near -1e9 (f32 spacing 64) would not be.
//
// Workgroup = 4 waves = 4 tiles of 16 rows of one (sequence, head); every wave keeps its tile's operands and accumulators in
// registers while the workgroup walks the other side in chunks of 64 rows (LDS: two 64 x (d_h + 4) images + row constants,
// at most 27.4 KB, static -- below the 64 KiB default, so no hipFuncSetAttribute).  The next chunk is loaded into registers while the
// current one is computed.  Every output element has exactly one writer: no atomics, bitwise reproducible.
//   attn_long_fwd_kernel   wave = query tile: S^T = K Q^T lands as [query = lane & 15][key = 16 j + 4 g + r], online softmax
//                          over the chunks (the P V trick of attn_f32_kernel: the probabilities are the A operand as they stand).
//   attn_long_dq_kernel    wave = query tile: S^T and dP^T = V dO^T per key tile, P from the statistics, dS = P (dP - delta),
//                          dQ += dS K.
//   attn_long_dkv_kernel   wave = key tile: S and dP in the other orientation, [key = lane & 15][query = 16 j + 4 g + r];
//                          dK += dS^T Q, dV += P^T dO.
// delta = rowsum(dO o O) is formed by each backward kernel from O and dO as it loads them (no extra buffer, no pre-pass).
// Inference: attn_long_fwd_kernel<48, false>, the forward without the statistics, is the attention of an exact-f32 forward call
// (UU3D_SCHEDULE_EXACT_F32) above 128 tokens -- attn_choose / launch_attn_infer in uu3d_launch.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "uu3d_gemm.h"

namespace uu3d {

constexpr int ATTN_LONG_MAX_L = 416;     // 26 tiles of 16: the longest sequence the training step takes (the f16x3 inference kernel's limit)
constexpr int ATTN_LONG_WAVES = 4;       // tiles per workgroup = rows per staged chunk / 16

namespace attn_long {
constexpr int W = ATTN_LONG_WAVES, CR = 16 * W;
constexpr float kLog2e = 1.44269504088896341f;

// staging of one chunk of CR rows: thread = (row tid >> 2, channels 12 (tid & 3) .. + 12) -> three float4 per matrix
__device__ inline int clamp_row(int row, int L) { return row < L ? row : L - 1; }
__device__ inline void load3(const float* p, f32x4 (&v)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) v[i] = *reinterpret_cast<const f32x4*>(p + 4 * i);
}
__device__ inline void store3(float* p, const f32x4 (&v)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) *reinterpret_cast<f32x4*>(p + 4 * i) = v[i];
}
// the additive key mask of key `key` of sequence b: 0 / -1e9 (masked) / -inf (padding past L)
__device__ inline float key_add(const uint8_t* key_mask, int b, int key, int L) {
    if (key >= L) return -INFINITY;
    return (key_mask != nullptr) ? (key_mask[(size_t)b * L + key] ? 0.0f : 1.0f) * -1e9f : 0.0f;
}
// the statistics argument of attn_long_fwd_kernel<DH, STATS>: the [B][H][L] {max, sum} buffer, or nothing at all
struct NoStats {};
template <bool STATS> struct StatsArg { using type = float2* __restrict__; };
template <> struct StatsArg<false> { using type = NoStats; };
template <bool STATS> using stats_arg_t = typename StatsArg<STATS>::type;
}  // namespace attn_long

// O (f32, row stride ldo, head h at channels h * 48) and stats[(b H + h) L + q] = {row max, row sum}.
// grid (B * H, ceil(NT / 4)), block 256.
// STATS = false: the inference instantiation (the exact-f32 forward above 128 tokens, launch_attn_infer) -- the statistics are what only
// the backward reads, so the last argument is an empty attn_long::NoStats instead of a pointer and nothing is stored for it; the body,
// and with it every bit of O, is the training instantiation's.
template <int DH, bool STATS = true>
__global__ void __launch_bounds__(64 * ATTN_LONG_WAVES)
attn_long_fwd_kernel(const float* __restrict__ qkv, const int ld, const int D, const int L, const int H,
                     const uint8_t* __restrict__ key_mask, float* __restrict__ out, const int ldo, attn_long::stats_arg_t<STATS> stats)
{
    using namespace attn_long;
    static_assert(DH == 48, "staging: four threads of 12 channels per row");
    constexpr int LD = DH + 4, KT = DH / 16;
    __shared__ __attribute__((aligned(16))) float Ks[CR * LD];
    __shared__ __attribute__((aligned(16))) float Vs[CR * LD];
    __shared__ float Ma[CR];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, qi = lane & 15, g = lane >> 4;
    const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
    const int NT = (L + 15) / 16, qt = (int)blockIdx.y * W + w;
    const bool active = qt < NT;                          // wave-uniform; idle waves still stage and meet the barriers
    const float* base = qkv + (size_t)b * L * ld + h * DH;
    const int srow = tid >> 2, sc = 12 * (tid & 3);

    f32x4 qf[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t)                          // query rows past L: a copy of the last row, never stored
        qf[t] = *reinterpret_cast<const f32x4*>(base + (size_t)clamp_row(16 * qt + qi, L) * ld + 16 * t + 4 * g);

    f32x4 kr[3], vr[3]; float mr;
    auto fetch = [&](int c0) {
        const int row = c0 + srow;
        const float* p = base + (size_t)clamp_row(row, L) * ld + sc;
        load3(p + D, kr); load3(p + 2 * D, vr);
        mr = key_add(key_mask, b, row, L);
    };
    const float scale_mul = 1.0f / sqrtf((float)DH);
    float m_run = -INFINITY, l_run = 0.f;
    f32x4 ot[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) ot[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

    fetch(0);
    for (int c0 = 0; c0 < L; c0 += CR) {
        __syncthreads();
        store3(&Ks[srow * LD + sc], kr); store3(&Vs[srow * LD + sc], vr);
        if ((tid & 3) == 0) Ma[srow] = mr;
        __syncthreads();
        if (c0 + CR < L) fetch(c0 + CR);
        if (!active) continue;
        // S^T tiles of this chunk: st[j][r] = <Q[16 qt + qi], K[c0 + 16 j + 4 g + r]>
        f32x4 st[W];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            f32x4 a = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < KT; ++t) {
                const f32x4 kf = *reinterpret_cast<const f32x4*>(&Ks[(16 * j + qi) * LD + 16 * t + 4 * g]);
#pragma unroll
                for (int s = 0; s < 4; ++s) a = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[s], qf[t][s], a, 0, 0, 0);
            }
            st[j] = a;
        }
        float cmax = -INFINITY;
#pragma unroll
        for (int j = 0; j < W; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) { st[j][r] = fmaf(st[j][r], scale_mul, Ma[16 * j + 4 * g + r]); cmax = fmaxf(cmax, st[j][r]); }
        cmax = fmaxf(cmax, __shfl_xor(cmax, 16)); cmax = fmaxf(cmax, __shfl_xor(cmax, 32));
        const float m_new = fmaxf(m_run, cmax);           // finite: every chunk holds at least one key < L
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * kLog2e);       // 0 at the first chunk
        float csum = 0.f;
#pragma unroll
        for (int j = 0; j < W; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float e = __builtin_amdgcn_exp2f((st[j][r] - m_new) * kLog2e); st[j][r] = e; csum += e; }
        csum += __shfl_xor(csum, 16); csum += __shfl_xor(csum, 32);
        l_run = fmaf(l_run, alpha, csum); m_run = m_new;
        // the accumulator's row 4 g + r is query 4 g + r: its factor lives in lane 4 g + r
        float ar[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) ar[r] = __shfl(alpha, 4 * g + r);
#pragma unroll
        for (int t = 0; t < KT; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) ot[t][r] *= ar[r];
#pragma unroll
            for (int j = 0; j < W; ++j)
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    ot[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(st[j][s], Vs[(16 * j + 4 * g + s) * LD + 16 * t + qi], ot[t], 0, 0, 0);
        }
    }
    if (!active) return;
    const float rl = 1.0f / l_run;
    float rr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) rr[r] = __shfl(rl, 4 * g + r);
    // C/D map: col = lane & 15 -> channel, row = 4 g + r -> query
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = 16 * qt + 4 * g + r;
            if (q < L) out[((size_t)b * L + q) * ldo + h * DH + 16 * t + qi] = ot[t][r] * rr[r];
        }
    if constexpr (STATS) {
        const int q = 16 * qt + qi;
        if (g == 0 && q < L) stats[(size_t)bh * L + q] = make_float2(m_run, l_run);
    }
}

// dQ into dqkv (the layout and row stride ld of qkv, channels h * 48 of the q third).  grid (B * H, ceil(NT / 4)), block 256.
template <int DH>
__global__ void __launch_bounds__(64 * ATTN_LONG_WAVES)
attn_long_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ O, const float* __restrict__ dO, const float2* __restrict__ stats,
                    const int ld, const int D, const int L, const int H, const uint8_t* __restrict__ key_mask,
                    float* __restrict__ dqkv, const int ldo)
{
    using namespace attn_long;
    static_assert(DH == 48, "staging: four threads of 12 channels per row");
    constexpr int LD = DH + 4, KT = DH / 16;
    __shared__ __attribute__((aligned(16))) float Ks[CR * LD];
    __shared__ __attribute__((aligned(16))) float Vs[CR * LD];
    __shared__ float Ma[CR];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, qi = lane & 15, g = lane >> 4;
    const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
    const int NT = (L + 15) / 16, qt = (int)blockIdx.y * W + w;
    const bool active = qt < NT;
    const float* base = qkv + (size_t)b * L * ld + h * DH;
    const int srow = tid >> 2, sc = 12 * (tid & 3);

    // this lane's query 16 qt + qi: Q and dO as B operands, its statistics, delta = <dO, O> (12 channels per lane, then across g)
    const int qrow = clamp_row(16 * qt + qi, L);
    f32x4 qf[KT], gf[KT];
    float delta = 0.f;
#pragma unroll
    for (int t = 0; t < KT; ++t) {
        qf[t] = *reinterpret_cast<const f32x4*>(base + (size_t)qrow * ld + 16 * t + 4 * g);
        const size_t o = ((size_t)b * L + qrow) * ldo + h * DH + 16 * t + 4 * g;
        gf[t] = *reinterpret_cast<const f32x4*>(dO + o);
        const f32x4 of = *reinterpret_cast<const f32x4*>(O + o);
#pragma unroll
        for (int s = 0; s < 4; ++s) delta = fmaf(gf[t][s], of[s], delta);
    }
    delta += __shfl_xor(delta, 16); delta += __shfl_xor(delta, 32);
    const float2 sv = stats[(size_t)bh * L + qrow];
    const float m_q = sv.x, rl_q = 1.0f / sv.y;

    f32x4 kr[3], vr[3]; float mr;
    auto fetch = [&](int c0) {
        const int row = c0 + srow;
        const float* p = base + (size_t)clamp_row(row, L) * ld + sc;
        load3(p + D, kr); load3(p + 2 * D, vr);
        mr = key_add(key_mask, b, row, L);
    };
    const float scale_mul = 1.0f / sqrtf((float)DH);
    f32x4 dq[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) dq[t] = (f32x4){0.f, 0.f, 0.f, 0.f};

    fetch(0);
    for (int c0 = 0; c0 < L; c0 += CR) {
        __syncthreads();
        store3(&Ks[srow * LD + sc], kr); store3(&Vs[srow * LD + sc], vr);
        if ((tid & 3) == 0) Ma[srow] = mr;
        __syncthreads();
        if (c0 + CR < L) fetch(c0 + CR);
        if (!active) continue;
        f32x4 ds[W];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f}, d = a;
#pragma unroll
            for (int t = 0; t < KT; ++t) {
                const f32x4 kf = *reinterpret_cast<const f32x4*>(&Ks[(16 * j + qi) * LD + 16 * t + 4 * g]);
                const f32x4 vf = *reinterpret_cast<const f32x4*>(&Vs[(16 * j + qi) * LD + 16 * t + 4 * g]);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    a = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[s], qf[t][s], a, 0, 0, 0);      // S^T[key 16j+4g+r][query qi]
                    d = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[s], gf[t][s], d, 0, 0, 0);      // dP^T
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f((fmaf(a[r], scale_mul, Ma[16 * j + 4 * g + r]) - m_q) * kLog2e) * rl_q;
                ds[j][r] = p * (d[r] - delta);
            }
        }
#pragma unroll
        for (int t = 0; t < KT; ++t)
#pragma unroll
            for (int j = 0; j < W; ++j)
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    dq[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ds[j][s], Ks[(16 * j + 4 * g + s) * LD + 16 * t + qi], dq[t], 0, 0, 0);
    }
    if (!active) return;
    float* dq_out = dqkv + (size_t)b * L * ld + h * DH;
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = 16 * qt + 4 * g + r;
            if (q < L) dq_out[(size_t)q * ld + 16 * t + qi] = dq[t][r] * scale_mul;
        }
}

// dK and dV into dqkv (k and v thirds).  grid (B * H, ceil(NT / 4)), block 256.
template <int DH>
__global__ void __launch_bounds__(64 * ATTN_LONG_WAVES)
attn_long_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ O, const float* __restrict__ dO, const float2* __restrict__ stats,
                     const int ld, const int D, const int L, const int H, const uint8_t* __restrict__ key_mask,
                     float* __restrict__ dqkv, const int ldo)
{
    using namespace attn_long;
    static_assert(DH == 48, "staging: four threads of 12 channels per row");
    constexpr int LD = DH + 4, KT = DH / 16;
    __shared__ __attribute__((aligned(16))) float Qs[CR * LD];
    __shared__ __attribute__((aligned(16))) float Gs[CR * LD];
    __shared__ float Mx[CR], Rl[CR], Dl[CR];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, qi = lane & 15, g = lane >> 4;
    const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
    const int NT = (L + 15) / 16, kt = (int)blockIdx.y * W + w;
    const bool active = kt < NT;
    const float* base = qkv + (size_t)b * L * ld + h * DH;
    const int srow = tid >> 2, sc = 12 * (tid & 3);

    // this lane's key 16 kt + qi: K and V as B operands and its additive mask
    const int key = 16 * kt + qi;
    f32x4 kf[KT], vf[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) {
        const float* p = base + (size_t)clamp_row(key, L) * ld + 16 * t + 4 * g;
        kf[t] = *reinterpret_cast<const f32x4*>(p + D);
        vf[t] = *reinterpret_cast<const f32x4*>(p + 2 * D);
    }
    const float madd = key_add(key_mask, b, key, L);

    // staged per query row: Q, dO, and (m, 1 / l, delta).  Rows past L are copies of row L - 1 WITH its row max, so that exp2 stays
    // <= 1 (finite) for any logit, and get 1 / l = 0, delta = 0: P = dS = 0 exactly.  (A max of 0 there made exp2 overflow to +inf
    // for logits above ~88.7, and inf * 0 = NaN in dK / dV.)
    f32x4 qr[3], gr[3]; float mr, rlr, dlr;
    auto fetch = [&](int c0) {
        const int row = c0 + srow, cr = clamp_row(row, L);
        load3(base + (size_t)cr * ld + sc, qr);
        const size_t o = ((size_t)b * L + cr) * ldo + h * DH + sc;
        load3(dO + o, gr);
        f32x4 orow[3]; load3(O + o, orow);
        float dl = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int s = 0; s < 4; ++s) dl = fmaf(gr[i][s], orow[i][s], dl);
        dl += __shfl_xor(dl, 1); dl += __shfl_xor(dl, 2);
        const float2 sv = stats[(size_t)bh * L + cr];
        mr = sv.x; rlr = row < L ? 1.0f / sv.y : 0.f; dlr = row < L ? dl : 0.f;
    };
    const float scale_mul = 1.0f / sqrtf((float)DH);
    f32x4 dk[KT], dv[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) { dk[t] = (f32x4){0.f, 0.f, 0.f, 0.f}; dv[t] = dk[t]; }

    fetch(0);
    for (int c0 = 0; c0 < L; c0 += CR) {
        __syncthreads();
        store3(&Qs[srow * LD + sc], qr); store3(&Gs[srow * LD + sc], gr);
        if ((tid & 3) == 0) { Mx[srow] = mr; Rl[srow] = rlr; Dl[srow] = dlr; }
        __syncthreads();
        if (c0 + CR < L) fetch(c0 + CR);
        if (!active) continue;
        // one query tile at a time: its P and dS feed dK / dV at once (all four tiles' P and dS live together cost 260 VGPRs)
#pragma unroll
        for (int j = 0; j < W; ++j) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f}, d = a;
#pragma unroll
            for (int t = 0; t < KT; ++t) {
                const f32x4 qa = *reinterpret_cast<const f32x4*>(&Qs[(16 * j + qi) * LD + 16 * t + 4 * g]);
                const f32x4 ga = *reinterpret_cast<const f32x4*>(&Gs[(16 * j + qi) * LD + 16 * t + 4 * g]);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    a = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[s], kf[t][s], a, 0, 0, 0);      // S[query 16j+4g+r][key qi]
                    d = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[s], vf[t][s], d, 0, 0, 0);      // dP
                }
            }
            f32x4 pp, ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = 16 * j + 4 * g + r;
                const float p = __builtin_amdgcn_exp2f((fmaf(a[r], scale_mul, madd) - Mx[q]) * kLog2e) * Rl[q];
                pp[r] = p; ds[r] = p * (d[r] - Dl[q]);
            }
#pragma unroll
            for (int t = 0; t < KT; ++t)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    dk[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ds[s], Qs[(16 * j + 4 * g + s) * LD + 16 * t + qi], dk[t], 0, 0, 0);
                    dv[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(pp[s], Gs[(16 * j + 4 * g + s) * LD + 16 * t + qi], dv[t], 0, 0, 0);
                }
        }
    }
    if (!active) return;
    float* dk_out = dqkv + (size_t)b * L * ld + D + h * DH;
    float* dv_out = dk_out + D;
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int kr = 16 * kt + 4 * g + r;
            if (kr < L) { dk_out[(size_t)kr * ld + 16 * t + qi] = dk[t][r] * scale_mul; dv_out[(size_t)kr * ld + 16 * t + qi] = dv[t][r]; }
        }
}

template <int DH>
constexpr size_t attn_long_lds_bytes() { return (2 * (size_t)attn_long::CR * (DH + 4) + 3 * attn_long::CR) * sizeof(float); }

}  // namespace uu3d
