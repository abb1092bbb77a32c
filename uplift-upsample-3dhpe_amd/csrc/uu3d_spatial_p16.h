// uu3d_spatial_p16.h -- the inference form of the f16x3 spatial stack on 16-token panels, activations kept in registers.
//
// Same function as spatial_stack_h3_kernel<J, 3, 1, false> (uu3d_spatial_h3.h): keypoint embedding + PE, 4 pre-LN blocks of 8-head
// attention over the 17 joints of a frame and a GELU MLP 32 -> 64 -> 32, spatial_norm, one launch.  Two changes of structure:
//
// * Dense frames on 16-token panels.  A workgroup holds FR whole frames packed back to back over NW waves of PW panels
//   (the library runs FR = 7, PW = 1: 119 tokens in 128 slots on 8 waves; the h3 kernel used 51 of 64).  A frame may straddle
//   two panels or two waves; every address of a token is relative to its frame, so a frame's result does not depend on where
//   in the workgroup it sits.
//   Spare slots run on finite values (a clamped frame) and store nothing.
//
// * No activation operand touches LDS.  Every product is transposed, C^T = W^T X^T on v_mfma_f32_16x16x32_f16 with the weight as
//   the A operand.  In the 16 x 16 result lane l = (t = l & 15, g = l >> 4) holds channels 4 g .. 4 g + 3 of token t: one head.
//   Two 16-channel tiles give the lane channels {4 g + r, 16 + 4 g + r}, exactly the 8 elements of its B fragment for the next
//   K = 32 product once the weights' k axis is packed in that order (p16_kch); the 64-wide hidden layer gives the 16 values of
//   fc2's two k-steps.  LayerNorm, residual stream, the hi / lo split and GELU stay in the lane; LayerNorm's moments cross the
//   4 lanes of a token with v_permlane16_swap + v_permlane32_swap.  Only K and V go through LDS (attention reads other tokens),
//   as f32 in the key-pair layout of sh3::head_attention, which runs here unchanged: lane (t, g) runs heads g and 4 + g.
//
// The LayerNorm parameters and biases of all blocks are copied into LDS once; a block then needs two barriers: one before its
// K / V stores (every wave is done reading the previous block's) and one after them.
//
// Toolchain rules of uu3d_spatial_h3.h / uu3d_pk.h hold here too: packed f32 by name only and never with op_sel (the kernel opts
// into the feature with UU3D_PK_TARGET), MFMA results fenced before inline-asm readers (20 wait states, more than the 11 an
// 8-pass 16x16x32 MFMA needs, behind every MFMA of the product), contraction off with every FMA written out.  The weight
// fragments are plain loads the compiler tracks (see load_w).
#pragma once
#include "uu3d_spatial_h3.h"

namespace uu3d {

// f16 fragment planes of one block, in halfs: per matrix [n-tile 16][k-step 32][plane hi/lo][lane][8],
// element j of lane l = split(W[p16_kch(s, l >> 4, j)][16 nt + (l & 15)]) of the Keras (in, out) kernel
struct SpatialFragLayoutP16 {
    static constexpr int frag = 64 * 8;                       // halfs per (n-tile, k-step, plane)
    static constexpr int fq = 0, fk = fq + 2 * 1 * 2 * frag, fv = fk + 2 * 1 * 2 * frag, fp = fv + 2 * 1 * 2 * frag;
    static constexpr int f1 = fp + 2 * 1 * 2 * frag;          // 32 -> 64: 4 n-tiles x 1 k-step
    static constexpr int f2 = f1 + 4 * 1 * 2 * frag;          // 64 -> 32: 2 n-tiles x 2 k-steps
    static constexpr int size = f2 + 2 * 2 * 2 * frag;        // 16384 halfs = 32 KiB per block
};
// input channel of element j of lane group g in k-step s: the channel the previous stage's accumulators hold there
__host__ __device__ inline constexpr int p16_kch(int s, int g, int j) { return 32 * s + 16 * (j >> 2) + 4 * g + (j & 3); }
// waves of a workgroup of FR frames of J tokens on PW panels per wave
__host__ __device__ inline constexpr int p16_waves(int J, int FR, int PW) { return (J * FR + 16 * PW - 1) / (16 * PW); }

namespace sp16 {
constexpr int NPARAM = sh3::NPARAM;                           // LayerNorm parameters and biases of one block (floats)
constexpr int KFLD = 9 * sh3::KPLD + sh3::KFPAD;              // floats per frame of the K (and of the V) image
template <int FR>
__host__ __device__ inline constexpr size_t lds_bytes(int depth) { return (size_t)2 * FR * KFLD * 4 + (size_t)depth * NPARAM * 4; }

template <int NT, int KS>
struct WF { h16x8 h[NT][KS], l[NT][KS]; };
// Plain loads the compiler counts itself, fragment (nt, s) plane p at ((nt KS + s) 2 + p) 64 + lane (the order of sh3::load_w).
// Loads issued by name with counted waits, as uu3d_spatial_h3.h does, went wrong here: hipcc took the destination registers of
// an in-flight load for temporaries (they count as written at the end of the asm statement), and the landing data overwrote
// LayerNorm arithmetic -- small, run-to-run varying errors.
template <int NT, int KS>
__device__ __forceinline__ void load_w(const _Float16* __restrict__ wf, const int lane, WF<NT, KS>& w) {
    const h16x8* base = reinterpret_cast<const h16x8*>(wf) + lane;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            w.h[nt][s] = base[((nt * KS + s) * 2 + 0) * 64];
            w.l[nt][s] = base[((nt * KS + s) * 2 + 1) * 64];
        }
}

// the lane's 8 values of k-step s (pairs v[4 s] .. v[4 s + 3]) -> its hi / lo B fragments
__device__ __forceinline__ void frag_of(const f32x2* v, h16x8& bh, h16x8& bl) {
    h16x4 h0, l0, h1, l1;
    sh3::split_pairs(v[0], v[1], h0, l0);
    sh3::split_pairs(v[2], v[3], h1, l1);
    bh = (h16x8){h0[0], h0[1], h0[2], h0[3], h1[0], h1[1], h1[2], h1[3]};
    bl = (h16x8){l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
    // A VALU write of an MFMA's A / B operand needs 2 wait states before the MFMA reads it.  The split writes these registers
    // inside inline asm, where hipcc's hazard recognizer pads only 1: without this nop the lo plane is read stale.
    asm volatile("s_nop 1" : "+v"(bh), "+v"(bl));
}

// C^T tiles of W^T X^T for NT output tiles of 16 channels and the wave's PW panels, K = 32 KS, f16x3 (hi.hi + (hi.lo + lo.hi) / 2048).
// out[pp][2 nt + e] = the pair (channels 16 nt + 4 g + 2 e, + 1) of token t of panel pp.
template <int PW, int NT, int KS>
__device__ __forceinline__ void mm(const WF<NT, KS>& w, const h16x8 (&bh)[PW][KS], const h16x8 (&bl)[PW][KS], f32x2 (&out)[PW][2 * NT]) {
    f32x4 acc0[PW][NT], acc1[PW][NT];
#pragma unroll
    for (int pp = 0; pp < PW; ++pp)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) { acc0[pp][nt] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc1[pp][nt] = acc0[pp][nt]; }
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int pp = 0; pp < PW; ++pp) {
                acc0[pp][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.h[nt][s], bh[pp][s], acc0[pp][nt], 0, 0, 0);
                acc1[pp][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.h[nt][s], bl[pp][s], acc1[pp][nt], 0, 0, 0);
                acc1[pp][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.l[nt][s], bh[pp][s], acc1[pp][nt], 0, 0, 0);
            }
    // 20 wait states between the LAST MFMA and the first inline-asm reader of any accumulator.  Every accumulator is tied to an
    // empty volatile statement IN FRONT of the nops (volatile statements keep their order): tying only one of them, as
    // pk::mfma_fence does, lets hipcc schedule the MFMAs of the other tiles behind the nops when their weight loads come late.
#pragma unroll
    for (int pp = 0; pp < PW; ++pp)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) pk::behind_fence(acc0[pp][nt], acc1[pp][nt]);
    asm volatile("s_nop 15\n\ts_nop 3" ::: "memory");
#pragma unroll
    for (int pp = 0; pp < PW; ++pp)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) pk::behind_fence(acc0[pp][nt], acc1[pp][nt]);
    const f32x2 inv = pk::splat(1.0f / H3_SCALE);
#pragma unroll
    for (int pp = 0; pp < PW; ++pp)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int e = 0; e < 2; ++e)
                out[pp][2 * nt + e] = pk::fma((f32x2){acc1[pp][nt][2 * e], acc1[pp][nt][2 * e + 1]}, inv,
                                              (f32x2){acc0[pp][nt][2 * e], acc0[pp][nt][2 * e + 1]});
}

// sum of p.x + p.y over the 4 lanes of a token (l, l ^ 16, l ^ 32, l ^ 48), the same order and value in all four:
// (g0 + g1) + (g2 + g3) through v_permlane16_swap (odd rows of the first operand <-> even rows of the second) and v_permlane32_swap
__device__ __forceinline__ float sum4(const f32x2 p) {
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    float v;
    asm("v_add_f32 %0, %1, %2\n\ts_nop 1" : "=v"(v) : "v"(p[0]), "v"(p[1]));      // + the wait states in front of the lane swap
    const u32x2 r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    const float h = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    const u32x2 s = __builtin_amdgcn_permlane32_swap(__float_as_uint(h), __float_as_uint(h), false, false);
    return __uint_as_float(s[0]) + __uint_as_float(s[1]);
}

// the lane's 4 pairs of a 32-wide parameter vector: channels 4 g .. + 3 and 16 + 4 g .. + 3
__device__ __forceinline__ void param_pairs(const float* b, const int g, f32x2* bp) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(b + 16 * u + 4 * g);
        bp[2 * u] = (f32x2){b4[0], b4[1]}; bp[2 * u + 1] = (f32x2){b4[2], b4[3]};
    }
}

// LayerNormalization over the 32 channels of a token, 8 of them in this lane (arithmetic of sh3::ln_tokens)
__device__ __forceinline__ void ln_token(const f32x2 (&x)[4], const f32x2 (&gp)[4], const f32x2 (&bp)[4], const float eps, f32x2 (&y)[4]) {
    const float mean = sum4(pk::add(pk::add(x[0], x[1]), pk::add(x[2], x[3]))) * (1.0f / 32.0f);
    const f32x2 m2 = pk::splat(mean);
    f32x2 q2;
    { const f32x2 d = pk::sub(x[0], m2); q2 = pk::mul(d, d); }
#pragma unroll
    for (int i = 1; i < 4; ++i) { const f32x2 d = pk::sub(x[i], m2); q2 = pk::fma(d, d, q2); }
    const float q = sum4(q2);
    const float rstd = 1.0f / sqrtf(q * (1.0f / 32.0f) + eps);
    const f32x2 r2 = pk::splat(rstd);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f32x2 inv = pk::mul(r2, gp[i]);
        y[i] = pk::fma(x[i], inv, pk::fnma(m2, inv, bp[i]));
    }
}
}  // namespace sp16

// out_lo == nullptr: out is the f32 (frames, J, 32) tensor; otherwise out_hi / out_lo are its two f16 planes.
// NW = ceil(J FR / 16 PW) waves per workgroup; dynamic LDS sp16::lds_bytes<FR>(depth).
template <int J, int FR, int PW>
__global__ void __launch_bounds__(64 * p16_waves(J, FR, PW)) UU3D_PK_TARGET
spatial_stack_p16_kernel(const float* __restrict__ kp2d, const SpatialParams p, const _Float16* __restrict__ wfrag,
                         float* __restrict__ out, _Float16* __restrict__ out_hi, _Float16* __restrict__ out_lo)
{
    // Every slot of every panel runs the same instructions; contraction is off and every FMA is written out, so a token's result
    // is the same bits wherever its frame sits.
#pragma clang fp contract(off)
    using namespace sp16;
    h3_flush_f16_denormals();
    constexpr int DS = 32, HS = 64, NP = (J + 1) / 2;
    constexpr int NW = p16_waves(J, FR, PW);
    static_assert(J == 17 && DS == 32 && HS == 64, "17 joints, d = 32, hidden 64");
    using LY = SpatialBlockLayoutV2<DS, HS>;
    using FL = SpatialFragLayoutP16;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    float* TK = reinterpret_cast<float*>(lds_raw);                      // K: [FR frames][9 key pairs][68] (+ pad) floats
    float* TV = TK + FR * KFLD;                                         // V likewise
    float* P = TV + FR * KFLD;                                          // [depth][352] LayerNorm parameters and biases

    const int lane = threadIdx.x & 63, t = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int nframes = p.total_frames;
    if (p.frame_list != nullptr) {
        nframes = p.frame_list[p.total_frames];
        if ((int)blockIdx.x * FR >= nframes) return;
    }
    // parameters of every block and the spare key slot of every frame (finite: its probability is forced to zero), once
    for (int k = threadIdx.x; k < p.depth * NPARAM; k += 64 * NW) P[k] = p.blocks[(size_t)(k / NPARAM) * LY::size + k % NPARAM];
    for (int k = threadIdx.x; k < FR * 2 * DS; k += 64 * NW) {
        const int f = k / (2 * DS), c = k % DS;
        (k % (2 * DS) < DS ? TK : TV)[f * KFLD + (NP - 1) * sh3::KPLD + 2 * c + 1] = 0.f;
    }
    __syncthreads();

    // slot -> token: slot s = 16 (PW wave + pp) + t is joint s % J of frame s / J of this workgroup
    int frame[PW], joint[PW], kslot[PW];
    unsigned kfr[PW];
    bool valid[PW], real[PW];
#pragma unroll
    for (int pp = 0; pp < PW; ++pp) {
        const int s = 16 * (PW * wave + pp) + t;
        real[pp] = s < J * FR;
        const int fl = real[pp] ? s / J : FR - 1;
        joint[pp] = real[pp] ? s % J : J - 1;
        int f = blockIdx.x * FR + fl;
        valid[pp] = real[pp] && (f < nframes);
        if (p.frame_list != nullptr) f = p.frame_list[min(f, nframes - 1)];
        frame[pp] = min(f, p.total_frames - 1);
        kslot[pp] = fl * KFLD + (joint[pp] >> 1) * sh3::KPLD + (joint[pp] & 1);
        kfr[pp] = (unsigned)(fl * KFLD * 4);
    }
    const unsigned tk_a = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const void*)TK;
    const unsigned tv_a = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const void*)TV;

    // keypoint embedding + spatial PE (u_u_t.py:321-323): pair i = channels 16 (i >> 1) + 4 g + 2 (i & 1), + 1
    f32x2 x[PW][4];
#pragma unroll
    for (int pp = 0; pp < PW; ++pp) {
        float kx = 0.f, ky = 0.f;
        if (valid[pp]) { const float2 k2 = *reinterpret_cast<const float2*>(kp2d + ((size_t)frame[pp] * J + joint[pp]) * 2); kx = k2.x; ky = k2.y; }
        const f32x2 kx2 = pk::splat(kx), ky2 = pk::splat(ky);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = 16 * (i >> 1) + 4 * g + 2 * (i & 1);
            const f32x2 w0 = *reinterpret_cast<const f32x2*>(p.embed_w + c), w1 = *reinterpret_cast<const f32x2*>(p.embed_w + DS + c);
            const f32x2 eb = *reinterpret_cast<const f32x2*>(p.embed_b + c), pe = *reinterpret_cast<const f32x2*>(p.pe + joint[pp] * DS + c);
            x[pp][i] = pk::add(pk::add(pk::fma(ky2, w1, pk::mul(kx2, w0)), eb), pe);
        }
    }
    auto wg_sync = [&]() __attribute__((always_inline)) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    // K / V of the lane's tokens into the key-pair image: channel c of joint j at [frame][j >> 1][c][j & 1]
    auto store_kv = [&](float* T, const f32x2 (&v)[PW][4]) __attribute__((always_inline)) {
#pragma unroll
        for (int pp = 0; pp < PW; ++pp) {
            if (!real[pp]) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = 16 * (i >> 1) + 4 * g + 2 * (i & 1);
                T[kslot[pp] + 2 * c] = v[pp][i][0]; T[kslot[pp] + 2 * c + 2] = v[pp][i][1];
            }
        }
    };

    for (int blk = 0; blk < p.depth; ++blk) {
        const _Float16* __restrict__ F = wfrag + (size_t)blk * FL::size;
        const float* W = P + blk * NPARAM;
        WF<2, 1> wq, wk, wv, wp;
        load_w(F + FL::fq, lane, wq); load_w(F + FL::fk, lane, wk); load_w(F + FL::fv, lane, wv);
        f32x2 gp[4], bp[4];

        // ---- attention half ----
        h16x8 bh[PW][1], bl[PW][1];
        param_pairs(W + LY::ln1_g, g, gp); param_pairs(W + LY::ln1_b, g, bp);
#pragma unroll
        for (int pp = 0; pp < PW; ++pp) {
            f32x2 y[4];
            ln_token(x[pp], gp, bp, 1e-5f, y);
            frag_of(y, bh[pp][0], bl[pp][0]);
        }
        f32x2 q[PW][4];
        {
            f32x2 kv[PW][4];
            mm<PW, 2, 1>(wq, bh, bl, q);
            param_pairs(W + LY::bq, g, bp);
#pragma unroll
            for (int pp = 0; pp < PW; ++pp)
#pragma unroll
                for (int i = 0; i < 4; ++i) q[pp][i] = pk::add(q[pp][i], bp[i]);
            mm<PW, 2, 1>(wk, bh, bl, kv);
            param_pairs(W + LY::bk, g, bp);
#pragma unroll
            for (int pp = 0; pp < PW; ++pp)
#pragma unroll
                for (int i = 0; i < 4; ++i) kv[pp][i] = pk::add(kv[pp][i], bp[i]);
            wg_sync();                                     // every wave is done reading the previous block's K / V
            store_kv(TK, kv);
            load_w(F + FL::fp, lane, wp);
            mm<PW, 2, 1>(wv, bh, bl, kv);
            param_pairs(W + LY::bv, g, bp);
#pragma unroll
            for (int pp = 0; pp < PW; ++pp)
#pragma unroll
                for (int i = 0; i < 4; ++i) kv[pp][i] = pk::add(kv[pp][i], bp[i]);
            store_kv(TV, kv);
        }
        wg_sync();                                         // K / V of every token of the frames are in LDS
        // softmax(q k^T / 2) v over the J joints of the token's frame: heads g (pairs 0, 1) and 4 + g (pairs 2, 3)
        f32x2 o[PW][4];
#pragma unroll
        for (int pp = 0; pp < PW; ++pp)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const unsigned off = kfr[pp] + (unsigned)((16 * u + 4 * g) * 2 * 4);
                f32x2 qa[1] = {q[pp][2 * u]}, qb[1] = {q[pp][2 * u + 1]}, oa[1], ob[1];
                sh3::head_attention<J, 1>(qa, qb, tk_a + off, tv_a + off, oa, ob);
                o[pp][2 * u] = oa[0]; o[pp][2 * u + 1] = ob[0];
            }
#pragma unroll
        for (int pp = 0; pp < PW; ++pp) frag_of(o[pp], bh[pp][0], bl[pp][0]);
        {
            f32x2 pr[PW][4];
            mm<PW, 2, 1>(wp, bh, bl, pr);
            param_pairs(W + LY::bp, g, bp);
#pragma unroll
            for (int pp = 0; pp < PW; ++pp)
#pragma unroll
                for (int i = 0; i < 4; ++i) x[pp][i] = pk::add(x[pp][i], pk::add(pr[pp][i], bp[i]));
        }

        // ---- MLP half ----
        WF<4, 1> w1;
        WF<2, 2> w2;
        load_w(F + FL::f1, lane, w1);
        load_w(F + FL::f2, lane, w2);
        param_pairs(W + LY::ln2_g, g, gp); param_pairs(W + LY::ln2_b, g, bp);
#pragma unroll
        for (int pp = 0; pp < PW; ++pp) {
            f32x2 y[4];
            ln_token(x[pp], gp, bp, 1e-5f, y);
            frag_of(y, bh[pp][0], bl[pp][0]);
        }
        h16x8 hh[PW][2], hl[PW][2];
        {
            f32x2 hd[PW][8], b1[8];
            mm<PW, 4, 1>(w1, bh, bl, hd);
            param_pairs(W + LY::b1, g, b1); param_pairs(W + LY::b1 + 32, g, b1 + 4);
#pragma unroll
            for (int pp = 0; pp < PW; ++pp) {
#pragma unroll
                for (int i = 0; i < 8; ++i) hd[pp][i] = sh3::gelu_pair(pk::add(hd[pp][i], b1[i]));
#pragma unroll
                for (int s = 0; s < 2; ++s) frag_of(hd[pp] + 4 * s, hh[pp][s], hl[pp][s]);
            }
        }
        {
            f32x2 z[PW][4];
            mm<PW, 2, 2>(w2, hh, hl, z);
            param_pairs(W + LY::b2, g, bp);
#pragma unroll
            for (int pp = 0; pp < PW; ++pp)
#pragma unroll
                for (int i = 0; i < 4; ++i) x[pp][i] = pk::add(x[pp][i], pk::add(z[pp][i], bp[i]));
        }
    }

    f32x2 gp[4], bp[4];
    param_pairs(p.norm_g, g, gp); param_pairs(p.norm_b, g, bp);
#pragma unroll
    for (int pp = 0; pp < PW; ++pp) {
        f32x2 y[4];
        ln_token(x[pp], gp, bp, 1e-6f, y);
        if (!valid[pp]) continue;
        const size_t at = ((size_t)frame[pp] * J + joint[pp]) * DS;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int c = 16 * u + 4 * g;
            if (out_lo != nullptr) {
                h16x4 hi, lo;
                sh3::split_pairs(y[2 * u], y[2 * u + 1], hi, lo);
                *reinterpret_cast<h16x4*>(out_hi + at + c) = hi;
                *reinterpret_cast<h16x4*>(out_lo + at + c) = lo;
            } else {
                *reinterpret_cast<f32x4*>(out + at + c) = (f32x4){y[2 * u][0], y[2 * u][1], y[2 * u + 1][0], y[2 * u + 1][1]};
            }
        }
    }
}

}  // namespace uu3d
