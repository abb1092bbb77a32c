// uu3d_spatial_generic.h -- the spatial stack of ONE frame in one workgroup, for handles with generic dims (inference only).
//
// uu3d_frame_features on a generic handle: keypoint embedding + spatial_pe, `depth` pre-LN blocks (LayerNorm eps 1e-5, q | k | v, attention
// over the J joints per head with logits / sqrt(d_h), projection + residual, LayerNorm, fc1, exact erf GELU, fc2 + residual), spatial_norm
// (eps 1e-6) -> S (F, J d_s).  J, d_s, h_s, the head count and the depth are run-time values.  Exact f32 (plain FMA), no MFMA, no atomics.
//
// Weights are read from the handle's master parameter buffer in its Keras (in, out) layout: neighbouring lanes take neighbouring output
// columns, so a wave reads whole rows of a kernel.  No operand pack is touched: a Trainer's repack cannot reach this stage.
//
// LDS (all dynamic, floats): X[J][d_s] the residual stream | Y[J][d_s] LayerNorm output, then the attention output | W[J][wmax + 1]
// q | k | v, then the hidden layer (wmax = max(3 d_s, h_s); the odd row pitch keeps the k rows of a wave's 64 joints on different banks) |
// P[hg][J][J | 1] the logits / weights of hg heads at a time.  Every element has ONE writer per phase; phases are separated by barriers.
// spatial_generic_lds_bytes is the rule of include/uu3d.h (FRAMES FORM): a frame that does not fit 160 KiB has no frames form.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

namespace uu3d {

// offsets (floats) of a spatial block's tensors in the master parameter buffer; -1: the tensor does not exist (QKV_BIAS = False)
struct SpatialGenericBlock { long long n1g, n1b, wq, bq, wk, bk, wv, bv, wp, bp, n2g, n2b, w1, b1, w2, b2; };

struct SpatialGenericParams {
    const float* params;                       // the master parameter buffer
    const SpatialGenericBlock* blocks;         // [depth], device memory
    long long emb_w, emb_b, pe, norm_g, norm_b;
    int J, ds, hs, H, depth, hg;               // hg: heads whose logits share the P buffer (spatial_generic_head_group)
};

constexpr int SG_THREADS = 256;
constexpr int SG_ROWS = 4;                     // rows of the frame a thread accumulates for its output column
constexpr size_t SG_LDS_LIMIT = (size_t)160 * 1024;

// heads per attention pass: as many as fit 2048 logits, at least one
__host__ __device__ inline int spatial_generic_head_group(int J, int H) {
    const int hg = 2048 / (J * (J | 1));
    return hg < 1 ? 1 : (hg > H ? H : hg);
}
__host__ __device__ inline int spatial_generic_wpitch(int ds, int hs) { return (3 * ds > hs ? 3 * ds : hs) + 1; }
// the frame's LDS in bytes: X + Y + W + P
__host__ __device__ inline size_t spatial_generic_lds_bytes(int J, int ds, int hs, int H) {
    return sizeof(float) * ((size_t)2 * J * ds + (size_t)J * spatial_generic_wpitch(ds, hs) + (size_t)spatial_generic_head_group(J, H) * J * (J | 1));
}

namespace sg {

__device__ __forceinline__ float gelu_erf(float h) { return 0.5f * h * (1.0f + erff(h * 0.70710678118654752440f)); }

// Y[r][c] = LayerNorm(X[r])[c] (Keras non-fused formula, two-pass statistics): one wave per row, rows pitch D in X, ldy in Y
__device__ __forceinline__ void layernorm(const float* X, const int J, const int D, const float* __restrict__ g, const float* __restrict__ b,
                                          const float eps, float* Y, const int ldy) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < J; r += SG_THREADS / 64) {
        const float* x = X + r * D;
        float s = 0.f;
        for (int c = lane; c < D; c += 64) s += x[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        const float mean = s / (float)D;
        float q = 0.f;
        for (int c = lane; c < D; c += 64) { const float d = x[c] - mean; q = fmaf(d, d, q); }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
        const float rstd = 1.0f / sqrtf(q / (float)D + eps);
        for (int c = lane; c < D; c += 64) {
            const float inv = rstd * g[c];
            Y[(size_t)r * ldy + c] = x[c] * inv + (b[c] - mean * inv);
        }
    }
}

// out[r][c] = f(sum_k A[r][k] Wg[k][c] + bias[c]) for r < J, c < N.  Wg: a Keras (K, N) kernel in global memory; bias may be NULL.
// MODE 0: store; 1: store GELU; 2: out[r][c] += (the residual: each element read and written by its one thread)
template <int MODE, int ROWS>
__device__ __forceinline__ void dense(const float* A, const int lda, const float* __restrict__ Wg, const float* __restrict__ bias,
                                      const int J, const int K, const int N, float* out, const int ldo) {
    const int groups = (J + ROWS - 1) / ROWS;
    for (int item = threadIdx.x; item < groups * N; item += SG_THREADS) {
        const int g = item / N, c = item - g * N, r0 = g * ROWS;
        int ro[ROWS];
#pragma unroll
        for (int i = 0; i < ROWS; ++i) ro[i] = (r0 + i < J ? r0 + i : J - 1) * lda;      // (rows past the frame: read the last row, store nothing)
        float acc[ROWS];
#pragma unroll
        for (int i = 0; i < ROWS; ++i) acc[i] = 0.f;
        for (int k = 0; k < K; ++k) {
            const float w = Wg[(size_t)k * N + c];
#pragma unroll
            for (int i = 0; i < ROWS; ++i) acc[i] = fmaf(A[ro[i] + k], w, acc[i]);
        }
        const float bc = bias != nullptr ? bias[c] : 0.f;
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            if (r0 + i >= J) break;
            const float v = acc[i] + bc;
            float* o = out + (r0 + i) * ldo + c;
            if (MODE == 0) *o = v;
            else if (MODE == 1) *o = gelu_erf(v);
            else *o = *o + v;
        }
    }
}

}  // namespace sg

// grid: one workgroup per frame; dynamic LDS: spatial_generic_lds_bytes(J, ds, hs, H).  ROWS: SG_ROWS, the one instantiation -- a template
// like every kernel of the library's headers, so that a host-only compile of this header (the LDS rule, tests/test_generic_frames_cpu.py)
// emits no kernel stub that would want device code linked in
template <int ROWS>
__global__ void __launch_bounds__(SG_THREADS)
spatial_generic_kernel(const float* __restrict__ frames, const SpatialGenericParams p, float* __restrict__ S)
{
    extern __shared__ float sg_lds[];
    const int J = p.J, ds = p.ds, hs = p.hs, H = p.H, dh = ds / H, Jp = J | 1;
    const int ldw = spatial_generic_wpitch(ds, hs);
    float* const X = sg_lds;
    float* const Y = X + J * ds;
    float* const W = Y + J * ds;
    float* const P = W + J * ldw;
    const float* const prm = p.params;
    auto at = [&](long long off) -> const float* { return off < 0 ? nullptr : prm + off; };
    const size_t f = blockIdx.x;
    const int tid = threadIdx.x;

    // keypoint embedding + spatial_pe (u_u_t.py:321-323)
    {
        const float* kp = frames + f * (size_t)J * 2;
        const float* We = at(p.emb_w); const float* be = at(p.emb_b); const float* pe = at(p.pe);
        for (int idx = tid; idx < J * ds; idx += SG_THREADS) {
            const int r = idx / ds, c = idx - r * ds;
            const float kx = kp[2 * r], ky = kp[2 * r + 1];
            X[idx] = (fmaf(ky, We[ds + c], kx * We[c]) + be[c]) + pe[idx];
        }
    }
    __syncthreads();

    const float sqrt_dh = sqrtf((float)dh);
    for (int blk = 0; blk < p.depth; ++blk) {
        const SpatialGenericBlock b = p.blocks[blk];
        sg::layernorm(X, J, ds, at(b.n1g), at(b.n1b), 1e-5f, Y, ds);
        __syncthreads();
        sg::dense<0, ROWS>(Y, ds, at(b.wq), at(b.bq), J, ds, ds, W, ldw);
        sg::dense<0, ROWS>(Y, ds, at(b.wk), at(b.bk), J, ds, ds, W + ds, ldw);
        sg::dense<0, ROWS>(Y, ds, at(b.wv), at(b.bv), J, ds, ds, W + 2 * ds, ldw);
        __syncthreads();
        // attention over the J joints, p.hg heads at a time: logits -> softmax -> weights x v into Y (LayerNorm 1's output is spent)
        for (int h0 = 0; h0 < H; h0 += p.hg) {
            const int nh = H - h0 < p.hg ? H - h0 : p.hg;
            for (int idx = tid; idx < nh * J * J; idx += SG_THREADS) {
                const int h = idx / (J * J), rem = idx - h * J * J, i = rem / J, j = rem - i * J;
                const float* q = W + i * ldw + (h0 + h) * dh;
                const float* k = W + j * ldw + ds + (h0 + h) * dh;
                float s = 0.f;
                for (int d = 0; d < dh; ++d) s = fmaf(q[d], k[d], s);
                P[(h * J + i) * Jp + j] = s / sqrt_dh;
            }
            __syncthreads();
            for (int row = tid; row < nh * J; row += SG_THREADS) {
                float* pr = P + row * Jp;
                float mx = pr[0];
                for (int j = 1; j < J; ++j) mx = fmaxf(mx, pr[j]);
                float sum = 0.f;
                for (int j = 0; j < J; ++j) { const float e = expf(pr[j] - mx); pr[j] = e; sum += e; }
                for (int j = 0; j < J; ++j) pr[j] = pr[j] / sum;
            }
            __syncthreads();
            for (int idx = tid; idx < nh * J * dh; idx += SG_THREADS) {
                const int h = idx / (J * dh), rem = idx - h * J * dh, i = rem / dh, d = rem - i * dh;
                const float* pr = P + (h * J + i) * Jp;
                const float* v = W + 2 * ds + (h0 + h) * dh + d;
                float o = 0.f;
                for (int j = 0; j < J; ++j) o = fmaf(pr[j], v[j * ldw], o);
                Y[i * ds + (h0 + h) * dh + d] = o;
            }
            __syncthreads();
        }
        sg::dense<2, ROWS>(Y, ds, at(b.wp), at(b.bp), J, ds, ds, X, ds);
        __syncthreads();
        sg::layernorm(X, J, ds, at(b.n2g), at(b.n2b), 1e-5f, Y, ds);
        __syncthreads();
        sg::dense<1, ROWS>(Y, ds, at(b.w1), at(b.b1), J, ds, hs, W, ldw);
        __syncthreads();
        sg::dense<2, ROWS>(W, ldw, at(b.w2), at(b.b2), J, hs, ds, X, ds);
        __syncthreads();
    }
    // spatial_norm (u_u_t.py:329) straight into S (F, J d_s)
    sg::layernorm(X, J, ds, at(p.norm_g), at(p.norm_b), 1e-6f, S + f * (size_t)J * ds, ds);
}

}  // namespace uu3d
