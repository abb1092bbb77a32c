// uu3d_ops.hip -- C ABI of the backward building blocks, of the forward operators and of the training step's GEMM forms (include/uu3d_ops.h).
#include <hip/hip_runtime.h>
#include <algorithm>
#include "../../include/uu3d.h"
#include "../../include/uu3d_ops.h"
#include "uu3d_gemm.h"
#include "uu3d_misc.h"
#include "uu3d_bwd.h"
#include "uu3d_launch.h"
#include "uu3d_pack.h"
#include "uu3d_tchain16.h"      // tchain_qf_index, tchain_qf_halfs
#include "uu3d_train_kernels.h" // the training step's loaders, epilogues and small kernels
#include <vector>
#include <initializer_list>

using namespace uu3d;

size_t uu3d_op_scratch_floats(void) { return kOpScratchFloats; }

int uu3d_op_gemm_tn(const float* a, int32_t lda, const float* b, int32_t ldb, int32_t R, int32_t P, int32_t Q, float* c,
                    int32_t ldc, float* scratch, size_t scratch_floats, void* stream) {
    if (!a || !b || !c || !scratch || R < 1 || P < 1 || Q < 1 || (lda & 3) || (ldb & 3) || (P & 3) || (Q & 3) || lda < P || ldb < Q || ldc < Q) return UU3D_ERR_INVALID_ARGUMENT;
    TnLoadPlain al{a, lda, R, P};
    EpStore ep{c, ldc};
    return launch_gemm_tn(al, b, ldb, R, P, Q, ep, scratch, scratch_floats, (hipStream_t)stream);
}
int uu3d_op_gemm_tn_h3(const float* a, int32_t lda, const float* b, int32_t ldb, int32_t R, int32_t P, int32_t Q, float* c,
                       int32_t ldc, float* scratch, size_t scratch_floats, void* stream) {
    if (!a || !b || !c || !scratch || R < 1 || P < 1 || Q < 1 || (lda & 3) || (ldb & 3) || (P & 3) || (Q & 3) || lda < P || ldb < Q || ldc < Q) return UU3D_ERR_INVALID_ARGUMENT;
    TnLoadPlain al{a, lda, R, P};
    EpStore ep{c, ldc};
    return launch_gemm_tn(al, b, ldb, R, P, Q, ep, scratch, scratch_floats, (hipStream_t)stream, true);
}

int uu3d_op_gemm_nt(const float* a, int32_t lda, const float* w, int32_t ldw, int32_t M, int32_t N, int32_t K, float* c,
                    int32_t ldc, float* scratch, size_t scratch_floats, void* stream) {
    if (!a || !w || !c || M < 1 || N < 64 || K < 32 || (N & 63) || (K & 31) || ldw != K || lda < K || (lda & 3) || ldc < N) return UU3D_ERR_INVALID_ARGUMENT;
    ALoadPlain al{a, lda, M, K};
    EpStore ep{c, ldc};
    return launch_gemm(al, w, M, N, K, ep, scratch, scratch_floats, (hipStream_t)stream);
}

int uu3d_op_colsum(const float* x, int32_t ldx, int32_t R, int32_t C, int32_t period, const uint8_t* mask, int32_t want,
                   float* out, int32_t accumulate, float* scratch, size_t scratch_floats, void* stream) {
    if (!x || !out || !scratch || R < 1 || C < 1 || period < 0 || ldx < C) return UU3D_ERR_INVALID_ARGUMENT;
    return launch_colsum(x, ldx, R, C, period, mask, want, out, accumulate, scratch, scratch_floats, (hipStream_t)stream);
}

int uu3d_op_row_stats(const float* x, int32_t ld, int32_t D, int32_t M, float eps, float* stats, void* stream) {
    if (!x || !stats || D < 4 || (D & 3) || D > 1024 || M < 1 || ld < D || (ld & 3)) return UU3D_ERR_INVALID_ARGUMENT;
    launch_row_stats(x, ld, D, M, eps, (float2*)stats, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_op_ln_bwd(const float* x, const float* dy, const float* stats, const float* gamma, int32_t ld, int32_t D, int32_t M,
                   float* dx, int32_t accumulate, float* dgamma, float* dbeta, float* scratch, size_t scratch_floats, void* stream) {
    if (!x || !dy || !stats || !gamma || !dx || !dgamma || !dbeta || !scratch || D < 4 || (D & 3) || D > 1024 || M < 1 || ld < D || (ld & 3)) return UU3D_ERR_INVALID_ARGUMENT;
    return launch_ln_bwd(x, dy, (const float2*)stats, gamma, ld, D, M, dx, accumulate, dgamma, dbeta, 0, scratch, scratch_floats, (hipStream_t)stream);
}

// the head dim 4 and MFMA kernels move a head's row as 16-byte pieces: row strides multiples of 4 floats, wide enough for [q | k | v] / the heads
static bool attn_args_ok(int32_t ld, int32_t D, int32_t B, int32_t L, int32_t H, int32_t dh, int32_t ldo) {
    return B >= 1 && L >= 1 && H >= 1 && (dh == 4 || dh == 48) && (int64_t)D == (int64_t)H * dh && (int64_t)ld >= (int64_t)3 * D && ldo >= D && !(ld & 3) && !(ldo & 3);
}
int uu3d_op_attn_fwd(const float* qkv, int32_t ld, int32_t D, int32_t B, int32_t L, int32_t H, int32_t dh, const uint8_t* mask,
                     float* out, int32_t ldo, void* stream) {
    if (!qkv || !out || !attn_args_ok(ld, D, B, L, H, dh, ldo)) return UU3D_ERR_INVALID_ARGUMENT;
    if (L > 128) return UU3D_ERR_UNSUPPORTED;
    return launch_attn_generic(false, qkv, nullptr, ld, D, B, L, H, dh, mask, out, ldo, (hipStream_t)stream);
}
int uu3d_op_attn_bwd(const float* qkv, const float* dout, int32_t ld, int32_t D, int32_t B, int32_t L, int32_t H, int32_t dh,
                     const uint8_t* mask, float* dqkv, int32_t ldo, void* stream) {
    if (!qkv || !dout || !dqkv || !attn_args_ok(ld, D, B, L, H, dh, ldo)) return UU3D_ERR_INVALID_ARGUMENT;
    if (L > 96) return UU3D_ERR_UNSUPPORTED;      // P and dS matrices of one head must fit the 160 KiB LDS
    return launch_attn_generic(true, qkv, dout, ld, D, B, L, H, dh, mask, dqkv, ldo, (hipStream_t)stream, DropCfg{}, read_switches().train.attn_bwd_generic);
}

// the kernels move rows as 16-byte pieces (q / k / v, O, dO; statistics as 8-byte pairs): leading dimensions multiples of 4 floats,
// base pointers 16-byte aligned
static bool attn_long_aligned(int32_t ld, int32_t ldo, std::initializer_list<const void*> ptrs) {
    if (ld < 1 || ldo < 1 || (ld & 3) || (ldo & 3)) return false;
    for (const void* p : ptrs) if ((uintptr_t)p & 15) return false;
    return true;
}
int uu3d_op_attn_long_fwd(const float* qkv, int32_t ld, int32_t D, int32_t B, int32_t L, int32_t H, const uint8_t* mask, float* out,
                          int32_t ldo, float* stats, void* stream) {
    if (!qkv || !out || !stats || B < 1 || H < 1 || !attn_long_aligned(ld, ldo, {qkv, out, stats})) return UU3D_ERR_INVALID_ARGUMENT;
    if (D != 48 * H || L < 1 || L > ATTN_LONG_MAX_L) return UU3D_ERR_UNSUPPORTED;
    return launch_attn_long(false, qkv, nullptr, nullptr, nullptr, ld, D, B, L, H, mask, out, (float2*)stats, ldo, (hipStream_t)stream);
}
// the inference instantiation (no statistics), launched through launch_attn_long_infer as the exact-f32 forward above 128 tokens launches it
int uu3d_op_attn_long_infer(const float* qkv, int32_t ld, int32_t D, int32_t B, int32_t L, int32_t H, const uint8_t* mask, float* out,
                            int32_t ldo, void* stream) {
    if (!qkv || !out || B < 1 || H < 1 || !attn_long_aligned(ld, ldo, {qkv, out})) return UU3D_ERR_INVALID_ARGUMENT;
    if (D != 48 * H || L < 1 || L > ATTN_LONG_MAX_L) return UU3D_ERR_UNSUPPORTED;
    const int st = launch_attn_long_infer(qkv, ld, D, B, L, H, mask, out, ldo, (hipStream_t)stream);
    return st != UU3D_OK ? st : hip_status();
}
int uu3d_op_attn_long_bwd(const float* qkv, const float* out, const float* dout, const float* stats, int32_t ld, int32_t D, int32_t B, int32_t L,
                          int32_t H, const uint8_t* mask, float* dqkv, int32_t ldo, void* stream) {
    if (!qkv || !out || !dout || !stats || !dqkv || B < 1 || H < 1 || !attn_long_aligned(ld, ldo, {qkv, out, dout, stats, dqkv})) return UU3D_ERR_INVALID_ARGUMENT;
    if (D != 48 * H || L < 1 || L > ATTN_LONG_MAX_L) return UU3D_ERR_UNSUPPORTED;
    return launch_attn_long(true, qkv, out, dout, (const float2*)stats, ld, D, B, L, H, mask, dqkv, nullptr, ldo, (hipStream_t)stream);
}

// ---- forward operators: the LayerNorm-fed Dense layers of the forward, each kernel on its own (launched through uu3d_launch.h, as the forward does) ----
// Keras (in, out) kernel w[K][N] on the host -> the transposed f16 planes Bt[n][k] the model keeps for every Dense kernel (uu3d_commit_weights: hi, lo * 2048)
static void split_transposed(const float* w, int K, int N, _Float16* bh, _Float16* bl) {
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < K; ++k) {
            const float x = w[(size_t)k * N + n];
            const _Float16 h = h3_hi(x);
            bh[(size_t)n * K + k] = h; bl[(size_t)n * K + k] = (_Float16)((x - (float)h) * H3_SCALE);
        }
}
static int upload_halfs(const std::vector<_Float16>& v, void* dst, hipStream_t stream) {
    if (hipMemcpyAsync(dst, v.data(), v.size() * sizeof(_Float16), hipMemcpyHostToDevice, stream) != hipSuccess) return UU3D_ERR_HIP;
    return hipStreamSynchronize(stream) == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

size_t uu3d_op_panel_operand_bytes(int32_t N) { return (N < 32 || (N & 31)) ? 0 : panel_b_halfs(N, 384) * sizeof(_Float16); }
size_t uu3d_op_panel_a_bytes(int32_t M) { return M < 1 ? 0 : panel_a_halfs(M, 384) * sizeof(_Float16); }

int uu3d_op_panel_pack(const float* w, int32_t N, void* operand_dev, void* stream) {
    if (!w || !operand_dev || N < 32 || (N & 31)) return UU3D_ERR_INVALID_ARGUMENT;
    const int K = 384;
    std::vector<_Float16> bh((size_t)N * K), bl((size_t)N * K), out(panel_b_halfs(N, K));
    split_transposed(w, K, N, bh.data(), bl.data());
    panel_pack_operand(bh.data(), bl.data(), N, K, K, out.data());
    return upload_halfs(out, operand_dev, (hipStream_t)stream);
}

int uu3d_op_panel_a_unpack(const void* frag_host, int32_t M, float* hi_host, float* lo_host) {
    if (!frag_host || !hi_host || !lo_host || M < 1) return UU3D_ERR_INVALID_ARGUMENT;
    const _Float16* f = reinterpret_cast<const _Float16*>(frag_host);
    for (int row = 0; row < M; ++row)
        for (int k = 0; k < 384; ++k) {
            const size_t at = panel_a_index(row, k, 384);
            hi_host[(size_t)row * 384 + k] = (float)f[at]; lo_host[(size_t)row * 384 + k] = (float)f[at + 512];
        }
    return UU3D_OK;
}

int uu3d_op_ln_dense_panel_ex(const float* x, int32_t ldx, int32_t M, const float* gamma, const float* beta, float eps, const void* operand,
                              const float* bias, int32_t N, int32_t waves, int32_t splits, int32_t epilogue, float qscale, void* a_scratch,
                              void* out, int32_t ldo, float* residual, const float* ln2_gamma, const float* ln2_beta, void* ln_out, void* stream_) {
    if (!x || !gamma || !beta || !operand || !bias || !a_scratch || M < 1 || N < 32 || (N & 31) || ldx < 384 || (ldx & 3)) return UU3D_ERR_INVALID_ARGUMENT;
    if ((waves != 4 && waves != 8) || splits < 0 || epilogue < UU3D_EP_BIAS || epilogue > UU3D_EP_BIAS_RESIDUAL_LN) return UU3D_ERR_INVALID_ARGUMENT;
    const bool res = epilogue == UU3D_EP_BIAS_RESIDUAL || epilogue == UU3D_EP_BIAS_RESIDUAL_LN;
    if (res ? (!residual || N != 384) : (!out || (epilogue == UU3D_EP_BIAS && ldo < N))) return UU3D_ERR_INVALID_ARGUMENT;
    if (epilogue == UU3D_EP_BIAS_SPLIT_Q && N % 3 != 0) return UU3D_ERR_INVALID_ARGUMENT;
    const int mt = (M + 127) / 128, chunks = N / 32;
    int S = splits;
    if (S == 0) {                                                     // any divisor that keeps <= 32 chunks per workgroup; prefer ~one round
        if (waves != 4) return UU3D_ERR_INVALID_ARGUMENT;
        for (int s = 1; s <= chunks; ++s) if (chunks % s == 0 && chunks / s <= PANEL_COLV_FLOATS / 32 && (S == 0 || (mt * s + 7) / 8 <= 32)) S = s;
    }
    if (S < 1 || chunks % S != 0 || chunks / S > PANEL_COLV_FLOATS / 32) return UU3D_ERR_INVALID_ARGUMENT;
    const int cpw = chunks / S;
    if (waves == 8 && !panel8_has(cpw)) return UU3D_ERR_INVALID_ARGUMENT;
    if (epilogue == UU3D_EP_BIAS_RESIDUAL_LN && (waves != 8 || S != 1 || !ln2_gamma || !ln2_beta || !ln_out)) return UU3D_ERR_INVALID_ARGUMENT;
    if ((double)M * (epilogue == UU3D_EP_BIAS ? ldo : N) * 4.0 >= 4.0e9) return UU3D_ERR_UNSUPPORTED;          // 32-bit byte offsets in the epilogue stores
    hipStream_t stream = (hipStream_t)stream_;
    _Float16* Af = reinterpret_cast<_Float16*>(a_scratch);
    const _Float16* Bf = reinterpret_cast<const _Float16*>(operand);
    hipLaunchKernelGGL((ln_split_frag_kernel<24, 8>), dim3((M + 7) / 8), dim3(128), 0, stream, x, ldx, M, eps, gamma, beta, Af);
    auto go = [&](const auto& ep) {
        if (waves == 8) (void)launch_panel8(stream, Af, Bf, bias, M, mt, S, cpw, ep);      // (panel8_has(cpw) held above)
        else launch_panel4(stream, Af, Bf, bias, M, mt, S, cpw, ep);
    };
    _Float16* oh = reinterpret_cast<_Float16*>(out);
    switch (epilogue) {
        case UU3D_EP_BIAS: go(PanelEpBias{reinterpret_cast<float*>(out), ldo}); break;
        case UU3D_EP_BIAS_RELU_SPLIT: go(PanelEpBiasReluSplit{oh, oh + (size_t)M * N, N}); break;
        case UU3D_EP_BIAS_SPLIT_Q: go(PanelEpBiasSplitQ{oh, oh + (size_t)M * N, N, N / 3, qscale}); break;
        case UU3D_EP_BIAS_RESIDUAL: {
            const PanelEpBiasResidual ep{residual, N};
            if (waves == 8) (void)launch_panel8(stream, Af, Bf, bias, M, mt, S, cpw, ep);
            else launch_panel4_residual(stream, Af, Bf, bias, M, mt, S, ep);
        } break;
        default: {
            const PanelEpBiasResidualLn ep{{residual, N}, ln2_gamma, ln2_beta, eps, reinterpret_cast<_Float16*>(ln_out)};
            (void)launch_panel8(stream, Af, Bf, bias, M, mt, 1, 12, ep);
        } break;
    }
    return hip_status();
}

int uu3d_op_ln_dense_panel(const float* x, int32_t ldx, int32_t M, const float* gamma, const float* beta, float eps, const void* operand,
                           const float* bias, int32_t N, int32_t relu, void* a_scratch, void* out, int32_t ldo, void* stream) {
    return uu3d_op_ln_dense_panel_ex(x, ldx, M, gamma, beta, eps, operand, bias, N, 4, 0, relu ? UU3D_EP_BIAS_RELU_SPLIT : UU3D_EP_BIAS, 1.0f,
                                     a_scratch, out, relu ? N : ldo, nullptr, nullptr, nullptr, nullptr, stream);
}

// ---- fused MLP of a temporal block (uu3d_mlp_fused.h) ----
size_t uu3d_op_mlp_operand_bytes(void) { return (panel_b_halfs(256 * MLPF_SLICES, 384) + mlpf_w2_halfs()) * sizeof(_Float16); }

int uu3d_op_mlp_pack(const float* w1, const float* w2, void* operand_dev, void* stream) {
    if (!w1 || !w2 || !operand_dev) return UU3D_ERR_INVALID_ARGUMENT;
    const int D = 32 * MLPF_OC, H = 256 * MLPF_SLICES;
    std::vector<_Float16> bh((size_t)D * H), bl((size_t)D * H), out(panel_b_halfs(H, D) + mlpf_w2_halfs());
    split_transposed(w1, D, H, bh.data(), bl.data());                // fc1: Bt[hidden][384] -> w1_pf
    panel_pack_operand(bh.data(), bl.data(), H, D, D, out.data());
    split_transposed(w2, H, D, bh.data(), bl.data());                // fc2: Bt[out][768] -> w2_mf
    mlpf_pack_w2(bh.data(), bl.data(), H, out.data() + panel_b_halfs(H, D));
    return upload_halfs(out, operand_dev, (hipStream_t)stream);
}

int uu3d_op_mlp_fused(const float* x, int32_t ldx, int32_t M, const float* gamma, const float* beta, float eps, const void* operand,
                      const float* b1, void* a_scratch, float* mslab, void* stream_) {
    if (!x || !gamma || !beta || !operand || !b1 || !a_scratch || !mslab || M < 1 || ldx < 384 || (ldx & 3)) return UU3D_ERR_INVALID_ARGUMENT;
    hipStream_t stream = (hipStream_t)stream_;
    _Float16* Af = reinterpret_cast<_Float16*>(a_scratch);
    const _Float16* W1f = reinterpret_cast<const _Float16*>(operand);
    hipLaunchKernelGGL((ln_split_frag_kernel<24, 8>), dim3((M + 7) / 8), dim3(128), 0, stream, x, ldx, M, eps, gamma, beta, Af);
    launch_mlp_fused(stream, Af, W1f, W1f + panel_b_halfs(256 * MLPF_SLICES, 384), b1, mslab, M);
    return hip_status();
}

// ---- few-row GEMM with LayerNorm in its loader (uu3d_gemm_wt.h) ----
static bool wt_dims_ok(int32_t N, int32_t K) { return N >= 32 && !(N & 31) && (K == 384 || K == 768); }
size_t uu3d_op_wt_operand_bytes(int32_t N, int32_t K) { return wt_dims_ok(N, K) ? (size_t)2 * N * K * sizeof(_Float16) : 0; }

int uu3d_op_wt_pack(const float* w, int32_t K, int32_t N, void* operand_dev, void* stream) {
    if (!w || !operand_dev || !wt_dims_ok(N, K)) return UU3D_ERR_INVALID_ARGUMENT;
    std::vector<_Float16> planes((size_t)2 * N * K);
    split_transposed(w, K, N, planes.data(), planes.data() + (size_t)N * K);
    return upload_halfs(planes, operand_dev, (hipStream_t)stream);
}

int uu3d_op_ln_dense_wt(const float* x, int32_t ldx, int32_t M, int32_t K, const float* gamma, const float* beta, float eps, const void* operand,
                        const float* bias, int32_t N, int32_t epilogue, float qscale, void* out, int32_t ldo, void* stream_) {
    if (!x || !gamma || !beta || !operand || !bias || !out || M < 1 || M > 512 || !wt_dims_ok(N, K) || ldx < K || (ldx & 3)) return UU3D_ERR_INVALID_ARGUMENT;
    if (epilogue < UU3D_EP_BIAS || epilogue > UU3D_EP_BIAS_SPLIT_Q || (epilogue == UU3D_EP_BIAS && ldo < N) || (epilogue == UU3D_EP_BIAS_SPLIT_Q && N % 3 != 0)) return UU3D_ERR_INVALID_ARGUMENT;
    hipStream_t stream = (hipStream_t)stream_;
    const _Float16* Bh = reinterpret_cast<const _Float16*>(operand); const _Float16* Bl = Bh + (size_t)N * K;
    const WtLoadF32 al{x, ldx, M, K, gamma, beta, eps, 1};
    _Float16* oh = reinterpret_cast<_Float16*>(out);
    bool ok;
    if (epilogue == UU3D_EP_BIAS) ok = launch_gemm_wt(stream, al, Bh, Bl, M, N, K, EpBias{reinterpret_cast<float*>(out), bias, ldo});
    else if (epilogue == UU3D_EP_BIAS_RELU_SPLIT) ok = launch_gemm_wt(stream, al, Bh, Bl, M, N, K, EpBiasReluSplit{oh, oh + (size_t)M * N, bias, N});
    else ok = launch_gemm_wt(stream, al, Bh, Bl, M, N, K, EpBiasSplitQ{oh, oh + (size_t)M * N, bias, N, N / 3, qscale});
    return ok ? hip_status() : UU3D_ERR_UNSUPPORTED;
}

// ---- the forward's temporal attention kernels (launch_attn_infer, uu3d_launch.h: the launch Launcher::attn makes) ----
size_t uu3d_op_attn_qf_bytes(int32_t rows) { return rows < 1 ? 0 : tchain_qf_halfs((rows + 127) / 128) * sizeof(_Float16); }

int uu3d_op_attn_qf_pack(const void* hi_host, const void* lo_host, int32_t rows, void* frag_host) {
    if (!hi_host || !lo_host || !frag_host || rows < 1) return UU3D_ERR_INVALID_ARGUMENT;
    const _Float16* hi = reinterpret_cast<const _Float16*>(hi_host); const _Float16* lo = reinterpret_cast<const _Float16*>(lo_host);
    _Float16* f = reinterpret_cast<_Float16*>(frag_host);
    for (int r = 0; r < rows; ++r)
        for (int k = 0; k < 1152; ++k) {
            f[tchain_qf_index((size_t)r, k, 0)] = hi[(size_t)r * 1152 + k];
            f[tchain_qf_index((size_t)r, k, 1)] = lo[(size_t)r * 1152 + k];
        }
    return UU3D_OK;
}

int uu3d_op_attn_qf_unpack(const void* frag_host, int32_t rows, void* hi_host, void* lo_host) {
    if (!hi_host || !lo_host || !frag_host || rows < 1) return UU3D_ERR_INVALID_ARGUMENT;
    const _Float16* f = reinterpret_cast<const _Float16*>(frag_host);
    _Float16* hi = reinterpret_cast<_Float16*>(hi_host); _Float16* lo = reinterpret_cast<_Float16*>(lo_host);
    for (int r = 0; r < rows; ++r)
        for (int k = 0; k < 1152; ++k) {
            hi[(size_t)r * 1152 + k] = f[tchain_qf_index((size_t)r, k, 0)];
            lo[(size_t)r * 1152 + k] = f[tchain_qf_index((size_t)r, k, 1)];
        }
    return UU3D_OK;
}

// ---- the temporal chain's layouts (uu3d_tchain16.h) on the HOST, through the kernel's own index functions ----
int uu3d_op_tchain_xs_pack(const float* x_host, int32_t M, int32_t slot, int32_t rows, void* scratch_host) {
    if (!x_host || !scratch_host || M < 1 || slot < 0 || slot > 1 || rows < 1 || rows > (M + 63) / 64 * 64) return UU3D_ERR_INVALID_ARGUMENT;
    float* s = reinterpret_cast<float*>(scratch_host) + (size_t)slot * ((M + 63) / 64) * T16_X_FLOATS_PER_TILE;
    for (int row = 0; row < rows; ++row)
        for (int ch = 0; ch < 384; ++ch) s[tchain16_xs_index(row, ch)] = x_host[(size_t)row * 384 + ch];
    return UU3D_OK;
}
int uu3d_op_tchain_xs_unpack(const void* scratch_host, int32_t M, int32_t slot, int32_t rows, float* x_host) {
    if (!x_host || !scratch_host || M < 1 || slot < 0 || slot > 1 || rows < 1 || rows > (M + 63) / 64 * 64) return UU3D_ERR_INVALID_ARGUMENT;
    const float* s = reinterpret_cast<const float*>(scratch_host) + (size_t)slot * ((M + 63) / 64) * T16_X_FLOATS_PER_TILE;
    for (int row = 0; row < rows; ++row)
        for (int ch = 0; ch < 384; ++ch) x_host[(size_t)row * 384 + ch] = s[tchain16_xs_index(row, ch)];
    return UU3D_OK;
}
int uu3d_op_panel_a_pack(const float* hi_host, const float* lo_host, int32_t M, void* frag_host) {
    if (!frag_host || !hi_host || !lo_host || M < 1) return UU3D_ERR_INVALID_ARGUMENT;
    const float* hi = hi_host; const float* lo = lo_host;
    _Float16* f = reinterpret_cast<_Float16*>(frag_host);
    for (int row = 0; row < M; ++row)
        for (int k = 0; k < 384; ++k) {
            const size_t at = panel_a_index(row, k, 384);
            f[at] = (_Float16)hi[(size_t)row * 384 + k]; f[at + 512] = (_Float16)lo[(size_t)row * 384 + k];
        }
    return UU3D_OK;
}

int uu3d_op_attn_infer(const void* qkv, int32_t in_layout, int32_t D, int32_t B, int32_t L, int32_t H, const uint8_t* mask, int32_t kernel,
                       void* out, int32_t out_layout, void* stream) {
    static_assert(UU3D_ATTN_AUTO == ATTN_AUTO && UU3D_ATTN_F32_WG == ATTN_F32_WG && UU3D_ATTN_HEAD_WAVE == ATTN_HEAD_WAVE && UU3D_ATTN_H3 == ATTN_H3, "uu3d_ops.h and uu3d_launch.h name the kernels alike");
    if (!qkv || !out || ((uintptr_t)qkv & 15) || ((uintptr_t)out & 15) || B < 1 || L < 1 || H < 1 || (int64_t)D != (int64_t)kAttnDH * H) return UU3D_ERR_INVALID_ARGUMENT;
    if (kernel < UU3D_ATTN_AUTO || kernel > UU3D_ATTN_H3 || in_layout < UU3D_ATTN_IN_F32 || in_layout > UU3D_ATTN_IN_QFRAG ||
        out_layout < UU3D_ATTN_OUT_F32 || out_layout > UU3D_ATTN_OUT_FRAG) return UU3D_ERR_INVALID_ARGUMENT;
    const bool planes_in = in_layout != UU3D_ATTN_IN_F32, planes_out = out_layout != UU3D_ATTN_OUT_F32;
    const bool qfrag = in_layout == UU3D_ATTN_IN_QFRAG, frag = out_layout == UU3D_ATTN_OUT_FRAG;
    if ((qfrag || frag) && D != 384) return UU3D_ERR_INVALID_ARGUMENT;
    if ((double)B * L * 3.0 * D * 4.0 >= 2.0e9) return UU3D_ERR_UNSUPPORTED;                 // 32-bit element offsets in the exact-f32 kernels
    AttnRule rule;                                                                          // precision f16x3, no switch set
    rule.forced = kernel;
    if (kernel == UU3D_ATTN_H3 ? (!planes_in || !planes_out) : (kernel != UU3D_ATTN_AUTO && planes_in)) return UU3D_ERR_INVALID_ARGUMENT;
    if (kernel == UU3D_ATTN_HEAD_WAVE && (L < 49 || L > 80 || H % 4 != 0)) return UU3D_ERR_INVALID_ARGUMENT;
    const int chosen = attn_choose(rule, L, H, planes_out, qfrag);
    if (chosen == ATTN_AUTO) return UU3D_ERR_UNSUPPORTED;                                    // beyond every kernel's length, as the forward answers
    if ((chosen == ATTN_H3) != planes_in) return UU3D_ERR_INVALID_ARGUMENT;                  // (UU3D_ATTN_AUTO only: the forced forms were checked above)
    const size_t lo_off = planes_out ? (size_t)B * L * D : 0;
    const int st = launch_attn_infer((hipStream_t)stream, reinterpret_cast<const float*>(qkv), D, B, L, H, mask, reinterpret_cast<float*>(out), lo_off, frag, qfrag, rule);
    return st != UU3D_OK ? st : hip_status();
}

// ---- the forward's tiled GEMMs (launch_fwd_gemm / launch_fwd_gemm_g, uu3d_launch.h: the launches Launcher::gemm / gemm_g make) ----
size_t uu3d_op_tiled_operand_bytes(int32_t N, int32_t K) { return (N < 1 || K < 1) ? 0 : (size_t)ru(N, 128) * ru(K, 32) * (sizeof(float) + 2 * sizeof(_Float16)); }

int uu3d_op_tiled_pack(const float* w, int32_t K, int32_t N, void* operand_dev, void* stream_) {
    if (!w || !operand_dev || K < 1 || N < 1) return UU3D_ERR_INVALID_ARGUMENT;
    const int Kp = ru(K, 32);
    const size_t n = (size_t)ru(N, 128) * Kp;
    std::vector<float> bt(n, 0.f);
    pack_dense_t(bt.data(), 0, w, K, N, Kp, 0);                      // the commit's pack and split (uu3d_pack.h)
    std::vector<_Float16> planes(2 * n);
    if (!split_operand_planes(bt.data(), n, planes.data(), planes.data() + n)) return UU3D_ERR_RANGE;
    hipStream_t stream = (hipStream_t)stream_;
    if (hipMemcpyAsync(operand_dev, bt.data(), n * sizeof(float), hipMemcpyHostToDevice, stream) != hipSuccess) return UU3D_ERR_HIP;
    if (hipMemcpyAsync(reinterpret_cast<float*>(operand_dev) + n, planes.data(), 2 * n * sizeof(_Float16), hipMemcpyHostToDevice, stream) != hipSuccess) return UU3D_ERR_HIP;
    return hipStreamSynchronize(stream) == hipSuccess ? UU3D_OK : UU3D_ERR_HIP;
}

int uu3d_op_tiled_split(int32_t M, int32_t N, int32_t K, int32_t target, size_t slab_floats, int32_t* slices, int32_t* kps) {
    if (M < 1 || N < 1 || K < 1 || target < 1 || !slices || !kps) return UU3D_ERR_INVALID_ARGUMENT;
    const SplitK s = splitk_rule(M, N, ru(K, 32) / 32, target, slab_floats, true);
    *slices = s.slices; *kps = s.kps;
    return UU3D_OK;
}

// >= 16 bytes of zeros on the device: what an out-of-range tap of GLoadConv3 reads (the forward's: the head of the model's f16 arena)
static const _Float16* conv_zero_source() {
    static const _Float16* const z = [] {
        void* p = nullptr;
        if (hipMalloc(&p, 128) != hipSuccess) return (const _Float16*)nullptr;
        if (hipMemset(p, 0, 128) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { (void)hipFree(p); return (const _Float16*)nullptr; }
        return (const _Float16*)p;
    }();
    return z;
}

int uu3d_op_tiled_dense(const uu3d_tiled_dense_args* a, void* stream_) {
    if (!a) return UU3D_ERR_INVALID_ARGUMENT;
    const int M = a->M, N = a->N, K = a->K, src = a->a_source, epi = a->epilogue;
    if (!a->a_dev || !a->operand_dev || !a->bias_dev || !a->out_dev || M < 1 || N < 1 || K < 1) return UU3D_ERR_INVALID_ARGUMENT;
    if ((a->precision != UU3D_PREC_F16X3 && a->precision != UU3D_PREC_F32) || a->splitk_target < 1 || (a->slab_floats != 0 && !a->slab_dev)) return UU3D_ERR_INVALID_ARGUMENT;
    const bool h3 = a->precision == UU3D_PREC_F16X3;
    const bool conv = src == UU3D_A_CONV3_F32 || src == UU3D_A_CONV3_PLANES, planes = src == UU3D_A_PLANES || src == UU3D_A_CONV3_PLANES;
    // the combinations uu3d_forward.inc launches (include/uu3d_ops.h lists them by call site)
    bool known = false;
    switch (src) {
        case UU3D_A_F32: known = epi == UU3D_EP_BIAS || epi == UU3D_EP_BIAS_RESIDUAL || epi == UU3D_EP_S2T; break;
        case UU3D_A_F32_LN: known = epi == UU3D_EP_BIAS || epi == UU3D_EP_BIAS_RELU || (h3 && (epi == UU3D_EP_BIAS_SPLIT_Q || epi == UU3D_EP_BIAS_RELU_SPLIT)); break;
        case UU3D_A_PLANES: known = h3 && (epi == UU3D_EP_BIAS_RESIDUAL || epi == UU3D_EP_S2T); break;
        case UU3D_A_CONV3_F32: known = epi == UU3D_EP_CONV_RESIDUAL; break;
        case UU3D_A_CONV3_PLANES: known = h3 && epi == UU3D_EP_CONV_RESIDUAL; break;
        default: break;
    }
    if (!known) return UU3D_ERR_INVALID_ARGUMENT;
    // the A source
    int lda = a->lda;
    if (conv) {
        const int Cc = a->conv_C;
        if (Cc < 1 || (Cc % (planes ? 32 : 4)) != 0 || (int64_t)K != (int64_t)3 * Cc || a->conv_L_in < 1 || a->conv_L_out < 1 || a->conv_stride < 1 || a->conv_pad_left < 0 ||
            M % a->conv_L_out != 0 || !a->xin_dev) return UU3D_ERR_INVALID_ARGUMENT;
        const int lo = (a->conv_stride > 1 && a->conv_pad_left == 0) ? 1 : 0;
        if ((int64_t)(a->conv_L_out - 1) * a->conv_stride + lo >= a->conv_L_in) return UU3D_ERR_INVALID_ARGUMENT;      // the identity row of the last output row
        if ((double)(M / a->conv_L_out) * a->conv_L_in * std::max(Cc, N) >= 536870912.0) return UU3D_ERR_UNSUPPORTED;
        lda = Cc;
    } else if (planes ? (K % 32 != 0 || lda < K || lda % 8 != 0) : (K % 4 != 0 || lda < K || lda % 4 != 0)) return UU3D_ERR_INVALID_ARGUMENT;
    if (planes && !a->a_lo_dev) return UU3D_ERR_INVALID_ARGUMENT;
    if (src == UU3D_A_F32_LN && (!a->ln_stats_dev || !a->ln_gamma_dev || !a->ln_beta_dev)) return UU3D_ERR_INVALID_ARGUMENT;
    // the epilogue
    if ((epi == UU3D_EP_BIAS || epi == UU3D_EP_BIAS_RELU) && a->ldo < N) return UU3D_ERR_INVALID_ARGUMENT;
    if (epi == UU3D_EP_BIAS_SPLIT_Q && N % 3 != 0) return UU3D_ERR_INVALID_ARGUMENT;
    const bool reads_pe = epi == UU3D_EP_S2T || (epi == UU3D_EP_BIAS_RESIDUAL && a->out2_dev != nullptr);
    if (reads_pe && (!a->pe_dev || a->period < 1)) return UU3D_ERR_INVALID_ARGUMENT;
    if (epi == UU3D_EP_S2T && a->mask_dev != nullptr && !a->token_dev) return UU3D_ERR_INVALID_ARGUMENT;
    if ((double)M * ru(std::max(std::max(N, lda), (epi == UU3D_EP_BIAS || epi == UU3D_EP_BIAS_RELU) ? a->ldo : N), 4) >= 536870912.0) return UU3D_ERR_UNSUPPORTED;   // 32-bit M * N in the combine's grid
    const _Float16* zero = nullptr;
    if (src == UU3D_A_CONV3_PLANES && (zero = conv_zero_source()) == nullptr) return UU3D_ERR_HIP;

    hipStream_t stream = (hipStream_t)stream_;
    const size_t nb = (size_t)ru(N, 128) * ru(K, 32);
    const float* Bt = reinterpret_cast<const float*>(a->operand_dev);
    const _Float16* Bh = reinterpret_cast<const _Float16*>(Bt + nb); const _Float16* Bl = Bh + nb;
    const float* Af = reinterpret_cast<const float*>(a->a_dev);
    const _Float16* Ah = reinterpret_cast<const _Float16*>(a->a_dev); const _Float16* Al = reinterpret_cast<const _Float16*>(a->a_lo_dev);
    float* outf = reinterpret_cast<float*>(a->out_dev);
    _Float16* oh = reinterpret_cast<_Float16*>(a->out_dev);
    auto rows = [&](const auto& al, const auto& ep) { launch_fwd_gemm(stream, al, Bt, Bh, Bl, M, N, K, ep, a->slab_dev, a->slab_floats, a->splitk_target, a->precision); };
    auto dma = [&](const auto& gl, const auto& ep) { launch_fwd_gemm_g(stream, gl, Bh, Bl, M, N, K, ep, a->slab_dev, a->slab_floats, a->splitk_target); };
    const EpBias ep_bias{outf, a->bias_dev, a->ldo};
    const EpBiasResidual ep_res{outf, a->bias_dev, N, a->out2_dev, a->out2_dev ? a->pe_dev : nullptr, a->out2_dev ? a->period : 1};
    const EpSpatialToTemporal ep_s2t{outf, a->bias_dev, N, a->mask_dev, a->token_dev, a->pe_dev, a->period};
    // MaxPool1D(pool 1, stride s) on the trimmed sequence; stride 1 keeps x untrimmed (the forward's strided_blocks)
    const int lo = (a->conv_stride > 1 && a->conv_pad_left == 0) ? 1 : 0;
    const EpConvResidual ep_conv{outf, a->bias_dev, N, a->xin_dev, a->conv_L_in, a->conv_L_out, a->conv_stride, lo, a->pe_dev};
    switch (src) {
        case UU3D_A_F32: {
            const ALoadPlain al{Af, lda, M, K};
            if (epi == UU3D_EP_BIAS) rows(al, ep_bias); else if (epi == UU3D_EP_BIAS_RESIDUAL) rows(al, ep_res); else rows(al, ep_s2t);
        } break;
        case UU3D_A_F32_LN: {
            const ALoadLayerNorm al{Af, reinterpret_cast<const float2*>(a->ln_stats_dev), a->ln_gamma_dev, a->ln_beta_dev, lda, M, K};
            if (epi == UU3D_EP_BIAS) rows(al, ep_bias);
            else if (epi == UU3D_EP_BIAS_RELU) rows(al, EpBiasRelu{outf, a->bias_dev, a->ldo});
            else if (epi == UU3D_EP_BIAS_RELU_SPLIT) rows(al, EpBiasReluSplit{oh, oh + (size_t)M * N, a->bias_dev, N});
            else rows(al, EpBiasSplitQ{oh, oh + (size_t)M * N, a->bias_dev, N, N / 3, a->qscale});
        } break;
        case UU3D_A_PLANES: {
            const GLoadPlain gl{Ah, Al, lda, M};
            if (epi == UU3D_EP_BIAS_RESIDUAL) dma(gl, ep_res); else dma(gl, ep_s2t);
        } break;
        case UU3D_A_CONV3_F32: rows(ALoadConv3{Af, a->conv_C, a->conv_L_in, a->conv_L_out, a->conv_stride, a->conv_pad_left, M, K}, ep_conv); break;
        default: dma(GLoadConv3{Ah, Al, zero, a->conv_C, a->conv_L_in, a->conv_L_out, a->conv_stride, a->conv_pad_left, M}, ep_conv); break;
    }
    return hip_status();
}

// ---- the training step's GEMM forms, each on its own (include/uu3d_ops.h: TRAINING GEMMS), through the step's own host dispatch ----
namespace {

// rows x ld of an operand block (uu3d_train_state.inc: dense / block): the GEMM reads it as Bt[rows][ld] with N <= rows, round_up(K, 32) == ld
struct TrainOperandDims { int rows, ld; };
bool train_operand_dims(int kind, int K, int N, int Cc, TrainOperandDims* d) {
    if (K < 1 || N < 1) return false;
    if ((double)K * N >= 268435456.0) return false;
    if (kind == 1) { *d = {ru(N, 128), ru(K, 32)}; return true; }                      // forward: Bt[round128(N)][Kp]
    if (kind == 4) { *d = {ru(K, 64), ru(N, 32)}; return true; }                       // backward: WK[round64(K)][round32(N)]
    if (kind == 5 && Cc >= 1 && K == 3 * Cc) { *d = {ru(Cc, 128), ru(3 * N, 32)}; return true; }   // conv-transpose: WT[round128(C)][round32(3 N)]
    return false;
}
// rows of the block a GEMM of output width N reads, by the kind of its operand
int train_operand_rows(int kind, int N) { return kind == 4 ? ru(N, 64) : ru(N, 128); }

dim3 ew_grid(long long n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

size_t uu3d_op_train_operand_bytes(int32_t kind, int32_t K, int32_t N, int32_t Cc) {
    TrainOperandDims d;
    return train_operand_dims(kind, K, N, Cc, &d) ? (size_t)d.rows * d.ld * (sizeof(float) + 2 * sizeof(_Float16)) : 0;
}

int uu3d_op_train_pack(const float* w_dev, int32_t kind, int32_t K, int32_t N, int32_t Cc, void* operand_dev, void* stream_) {
    TrainOperandDims d;
    if (!w_dev || !operand_dev || !train_operand_dims(kind, K, N, Cc, &d)) return UU3D_ERR_INVALID_ARGUMENT;
    hipStream_t stream = (hipStream_t)stream_;
    const size_t n = (size_t)d.rows * d.ld;
    const PackDesc desc{0, 0, kind, K, N, d.ld, 0, kind == 5 ? Cc : 0};
    const int first = 0;
    char* table = nullptr;                                           // the one-entry descriptor table of this call
    if (hipMalloc((void**)&table, 256) != hipSuccess) return UU3D_ERR_HIP;
    int st = UU3D_OK;
    if (hipMemcpyAsync(table, &desc, sizeof(desc), hipMemcpyHostToDevice, stream) != hipSuccess ||
        hipMemcpyAsync(table + 128, &first, sizeof(first), hipMemcpyHostToDevice, stream) != hipSuccess ||
        hipMemsetAsync(operand_dev, 0, n * (sizeof(float) + 2 * sizeof(_Float16)), stream) != hipSuccess) st = UU3D_ERR_HIP;
    if (st == UU3D_OK) {
        float* arena = reinterpret_cast<float*>(operand_dev);
        hipLaunchKernelGGL(repack_kernel, dim3(repack_blocks(kind, K, N)), dim3(256), 0, stream, w_dev, arena, reinterpret_cast<const PackDesc*>(table),
                           reinterpret_cast<const int*>(table + 128), 1, reinterpret_cast<_Float16*>(arena + n), (long long)n);
        st = hip_status();
    }
    if (hipStreamSynchronize(stream) != hipSuccess && st == UU3D_OK) st = UU3D_ERR_HIP;      // (the table is the call's own)
    (void)hipFree(table);
    return st;
}

int uu3d_op_train_dense(const uu3d_train_dense_args* a, void* stream_) {
    if (!a) return UU3D_ERR_INVALID_ARGUMENT;
    const int M = a->M, N = a->N, K = a->K, src = a->a_source, epi = a->epilogue, kind = a->operand_kind;
    if (!a->a_dev || !a->operand_dev || !a->out_dev || M < 1 || N < 1 || K < 4 || (K & 3)) return UU3D_ERR_INVALID_ARGUMENT;
    if ((a->precision != UU3D_PREC_F16X3 && a->precision != UU3D_PREC_F32) || (a->slab_floats != 0 && !a->slab_dev)) return UU3D_ERR_INVALID_ARGUMENT;
    // the combinations the training step launches (include/uu3d_ops.h lists them by call site)
    bool known = false;
    switch (src) {
        case UU3D_TA_PLAIN: known = (kind == 1 && epi == UU3D_TEP_BIAS_RES_GATE) ||
                                    (kind == 4 && (epi == UU3D_TEP_STORE || epi == UU3D_TEP_ADD || epi == UU3D_TEP_RELU_MASK || epi == UU3D_TEP_GELU_GRAD)); break;
        case UU3D_TA_LN: known = kind == 1 && (epi == UU3D_TEP_BIAS || epi == UU3D_TEP_BIAS_RELU); break;
        case UU3D_TA_GELU: known = kind == 1 && epi == UU3D_TEP_BIAS_RES_GATE; break;
        case UU3D_TA_CONV3: known = kind == 1 && epi == UU3D_TEP_CONV_RESIDUAL; break;
        case UU3D_TA_CONVT: known = kind == 5 && epi == UU3D_TEP_RELU_MASK; break;
        default: break;
    }
    if (!known) return UU3D_ERR_INVALID_ARGUMENT;
    const bool conv = src == UU3D_TA_CONV3 || src == UU3D_TA_CONVT;
    int lda = a->lda;
    if (conv) {
        const int Cc = a->conv_C;                                    // channels of a gathered row
        if (Cc < 4 || (Cc & 3) || (int64_t)K != (int64_t)3 * Cc || a->conv_L_in < 1 || a->conv_L_out < 1 || a->conv_stride < 1 || a->conv_pad_left < 0) return UU3D_ERR_INVALID_ARGUMENT;
        if (M % (src == UU3D_TA_CONV3 ? a->conv_L_out : a->conv_L_in) != 0) return UU3D_ERR_INVALID_ARGUMENT;
        lda = Cc;
    } else if (lda < K || (lda & 3)) return UU3D_ERR_INVALID_ARGUMENT;
    if (src == UU3D_TA_LN && (!a->ln_stats_dev || !a->ln_gamma_dev || !a->ln_beta_dev)) return UU3D_ERR_INVALID_ARGUMENT;
    const int ldo = a->ldo;
    if (ldo < N) return UU3D_ERR_INVALID_ARGUMENT;
    const bool bias = epi == UU3D_TEP_BIAS || epi == UU3D_TEP_BIAS_RELU || epi == UU3D_TEP_BIAS_RES_GATE || epi == UU3D_TEP_CONV_RESIDUAL;
    if (bias && !a->bias_dev) return UU3D_ERR_INVALID_ARGUMENT;
    const bool aux = epi == UU3D_TEP_BIAS_RES_GATE || epi == UU3D_TEP_CONV_RESIDUAL || epi == UU3D_TEP_RELU_MASK || epi == UU3D_TEP_GELU_GRAD;
    if (aux && !a->aux_dev) return UU3D_ERR_INVALID_ARGUMENT;
    const bool gated = epi == UU3D_TEP_BIAS_RES_GATE || epi == UU3D_TEP_CONV_RESIDUAL;
    if (gated && ((a->gate_dev != nullptr && (!(a->keep > 0.f) || a->rps < 1)) || !(a->drop_rate >= 0.f) || !(a->drop_rate < 1.f))) return UU3D_ERR_INVALID_ARGUMENT;
    if (epi == UU3D_TEP_BIAS_RES_GATE && a->out2_dev != nullptr && (!a->pe_dev || a->period < 1)) return UU3D_ERR_INVALID_ARGUMENT;
    int lo = 0;
    if (epi == UU3D_TEP_CONV_RESIDUAL) {
        lo = (a->conv_stride > 1 && a->conv_pad_left == 0) ? 1 : 0;
        if ((int64_t)(a->conv_L_out - 1) * a->conv_stride + lo >= a->conv_L_in) return UU3D_ERR_INVALID_ARGUMENT;      // the identity row of the last output row
        if (a->gate_dev != nullptr && a->rps != a->conv_L_out) return UU3D_ERR_INVALID_ARGUMENT;                      // one gate per sequence
    }
    const int Kp = ru(K, 32);
    const double in_rows = src == UU3D_TA_CONV3 ? (double)(M / a->conv_L_out) * a->conv_L_in : (src == UU3D_TA_CONVT ? (double)(M / a->conv_L_in) * a->conv_L_out : (double)M);
    if ((double)M * ru(std::max(N, ldo), 4) >= 536870912.0 || in_rows * std::max(lda, ldo) >= 536870912.0) return UU3D_ERR_UNSUPPORTED;   // 32-bit M * N in the combine's grid

    hipStream_t stream = (hipStream_t)stream_;
    const size_t nb = (size_t)train_operand_rows(kind, N) * Kp;
    const float* Bt = reinterpret_cast<const float*>(a->operand_dev);
    const bool h3 = a->precision == UU3D_PREC_F16X3;
    const _Float16* Bh = h3 ? reinterpret_cast<const _Float16*>(Bt + nb) : nullptr; const _Float16* Bl = h3 ? Bh + nb : nullptr;
    int st = UU3D_OK;
    auto go = [&](const auto& al, const auto& ep) { st = launch_gemm(al, Bt, M, N, K, ep, a->slab_dev, a->slab_floats, stream, Bh, Bl); };
    const DropCfg drop = drop_cfg(gated ? a->drop_rate : 0.f, a->drop_seed, a->drop_site);
    const EpBiasResGate ep_gate{a->out_dev, a->aux_dev, a->bias_dev, ldo, a->gate_dev, a->keep, a->rps, a->out2_dev, a->out2_dev ? a->pe_dev : nullptr,
                                a->out2_dev ? a->period : 1, drop};
    const float scale = a->scale;
    switch (src) {
        case UU3D_TA_PLAIN: {
            const ALoadPlain al{a->a_dev, lda, M, K};
            if (epi == UU3D_TEP_BIAS_RES_GATE) go(al, ep_gate);
            else if (epi == UU3D_TEP_STORE) go(al, EpStore{a->out_dev, ldo});
            else if (epi == UU3D_TEP_ADD) go(al, EpAdd{a->out_dev, ldo});
            else if (epi == UU3D_TEP_RELU_MASK) go(al, EpReluMask{a->out_dev, a->aux_dev, ldo, scale});
            else go(al, EpGeluGrad{a->out_dev, a->aux_dev, ldo});
        } break;
        case UU3D_TA_LN: {
            const ALoadLayerNorm al{a->a_dev, reinterpret_cast<const float2*>(a->ln_stats_dev), a->ln_gamma_dev, a->ln_beta_dev, lda, M, K};
            if (epi == UU3D_TEP_BIAS) go(al, EpBias{a->out_dev, a->bias_dev, ldo}); else go(al, EpBiasRelu{a->out_dev, a->bias_dev, ldo});
        } break;
        case UU3D_TA_GELU: go(ALoadGelu{a->a_dev, lda, M, K}, ep_gate); break;
        case UU3D_TA_CONV3:
            go(ALoadConv3{a->a_dev, a->conv_C, a->conv_L_in, a->conv_L_out, a->conv_stride, a->conv_pad_left, M, K},
               EpConvResidual{a->out_dev, a->bias_dev, ldo, a->aux_dev, a->conv_L_in, a->conv_L_out, a->conv_stride, lo, a->pe_dev, a->gate_dev, a->keep, drop});
            break;
        default:
            go(ALoadConvT{a->a_dev, a->conv_C, a->conv_L_in, a->conv_L_out, a->conv_stride, a->conv_pad_left, M, K}, EpReluMask{a->out_dev, a->aux_dev, ldo, scale});
            break;
    }
    return st;
}

int uu3d_op_train_wgrad(const uu3d_train_wgrad_args* a, void* stream_) {
    if (!a) return UU3D_ERR_INVALID_ARGUMENT;
    const int R = a->R, P = a->P, Q = a->Q, src = a->a_source, epi = a->epilogue;
    if (!a->a_dev || !a->b_dev || !a->out_dev || R < 1 || P < 4 || Q < 4 || (P & 3) || (Q & 3) || a->ldb < Q || (a->ldb & 3)) return UU3D_ERR_INVALID_ARGUMENT;
    if ((a->slab_floats != 0 && !a->slab_dev) || (a->h3 != 0 && a->h3 != 1)) return UU3D_ERR_INVALID_ARGUMENT;
    // the combinations the training step launches
    const bool known = (epi == UU3D_WEP_STORE && (src == UU3D_TA_PLAIN || src == UU3D_TA_LN || src == UU3D_TA_GELU || src == UU3D_TA_CONV3)) ||
                       (epi == UU3D_WEP_STORE3 && src == UU3D_TA_LN);
    if (!known) return UU3D_ERR_INVALID_ARGUMENT;
    if (src == UU3D_TA_CONV3) {
        const int Cc = a->conv_C;
        if (Cc < 4 || (Cc & 3) || (int64_t)P != (int64_t)3 * Cc || a->conv_L_in < 1 || a->conv_L_out < 1 || a->conv_stride < 1 || a->conv_pad_left < 0 ||
            R % a->conv_L_out != 0) return UU3D_ERR_INVALID_ARGUMENT;
        if ((double)(R / a->conv_L_out) * a->conv_L_in * Cc >= 536870912.0) return UU3D_ERR_UNSUPPORTED;
    } else if (a->lda < P || (a->lda & 3)) return UU3D_ERR_INVALID_ARGUMENT;
    if (src == UU3D_TA_LN && (!a->ln_stats_dev || !a->ln_gamma_dev || !a->ln_beta_dev)) return UU3D_ERR_INVALID_ARGUMENT;
    if (epi == UU3D_WEP_STORE3 ? (!a->out1_dev || !a->out2_dev || Q % 3 != 0) : a->ldo < Q) return UU3D_ERR_INVALID_ARGUMENT;
    if ((double)R * std::max(a->lda, a->ldb) >= 536870912.0 || (double)P * std::max(Q, a->ldo) >= 536870912.0) return UU3D_ERR_UNSUPPORTED;

    hipStream_t stream = (hipStream_t)stream_;
    int st = UU3D_OK;
    auto go = [&](const auto& al, const auto& ep) { st = launch_gemm_tn(al, a->b_dev, a->ldb, R, P, Q, ep, a->slab_dev, a->slab_dev ? a->slab_floats : 0, stream, a->h3 != 0); };
    const EpStore ep{a->out_dev, a->ldo};
    switch (src) {
        case UU3D_TA_PLAIN: go(TnLoadPlain{a->a_dev, a->lda, R, P}, ep); break;
        case UU3D_TA_LN: {
            const TnLoadLayerNorm al{a->a_dev, reinterpret_cast<const float2*>(a->ln_stats_dev), a->ln_gamma_dev, a->ln_beta_dev, a->lda, R, P};
            if (epi == UU3D_WEP_STORE3) go(al, EpStore3{a->out_dev, a->out1_dev, a->out2_dev, Q / 3}); else go(al, ep);
        } break;
        case UU3D_TA_GELU: go(TnLoadGelu{a->a_dev, a->lda, R, P}, ep); break;
        default: go(TnLoadConv3{a->a_dev, a->conv_C, a->conv_L_in, a->conv_L_out, a->conv_stride, a->conv_pad_left, R, P}, ep); break;
    }
    return st;
}

int uu3d_op_colsum3(const float* x, int32_t ldx, int32_t R, int32_t seg, float* out0, float* out1, float* out2, int32_t accumulate,
                    float* scratch, size_t scratch_floats, void* stream) {
    if (!x || !out0 || !out1 || !out2 || !scratch || R < 1 || seg < 1 || seg > 178956970 || ldx < 3 * seg) return UU3D_ERR_INVALID_ARGUMENT;
    return launch_colsum(x, ldx, R, 3 * seg, 0, nullptr, 0, ReduceOut{out0, out1, out2, seg}, accumulate, scratch, scratch_floats, (hipStream_t)stream);
}

int uu3d_op_ln_bwd_ex(const float* x, const float* dy, const float* stats, const float* gamma, int32_t ld, int32_t D, int32_t M, float* dx,
                      const float* res, const float* gate, float keep, int32_t rps, float* gated_out, float* dgamma, float* dbeta,
                      float* scratch, size_t scratch_floats, void* stream_) {
    if (!x || !dy || !stats || !gamma || !dx || !dgamma || !dbeta || !scratch || D < 4 || (D & 3) || D > 1024 || M < 1 || ld < D || (ld & 3)) return UU3D_ERR_INVALID_ARGUMENT;
    if ((gate != nullptr) != (gated_out != nullptr) || (gate != nullptr && (!(keep > 0.f) || rps < 1))) return UU3D_ERR_INVALID_ARGUMENT;
    if ((size_t)2 * D > scratch_floats) return UU3D_ERR_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    const LnBwdGated gated = gate != nullptr ? LnBwdGated{gate, keep, rps, gated_out} : LnBwdGated{nullptr, 1.f, 1, nullptr};
    const int slices = launch_ln_bwd_rows(x, dy, (const float2*)stats, gamma, ld, D, M, dx, res != nullptr, res, scratch, scratch_floats, stream, gated);
    launch_ln_bwd_combine(scratch, D, slices, dgamma, dbeta, 0, stream);
    return hip_status();
}

int uu3d_op_identity_bwd(const float* dout, int32_t B, int32_t L_in, int32_t L_out, int32_t stride, int32_t lo, int32_t D, float* dmid, void* stream) {
    if (!dout || !dmid || B < 1 || L_in < 1 || L_out < 1 || stride < 1 || lo < 0 || D < 1) return UU3D_ERR_INVALID_ARGUMENT;
    if ((double)B * std::max(L_in, L_out) * D >= 2147483648.0) return UU3D_ERR_UNSUPPORTED;       // 32-bit element index in the kernel
    hipLaunchKernelGGL(identity_bwd_kernel, ew_grid((long long)B * L_in * D), dim3(256), 0, (hipStream_t)stream, dout, B, L_in, L_out, stride, lo, D, dmid);
    return hip_status();
}

int uu3d_op_scale_rows(const float* in, int32_t rows, int32_t D, const float* gate, float keep, int32_t rps, const uint8_t* row_mask, int32_t want,
                       float* out, void* stream) {
    if (!in || !out || rows < 1 || D < 1 || (gate != nullptr && (!(keep > 0.f) || rps < 1)) || (want != 0 && want != 1)) return UU3D_ERR_INVALID_ARGUMENT;
    if ((double)rows * D >= 2147483648.0) return UU3D_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(scale_rows_kernel, ew_grid((long long)rows * D), dim3(256), 0, (hipStream_t)stream, in, rows, D, gate, keep, rps, row_mask, want, out);
    return hip_status();
}
