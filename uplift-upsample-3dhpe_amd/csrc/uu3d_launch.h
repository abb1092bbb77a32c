// uu3d_launch.h -- host-side launch helpers shared by the ops ABI, the forward and the training step.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include "../../include/uu3d.h"
#include "uu3d_gemm.h"
#include "uu3d_gemm_h3.h"
#include "uu3d_bwd.h"
#include "uu3d_attn_long.h"
#include "uu3d_gemm_panel.h"
#include "uu3d_gemm_panel8.h"
#include "uu3d_gemm_wt.h"
#include "uu3d_mlp_fused.h"
#include "uu3d_attn.h"
#include "uu3d_attn_h3.h"
#include "uu3d_tchain16.h"

namespace uu3d {

// Dynamic LDS beyond the 64 KiB default needs hipFuncAttributeMaxDynamicSharedMemorySize on the kernel: set once per process for
// every instantiation that is launched (one device per process).  allow_lds<kernel<...>>(bytes) in front of the launch.
template <auto Kern>
inline void allow_lds(size_t bytes) {
    static const bool once = (hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess);
    (void)once;
}

// Split-K of the tiled forward GEMMs (64 x 64 tiles, k-tiles of 32): problems with too few tiles to fill the chip are cut along K into
// slabs and combined in order (splitk_reduce_kernel).  Returns {slices, k-tiles per slice}; {1, KT} = unsplit.
//   target: workgroups the launch aims for;  slab_floats: capacity of the partial-sum buffer (0: none, never split);
//   full_chip_exception: >= 200 tiles with a short contraction fill the chip unsplit (strided block 2's projection, 276 tiles x 12 k-tiles,
//   13.3 us against 12.6 + 6.5 us split three ways + reduce; the heads and the K = 2304 convolutions measured faster split)
struct SplitK { int slices, kps; };
inline SplitK splitk_rule(int M, int N, int KT, int target, size_t slab_floats, bool full_chip_exception) {
    const int tiles = ((M + 63) / 64) * ((N + 63) / 64);
    int slices = 1;
    if (tiles < 384 && KT >= 8 && !(full_chip_exception && tiles >= 200 && KT <= 16)) slices = std::max(1, std::min(KT / 4, (target + tiles / 2) / tiles));
    int kps = (KT + slices - 1) / slices;
    slices = (KT + kps - 1) / kps;
    if (slices > 1 && (size_t)slices * M * ((N + 3) / 4 * 4) > slab_floats) { slices = 1; kps = KT; }
    return {slices, kps};
}

constexpr size_t kOpScratchFloats = (size_t)1536 * 4096;

inline int ru(int v, int m) { return (v + m - 1) / m * m; }
inline hipError_t& last_launch_error() { static thread_local hipError_t e = hipSuccess; return e; }      // what hip_status() last consumed (for the error text)
inline int hip_status() { const hipError_t e = hipGetLastError(); if (e != hipSuccess) last_launch_error() = e; return e == hipSuccess ? UU3D_OK : UU3D_ERR_HIP; }

// C = A-op x Bt^T with the forward GEMM kernel (64x64 tiles, deterministic split-K when few tiles).
// Bh / Bl != nullptr: the operand's f16 hi / lo planes (same [Np][Kp] layout) -> f16x3 kernel (uu3d_gemm_h3.h).
template <class AL, class EP>
int launch_gemm(const AL& al, const float* Bt, int M, int N, int K, const EP& ep, float* slab, size_t slab_floats, hipStream_t stream,
                const _Float16* Bh = nullptr, const _Float16* Bl = nullptr) {
    const int Kp = ru(K, 32), KT = Kp / 32;
    const auto [slices, kps] = splitk_rule(M, N, KT, 768, slab == nullptr ? 0 : slab_floats, false);     // (training step: 384 / 1536 target workgroups measure +0.5 %, no split +6 %)
    const int ldslab = ru(N, 4);
    const int mt = (M + 63) / 64, nt = (N + 63) / 64;
    const int grid = ru(mt, 8) * nt;
    if (Bh != nullptr && Bl != nullptr) {
        constexpr size_t ldsh = gemm_h3_lds_bytes(64, 64);
        if (slices == 1) {
            if (gemm_h3_deep(grid)) hipLaunchKernelGGL((gemm_h3_kernel<1, 1, AL, EP, 1>), dim3(grid, 1), dim3(256), ldsh, stream, al, Bh, Bl, M, N, Kp, mt, nt, KT, ep);
            else hipLaunchKernelGGL((gemm_h3_kernel<1, 1, AL, EP>), dim3(grid, 1), dim3(256), ldsh, stream, al, Bh, Bl, M, N, Kp, mt, nt, KT, ep);
        } else {
            EpSlab es{slab, ldslab, (size_t)M * ldslab};
            if (gemm_h3_deep(grid * slices)) hipLaunchKernelGGL((gemm_h3_kernel<1, 1, AL, EpSlab, 1>), dim3(grid, slices), dim3(256), ldsh, stream, al, Bh, Bl, M, N, Kp, mt, nt, kps, es);
            else hipLaunchKernelGGL((gemm_h3_kernel<1, 1, AL, EpSlab>), dim3(grid, slices), dim3(256), ldsh, stream, al, Bh, Bl, M, N, Kp, mt, nt, kps, es);
            hipLaunchKernelGGL(splitk_reduce_kernel<EP>, dim3((M * N + 255) / 256), dim3(256), 0, stream, slab, slices,
                               (size_t)M * ldslab, M, N, ldslab, ep);
        }
        return hip_status();
    }
    constexpr size_t lds = gemm_lds_bytes(64, 64);
    if (slices == 1) {
        hipLaunchKernelGGL((gemm_f32_kernel<64, 64, AL, EP>), dim3(grid, 1), dim3(256), lds, stream, al, Bt, M, N, Kp, mt, nt, KT, ep);
    } else {
        EpSlab es{slab, ldslab, (size_t)M * ldslab};
        hipLaunchKernelGGL((gemm_f32_kernel<64, 64, AL, EpSlab>), dim3(grid, slices), dim3(256), lds, stream, al, Bt, M, N, Kp, mt, nt, kps, es);
        hipLaunchKernelGGL(splitk_reduce_kernel<EP>, dim3((M * N + 255) / 256), dim3(256), 0, stream, slab, slices,
                           (size_t)M * ldslab, M, N, ldslab, ep);
    }
    return hip_status();
}

inline int tnh_target_wgs() { return process_switches().tnh_wgs; }     // (UU3D_TNH_WGS, default 192) these GEMMs share the chip with the activation-gradient chain: fewer, longer workgroups and half the combine traffic (384: 3.74 ms per step, 192: 3.60, 128: 3.61, 96: 3.65)
// C[P][Q] = A^T B over R rows, split over R into slabs, combined in order.
template <class AL, class EP>
int launch_gemm_tn(const AL& al, const float* B, int ldb, int R, int P, int Q, const EP& ep, float* slab, size_t slab_floats, hipStream_t stream,
                   bool h3 = false) {
    if (h3 && P >= 128 && Q >= 128) {        // f16x3 on 128 x 128 tiles (gemm_tn_h3_kernel); narrow results stay on the exact-f32 kernel
        const int pt = (P + 127) / 128, qt = (Q + 127) / 128, tiles = pt * qt;
        const int KT = (R + 31) / 32;
        const int ldslab = ru(Q, 4);
        int slices = std::max(1, std::min(KT / 2, (tnh_target_wgs() + tiles - 1) / tiles));
        while (slices > 1 && (size_t)slices * P * ldslab > slab_floats) --slices;
        const int kps = (KT + slices - 1) / slices;
        slices = (KT + kps - 1) / kps;
        auto k1 = gemm_tn_h3_kernel<AL, EP>; auto ks = gemm_tn_h3_kernel<AL, EpSlab>;
        allow_lds<gemm_tn_h3_kernel<AL, EP>>(TNH_LDS_BYTES); allow_lds<gemm_tn_h3_kernel<AL, EpSlab>>(TNH_LDS_BYTES);
        if (slices == 1) {
            hipLaunchKernelGGL(k1, dim3(tiles, 1), dim3(256), TNH_LDS_BYTES, stream, al, B, ldb, R, P, Q, pt, qt, KT, ep);
        } else {
            EpSlab es{slab, ldslab, (size_t)P * ldslab};
            hipLaunchKernelGGL(ks, dim3(tiles, slices), dim3(256), TNH_LDS_BYTES, stream, al, B, ldb, R, P, Q, pt, qt, kps, es);
            hipLaunchKernelGGL(splitk_reduce_kernel<EP>, dim3((P * Q + 255) / 256), dim3(256), 0, stream, slab, slices,
                               (size_t)P * ldslab, P, Q, ldslab, ep);
        }
        return hip_status();
    }
    const int pt = (P + 63) / 64, qt = (Q + 63) / 64, tiles = pt * qt;
    const int KT = (R + 31) / 32;
    // <= 48 slabs when the combine is one thread per element; tall-skinny results (<= 4 tiles, e.g. the spatial stack's
    // 32 x 32 weight gradients over 77k rows) take up to 256 slabs and the 16-lane combine instead (512 slabs: +1.4 % per training step)
    const bool skinny = tiles <= 4 && KT >= 256;
    int slices = skinny ? std::max(1, std::min(KT / 4, 256 / tiles))
                        : std::max(1, std::min(std::min(std::max(KT / 4, 1), 48), (1024 + tiles / 2) / tiles));
    const int ldslab = ru(Q, 4);
    while (slices > 1 && (size_t)slices * P * ldslab > slab_floats) --slices;
    int kps = (KT + slices - 1) / slices;
    slices = (KT + kps - 1) / kps;
    if (slices == 1) {
        hipLaunchKernelGGL((gemm_tn_kernel<AL, EP>), dim3(tiles, 1), dim3(256), 0, stream, al, B, ldb, R, P, Q, pt, qt, KT, ep);
    } else {
        EpSlab es{slab, ldslab, (size_t)P * ldslab};
        hipLaunchKernelGGL((gemm_tn_kernel<AL, EpSlab>), dim3(tiles, slices), dim3(256), 0, stream, al, B, ldb, R, P, Q, pt, qt, kps, es);
        if (skinny)
            hipLaunchKernelGGL(splitk_reduce16_kernel<EP>, dim3((P * Q + 15) / 16), dim3(256), 0, stream, slab, slices,
                               (size_t)P * ldslab, P, Q, ldslab, ep);
        else
            hipLaunchKernelGGL(splitk_reduce_kernel<EP>, dim3((P * Q + 255) / 256), dim3(256), 0, stream, slab, slices,
                               (size_t)P * ldslab, P, Q, ldslab, ep);
    }
    return hip_status();
}

inline int launch_colsum(const float* x, int ldx, int R, int C, int period, const uint8_t* mask, int want, const ReduceOut out,
                         int accumulate, float* scratch, size_t scratch_floats, hipStream_t stream) {
    const int P = period > 0 ? period : 1;
    int slices = std::max(1, std::min(256, R / std::max(128, P)));      // >= 128 rows (and one period) per workgroup
    while (slices > 1 && (size_t)slices * P * C > scratch_floats) --slices;
    if ((size_t)slices * P * C > scratch_floats) return UU3D_ERR_WORKSPACE;
    if (period > 0 && mask == nullptr && (C % 4) == 0 && (ldx % 4) == 0 && R % period == 0) {
        const int nb = R / period, xb = (period * (C / 4) + 255) / 256;
        slices = std::max(1, std::min(std::max(1, 512 / xb), nb / 4));         // ~512 workgroups, >= 4 samples per thread
        while (slices > 1 && (size_t)slices * P * C > scratch_floats) --slices;
        if ((size_t)slices * P * C > scratch_floats) return UU3D_ERR_WORKSPACE;
        hipLaunchKernelGGL(colsum_period4_kernel, dim3(xb, slices), dim3(256), 0, stream, x, ldx, nb, period, C, scratch, slices);
    } else
    if (period <= 0 && mask == nullptr && (C % 4) == 0 && (ldx % 4) == 0) {
        const int cgs = std::max(1, std::min(64, (C + 3) / 4));
        const int xb = (C + 4 * cgs - 1) / (4 * cgs);
        slices = std::max(1, std::min(std::max(1, 320 / xb), R / 64));    // ~one workgroup per CU, >= 64 rows each; more slabs only move the time into the combine
        while (slices > 1 && (size_t)slices * C > scratch_floats) --slices;
        hipLaunchKernelGGL(colsum4_kernel, dim3(xb, slices), dim3(256), 0, stream, x, ldx, R, C, scratch, slices, cgs);
    } else
    hipLaunchKernelGGL(colsum_kernel, dim3((C + 63) / 64, slices), dim3(256), 0, stream, x, ldx, R, C, period, mask, want, scratch, slices);
    launch_reduce_partials(scratch, P * C, (size_t)P * C, slices, out, accumulate, stream);
    return hip_status();
}
inline int launch_colsum(const float* x, int ldx, int R, int C, int period, const uint8_t* mask, int want, float* out,
                         int accumulate, float* scratch, size_t scratch_floats, hipStream_t stream) {
    const int n = (period > 0 ? period : 1) * C;
    return launch_colsum(x, ldx, R, C, period, mask, want, ReduceOut{out, nullptr, nullptr, n > 0 ? n : 1}, accumulate, scratch, scratch_floats, stream);
}

// LayerNorm backward in two launches: the row kernel (dx, per-workgroup partial dgamma / dbeta in scratch; returns the number of
// partial slices) and the combine of the partials, which may run on another stream behind the first.
// accumulate: dx = res + d x (res == nullptr: dx itself, in place).
// Returns 0 without a launch when scratch cannot hold even one workgroup's partials (2 D floats) or there are no rows.
inline int launch_ln_bwd_rows(const float* x, const float* dy, const float2* stats, const float* gamma, int ld, int D, int M, float* dx,
                              int accumulate, const float* res, float* scratch, size_t scratch_floats, hipStream_t stream,
                              const LnBwdGated gated = LnBwdGated{nullptr, 1.f, 1, nullptr}) {
    if (!res) res = dx;
    if (M < 1 || D < 1 || (size_t)2 * D > scratch_floats) return 0;
    // wide rows (D = 384): >= 500 workgroups at M = 4544 (8 rows per wave left 114 of 256 CUs idle), <= 2048 partial rows;
    // the spatial stack's D = 32 rows are cheap and many (77 k): fewer, longer workgroups keep the combine short
    if ((D == 32 || D == 64) && ld % 4 == 0) {          // narrow rows: D / 4 lanes per row, 256 * 4 / D rows per workgroup at once
        const int RG = 1024 / D;
        int rpg = std::max(4, (M + RG * 512 - 1) / (RG * 512));
        int wgs = (M + RG * rpg - 1) / (RG * rpg);
        while (wgs > 1 && (size_t)wgs * 2 * D > scratch_floats) { rpg *= 2; wgs = (M + RG * rpg - 1) / (RG * rpg); }
        if (D == 32) hipLaunchKernelGGL(ln_bwd_narrow_kernel<8>, dim3(wgs), dim3(256), 0, stream, x, dy, stats, gamma, ld, M, rpg, dx, res, accumulate, scratch, gated);
        else hipLaunchKernelGGL(ln_bwd_narrow_kernel<16>, dim3(wgs), dim3(256), 0, stream, x, dy, stats, gamma, ld, M, rpg, dx, res, accumulate, scratch, gated);
        return wgs;
    }
    int rpw = (D > 64) ? std::max(2, (M + 4 * 2048 - 1) / (4 * 2048)) : std::max(8, (M + 4 * 512 - 1) / (4 * 512));
    int wgs = (M + 4 * rpw - 1) / (4 * rpw);
    while (wgs > 1 && (size_t)wgs * 2 * D > scratch_floats) { rpw *= 2; wgs = (M + 4 * rpw - 1) / (4 * rpw); }
    if (D <= 512) hipLaunchKernelGGL(ln_bwd_kernel<2>, dim3(wgs), dim3(256), 0, stream, x, dy, stats, gamma, ld, D, M, rpw, dx, res, accumulate, scratch, gated);
    else hipLaunchKernelGGL(ln_bwd_kernel<4>, dim3(wgs), dim3(256), 0, stream, x, dy, stats, gamma, ld, D, M, rpw, dx, res, accumulate, scratch, gated);
    return wgs;
}

// partial layout [slice][2][D]; dgamma/dbeta: written (acc_params == 0) or accumulated
inline void launch_ln_bwd_combine(const float* scratch, int D, int slices, float* dgamma, float* dbeta, int acc_params, hipStream_t stream) {
    if (dbeta == dgamma + D) {      // gamma and beta are neighbours in the flat gradient buffer: one combine over [dgamma | dbeta]
        launch_reduce_partials(scratch, 2 * D, (size_t)2 * D, slices, dgamma, acc_params, stream);
    } else {
        launch_reduce_partials(scratch, D, (size_t)2 * D, slices, dgamma, acc_params, stream);
        launch_reduce_partials(scratch + D, D, (size_t)2 * D, slices, dbeta, acc_params, stream);
    }
}

inline int launch_ln_bwd(const float* x, const float* dy, const float2* stats, const float* gamma, int ld, int D, int M, float* dx,
                         int accumulate, float* dgamma, float* dbeta, int acc_params, float* scratch, size_t scratch_floats, hipStream_t stream) {
    if (M < 1 || D < 1) return UU3D_ERR_INVALID_ARGUMENT;
    if ((size_t)2 * D > scratch_floats) return UU3D_ERR_WORKSPACE;
    const int slices = launch_ln_bwd_rows(x, dy, stats, gamma, ld, D, M, dx, accumulate, nullptr, scratch, scratch_floats, stream);
    launch_ln_bwd_combine(scratch, D, slices, dgamma, dbeta, acc_params, stream);
    return hip_status();
}

// head dims the generic forward kernel is instantiated for (launch_attn_generic)
inline bool attn_generic_head_dim_ok(int dh) { return dh == 2 || dh == 4 || dh == 8 || dh == 12 || dh == 16 || dh == 24 || dh == 32 || dh == 48 || dh == 64; }

// drop: Dropout on the attention weights (training with ATTENTION_DROP_RATE > 0) -- only the generic kernels implement it, so the
// unrolled / MFMA backward kernels are not taken then
// bwd_generic (UU3D_ATTN_BWD_GENERIC): the backward stays on the generic kernel for every shape
inline int launch_attn_generic(bool backward, const float* qkv, const float* dO, int ld, int D, int B, int L, int H, int dh,
                               const uint8_t* mask, float* out, int ldo, hipStream_t stream, const DropCfg drop = DropCfg{}, bool bwd_generic = false) {
    const int total = B * H;
    const dim3 block(128);
    if (dh != 4 && dh != 48) {
        // other head dims (generic-dims models, uu3d_create): thread = query row, one (sequence, head) per workgroup
        if (L > 128) return UU3D_ERR_UNSUPPORTED;
        const dim3 grid(total);
#define UU3D_ATTNG_CASE(d) case d: { allow_lds<attn_generic_fwd_kernel<d>>(160 * 1024); allow_lds<attn_generic_bwd_kernel<d>>(160 * 1024); \
            if (attn_generic_lds_bytes<d>(L, backward) > (size_t)160 * 1024) return UU3D_ERR_UNSUPPORTED; \
            if (backward) hipLaunchKernelGGL(attn_generic_bwd_kernel<d>, grid, block, attn_generic_lds_bytes<d>(L, true), stream, qkv, dO, ld, D, L, H, mask, out, ldo, 1, total, drop); \
            else hipLaunchKernelGGL(attn_generic_fwd_kernel<d>, grid, block, attn_generic_lds_bytes<d>(L, false), stream, qkv, ld, D, L, H, mask, out, ldo, 1, total, drop); } break;
        switch (dh) {
            UU3D_ATTNG_CASE(2) UU3D_ATTNG_CASE(8) UU3D_ATTNG_CASE(12) UU3D_ATTNG_CASE(16) UU3D_ATTNG_CASE(24) UU3D_ATTNG_CASE(32) UU3D_ATTNG_CASE(64)
            default: return UU3D_ERR_UNSUPPORTED;
        }
#undef UU3D_ATTNG_CASE
        return hip_status();
    }
    if (dh == 4) {
        const int pack = std::max(1, 128 / L);                         // (sequence, head) pairs per workgroup
        const dim3 grid((total + pack - 1) / pack);
        const size_t lds = attn_generic_lds_bytes<4>(L, backward) * pack;
        if (lds > (size_t)160 * 1024) return UU3D_ERR_UNSUPPORTED;
        if (backward) allow_lds<attn_generic_bwd_kernel<4>>(160 * 1024);      // P and dS of L >= 83 tokens pass the 64 KiB default
        if (backward && L == 17 && mask == nullptr && !drop.on() && !bwd_generic)     // the spatial stack's shape: unrolled, rows in registers
            hipLaunchKernelGGL(attn_small_bwd_kernel<17>, grid, block, attn_small_bwd_lds_bytes<17>() * pack, stream, qkv, dO, ld, D, H, out, ldo, pack, total);
        else if (backward) hipLaunchKernelGGL(attn_generic_bwd_kernel<4>, grid, block, lds, stream, qkv, dO, ld, D, L, H, mask, out, ldo, pack, total, drop);
        else hipLaunchKernelGGL(attn_generic_fwd_kernel<4>, grid, block, lds, stream, qkv, ld, D, L, H, mask, out, ldo, pack, total, drop);
    } else {
        const dim3 grid(total);
        const size_t lds = attn_generic_lds_bytes<48>(L, backward);
        if (backward && L <= 128 && !drop.on() && !bwd_generic) {
            // MFMA backward, tiles in registers (attn_bwd_mfma_kernel); dqkv has the layout (and leading dimension) of qkv
            const int NT = (L + 15) / 16;
            const size_t l2 = attn_bwd_mfma_lds_bytes<48>(NT);
#define UU3D_ATTNB_CASE(nt) case nt: { allow_lds<attn_bwd_mfma_kernel<nt, 48>>(attn_bwd_mfma_lds_bytes<48>(nt)); \
            hipLaunchKernelGGL((attn_bwd_mfma_kernel<nt, 48>), grid, dim3(64 * nt), l2, stream, qkv, dO, ld, D, L, H, mask, out, ldo); } break;
            switch (NT) {
                UU3D_ATTNB_CASE(1) UU3D_ATTNB_CASE(2) UU3D_ATTNB_CASE(3) UU3D_ATTNB_CASE(4)
                UU3D_ATTNB_CASE(5) UU3D_ATTNB_CASE(6) UU3D_ATTNB_CASE(7) UU3D_ATTNB_CASE(8)
            }
#undef UU3D_ATTNB_CASE
        } else if (backward) {
            allow_lds<attn_generic_bwd_kernel<48>>(160 * 1024);
            hipLaunchKernelGGL(attn_generic_bwd_kernel<48>, grid, block, lds, stream, qkv, dO, ld, D, L, H, mask, out, ldo, 1, total, drop);
        } else {
            allow_lds<attn_generic_fwd_kernel<48>>(160 * 1024);
            hipLaunchKernelGGL(attn_generic_fwd_kernel<48>, grid, block, lds, stream, qkv, ld, D, L, H, mask, out, ldo, 1, total, drop);
        }
    }
    return hip_status();
}

// Exact-f32 attention over 1 .. ATTN_LONG_MAX_L tokens, head dim 48, without attention Dropout (uu3d_attn_long.h): the training step's
// layers of more than 128 tokens.  Forward: O (row stride ldo) and the row statistics stats[B][H][L] = {max, sum}.  Backward: dQ, dK, dV
// into dqkv in the layout and row stride ld of qkv, from O and dO (both row stride ldo) and the forward's statistics.
inline bool attn_long_shape_ok(int D, int B, int L, int H) { return B >= 1 && H >= 1 && L >= 1 && L <= ATTN_LONG_MAX_L && D == 48 * H; }
// one workgroup per (sequence, head) and ATTN_LONG_WAVES query (backward: key) tiles: the grid of all three kernels and of the inference forward
inline dim3 attn_long_grid(int B, int L, int H) { return dim3(B * H, (L + 16 * ATTN_LONG_WAVES - 1) / (16 * ATTN_LONG_WAVES)); }
inline int launch_attn_long(bool backward, const float* qkv, const float* O, const float* dO, const float2* stats, int ld, int D, int B, int L,
                            int H, const uint8_t* mask, float* out, float2* stats_out, int ldo, hipStream_t stream) {
    if (!attn_long_shape_ok(D, B, L, H)) return UU3D_ERR_UNSUPPORTED;
    const dim3 grid = attn_long_grid(B, L, H), block(64 * ATTN_LONG_WAVES);
    if (!backward) {
        hipLaunchKernelGGL(attn_long_fwd_kernel<48>, grid, block, 0, stream, qkv, ld, D, L, H, mask, out, ldo, stats_out);
    } else {
        hipLaunchKernelGGL(attn_long_dq_kernel<48>, grid, block, 0, stream, qkv, O, dO, stats, ld, D, L, H, mask, out, ldo);
        hipLaunchKernelGGL(attn_long_dkv_kernel<48>, grid, block, 0, stream, qkv, O, dO, stats, ld, D, L, H, mask, out, ldo);
    }
    return hip_status();
}
// The same forward without the statistics (attn_long_fwd_kernel<48, false>: the same bits in O): the inference forward's exact-f32 attention
// above 128 tokens (launch_attn_infer below) and uu3d_op_attn_long_infer.  Launches only; the caller reads the launch error.
inline int launch_attn_long_infer(const float* qkv, int ld, int D, int B, int L, int H, const uint8_t* mask, float* out, int ldo, hipStream_t stream) {
    if (!attn_long_shape_ok(D, B, L, H)) return UU3D_ERR_UNSUPPORTED;
    hipLaunchKernelGGL((attn_long_fwd_kernel<48, false>), attn_long_grid(B, L, H), dim3(64 * ATTN_LONG_WAVES), 0, stream, qkv, ld, D, L, H, mask, out, ldo,
                       attn_long::NoStats{});
    return UU3D_OK;
}

// ---- forward: row-panel GEMM, fused MLP, few-row GEMM.  The forward's Launcher (uu3d_forward.inc) and the operator ABI (uu3d_ops.hip) launch
// through these, so that an operator runs the instantiation the forward runs. ----
// chunk counts the 8-wave row-panel kernel (uu3d_gemm_panel8.h) is instantiated for      (9: QKV at 284 row tiles = batch 512, four column ranges)
inline constexpr bool panel8_has(int cpw) { return cpw == 4 || cpw == 6 || cpw == 8 || cpw == 9 || cpw == 12; }
// (row tiles x S column ranges) work items, dealt to the 8 XCDs in contiguous blocks (gemm_h3_panel_kernel)
inline dim3 panel_grid(int mt, int S) { return dim3(8 * S, ((mt * S + 7) / 8 + S - 1) / S); }
// Returns false (nothing launched) when the 8-wave kernel has no instantiation for cpw chunks per workgroup.
template <class EP>
bool launch_panel8(hipStream_t stream, const _Float16* Af, const _Float16* Bf, const float* colv, int M, int mt, int S, int cpw, const EP& ep) {
    const dim3 grid = panel_grid(mt, S);
#define UU3D_P8_LAUNCH(CPW) { allow_lds<gemm_h3_panel8_kernel<EP, CPW, 3>>(P8_LDS_TOTAL); \
        hipLaunchKernelGGL((gemm_h3_panel8_kernel<EP, CPW, 3>), grid, dim3(512), P8_LDS_TOTAL, stream, Af, Bf, colv, M, mt, S, ep); return true; }
    switch (cpw) {
        case 4: UU3D_P8_LAUNCH(4)
        case 6: UU3D_P8_LAUNCH(6)
        case 8: UU3D_P8_LAUNCH(8)
        case 9: UU3D_P8_LAUNCH(9)
        case 12: UU3D_P8_LAUNCH(12)
        default: return false;
    }
#undef UU3D_P8_LAUNCH
}
// the 4-wave kernel; CPW != 0: the chunk loop unrolled for that many chunks per workgroup
template <class EP, int CPW = 0>
void launch_panel4(hipStream_t stream, const _Float16* Af, const _Float16* Bf, const float* colv, int M, int mt, int S, int cpw, const EP& ep) {
    allow_lds<gemm_h3_panel_kernel<24, EP, CPW>>(PANEL_LDS_TOTAL);
    hipLaunchKernelGGL((gemm_h3_panel_kernel<24, EP, CPW>), panel_grid(mt, S), dim3(256), PANEL_LDS_TOTAL, stream, Af, Bf, colv, M, mt, S, cpw, ep);
}
// x[M][384] += A B + colv on the 4-wave kernel (N = 384, 12 chunks): S = 3 / 2 / 1 column ranges per row tile run the forms with the chunk loop
// unrolled (CPW = 4 / 6 / 12: uu3d_gemm_panel.h says why an epilogue that loads needs them); any other divisor of 12 the runtime loop
inline void launch_panel4_residual(hipStream_t stream, const _Float16* Af, const _Float16* Bf, const float* colv, int M, int mt, int S, const PanelEpBiasResidual& ep) {
    if (S == 3) launch_panel4<PanelEpBiasResidual, 4>(stream, Af, Bf, colv, M, mt, S, 4, ep);
    else if (S == 2) launch_panel4<PanelEpBiasResidual, 6>(stream, Af, Bf, colv, M, mt, S, 6, ep);
    else if (S == 1) launch_panel4<PanelEpBiasResidual, 12>(stream, Af, Bf, colv, M, mt, S, 12, ep);
    else launch_panel4<PanelEpBiasResidual>(stream, Af, Bf, colv, M, mt, S, 12 / S, ep);
}
// vit.MLP of a temporal block in one launch (uu3d_mlp_fused.h): the fc2 partial sums of the MLPF_SLICES hidden slices -> mslab[slice][M][384]
inline void launch_mlp_fused(hipStream_t stream, const _Float16* Af, const _Float16* W1f, const _Float16* W2f, const float* b1, float* mslab, int M) {
    const int mt = (M + 127) / 128;
    allow_lds<mlp_fused_h3_kernel<>>(PANEL_LDS_TOTAL);
    hipLaunchKernelGGL(mlp_fused_h3_kernel<>, panel_grid(mt, MLPF_SLICES), dim3(256), PANEL_LDS_TOTAL, stream, Af, W1f, W2f, b1, mslab, M, mt);
}
// Few rows (uu3d_gemm_wt.h): one workgroup per 32 x 32 tile, the contraction split over its waves.  Bh / Bl: the operand's planes [N][Kp].
// Returns false (nothing launched) when the contraction is longer than one batch of loads per wave holds (K > 768).
template <class AL, class EP>
bool launch_gemm_wt(hipStream_t stream, const AL& al, const _Float16* Bh, const _Float16* Bl, int M, int N, int K, const EP& ep) {
    const int Kp = ru(K, 32), slices = Kp / 16;
    const int mt = (M + 31) / 32, nt = (N + 31) / 32;
    if (slices > 6 * WT_MAX_WAVES) return false;             // K <= 768: one batch of loads per wave
    const int kw = (slices + 5) / 6;
    hipLaunchKernelGGL((gemm_h3_wt_kernel<AL, EP, 6>), dim3(mt * nt), dim3(64 * kw), gemm_wt_lds_bytes(kw), stream, al, Bh, Bl, M, N, Kp, nt, ep);
    return true;
}

// ---- forward: the tiled GEMMs (uu3d_gemm.h, uu3d_gemm_h3.h).  Tile shape, DEEP form and split are decided HERE and nowhere else: the forward's
// Launcher::gemm / gemm_g and the operator ABI (uu3d_op_tiled_dense) both launch through launch_fwd_gemm / launch_fwd_gemm_g. ----
template <int BM, int BN, class AL, class EP>
void launch_gemm_f32_tile(hipStream_t stream, const AL& al, const float* Bt, int M, int N, int Kp, int slices, int kt_per_split, const EP& ep) {
    auto kern = gemm_f32_kernel<BM, BN, AL, EP>;
    constexpr size_t lds = gemm_lds_bytes(BM, BN);
    allow_lds<gemm_f32_kernel<BM, BN, AL, EP>>(lds);
    const int mt = (M + BM - 1) / BM, nt = (N + BN - 1) / BN;
    const int grid = ru(mt, 8) * nt;
    hipLaunchKernelGGL(kern, dim3(grid, slices), dim3(256), lds, stream, al, Bt, M, N, Kp, mt, nt, kt_per_split, ep);
}
template <int TM, int TN, class AL, class EP>
void launch_gemm_h3_tile(hipStream_t stream, const AL& al, const _Float16* Bh, const _Float16* Bl, int M, int N, int Kp, int slices, int kt_per_split, const EP& ep) {
    auto kern = gemm_h3_kernel<TM, TN, AL, EP>;
    auto kern_deep = gemm_h3_kernel<TM, TN, AL, EP, 1>;     // few workgroups per CU: loads three k-tiles ahead (uu3d_gemm_h3.h)
    constexpr size_t lds = gemm_h3_lds_bytes(64 * TM, 64 * TN);
    allow_lds<gemm_h3_kernel<TM, TN, AL, EP>>(lds); allow_lds<gemm_h3_kernel<TM, TN, AL, EP, 1>>(lds);
    const int mt = (M + 64 * TM - 1) / (64 * TM), nt = (N + 64 * TN - 1) / (64 * TN);
    const int grid = ru(mt, 8) * nt;
    if (gemm_h3_deep(grid * slices)) hipLaunchKernelGGL(kern_deep, dim3(grid, slices), dim3(256), lds, stream, al, Bh, Bl, M, N, Kp, mt, nt, kt_per_split, ep);
    else hipLaunchKernelGGL(kern, dim3(grid, slices), dim3(256), lds, stream, al, Bh, Bl, M, N, Kp, mt, nt, kt_per_split, ep);
}
template <int TM, int TN, class GL, class EP>
void launch_gemm_h3g_tile(hipStream_t stream, const GL& gl, const _Float16* Bh, const _Float16* Bl, int M, int N, int Kp, int slices, int kt_per_split, const EP& ep) {
    auto kern = gemm_h3g_kernel<TM, TN, GL, EP>;
    constexpr size_t lds = gemm_h3g_lds_bytes(64 * TM, 64 * TN);
    allow_lds<gemm_h3g_kernel<TM, TN, GL, EP>>(lds);
    const int mt = (M + 64 * TM - 1) / (64 * TM), nt = (N + 64 * TN - 1) / (64 * TN);
    const int grid = ru(mt, 8) * nt;
    hipLaunchKernelGGL(kern, dim3(grid, slices), dim3(256), lds, stream, gl, Bh, Bl, M, N, Kp, mt, nt, kt_per_split, ep);
}
template <class EP>
void launch_splitk_reduce(hipStream_t stream, const float* slab, int slices, int M, int N, const EP& ep) {
    const int ldslab = ru(N, 4);
    hipLaunchKernelGGL(splitk_reduce_kernel<EP>, dim3((M * N + 255) / 256), dim3(256), 0, stream, slab, slices, (size_t)M * ldslab, M, N, ldslab, ep);
}
// C[M][N] = A-op[M][K] W with the A operand read by a loader of uu3d_gemm.h (f32 rows; the f16x3 kernel splits them while it stages them).
//   precision f16x3: gemm_h3_kernel on the operand's planes Bh / Bl;  f32: gemm_f32_kernel on Bt.  All three [Np][Kp], Kp = round_up(K, 32).
//   64 x 64 tiles (4 workgroups per CU) measured fastest on every shape of the model but the ones named below (tools/gemm_bench.hip).
//   Problems with too few tiles to fill the chip are split along K into slabs and combined deterministically (splitk_reduce_kernel):
//   splitk_rule with the forward's exception, aiming for `target` workgroups, the slab holding slab_floats floats.
// Launches only; the caller reads the launch error.
template <class AL, class EP>
void launch_fwd_gemm(hipStream_t stream, const AL& al, const float* Bt, const _Float16* Bh, const _Float16* Bl, int M, int N, int K, const EP& ep,
                     float* slab, size_t slab_floats, int target, int precision) {
    const int Kp = ru(K, 32), KT = Kp / 32;
    const int tiles = ((M + 63) / 64) * ((N + 63) / 64);
    const auto [slices, kps] = splitk_rule(M, N, KT, target, slab_floats, true);
    const int ldslab = ru(N, 4);
    if (precision == UU3D_PREC_F16X3) {
        if (slices == 1) {
            // measured (tools/gemm_bench): 64x128 is the fastest f16x3 tile on every shape of the model
            if (N % 128 == 0 && tiles >= 512) launch_gemm_h3_tile<1, 2>(stream, al, Bh, Bl, M, N, Kp, 1, KT, ep);
            else launch_gemm_h3_tile<1, 1>(stream, al, Bh, Bl, M, N, Kp, 1, KT, ep);
        } else {
            EpSlab es{slab, ldslab, (size_t)M * ldslab};
            launch_gemm_h3_tile<1, 1>(stream, al, Bh, Bl, M, N, Kp, slices, kps, es);
            launch_splitk_reduce(stream, slab, slices, M, N, ep);
        }
    } else if (slices == 1) {
        // measured (tools/gemm_bench): 64x128 beats 64x64 by ~8 % on the N = 384 GEMMs, loses elsewhere
        if (N % 128 == 0 && N <= 512 && tiles >= 512) launch_gemm_f32_tile<64, 128>(stream, al, Bt, M, N, Kp, 1, KT, ep);
        else launch_gemm_f32_tile<64, 64>(stream, al, Bt, M, N, Kp, 1, KT, ep);
    } else {
        EpSlab es{slab, ldslab, (size_t)M * ldslab};
        launch_gemm_f32_tile<64, 64>(stream, al, Bt, M, N, Kp, slices, kps, es);
        launch_splitk_reduce(stream, slab, slices, M, N, ep);
    }
}
// The f16x3 GEMM whose A operand already is a pair of f16 planes (written by ln_split / attention / the ReLU epilogue / the spatial stack):
// the LDS-DMA kernel gemm_h3g_kernel, K % 32 == 0 (the caller checks).  Same split-K policy as launch_fwd_gemm.
template <class GL, class EP>
void launch_fwd_gemm_g(hipStream_t stream, const GL& gl, const _Float16* Bh, const _Float16* Bl, int M, int N, int K, const EP& ep,
                       float* slab, size_t slab_floats, int target) {
    const int KT = K / 32;
    const int tiles = ((M + 63) / 64) * ((N + 63) / 64);
    const auto [slices, kps] = splitk_rule(M, N, KT, target, slab_floats, true);
    const int ldslab = ru(N, 4);
    if (slices == 1) {
        // measured (tools/gemm_bench, M = 4544 / 1472 rows): 64x128 is the fastest LDS-DMA tile down to ~200 tiles
        if (N % 128 == 0 && tiles >= 256) launch_gemm_h3g_tile<1, 2>(stream, gl, Bh, Bl, M, N, K, 1, KT, ep);
        else launch_gemm_h3g_tile<1, 1>(stream, gl, Bh, Bl, M, N, K, 1, KT, ep);
    } else {
        EpSlab es{slab, ldslab, (size_t)M * ldslab};
        // split K with many tiles (strided block 1's convolution: 276 tiles x 3 slices of K = 768): 64 x 128 tiles move a
        // quarter less through L2 -> LDS than 64 x 64 (41.6 -> 36.5 us); with few tiles the 64 x 64 grid fills more CUs
        if (N % 128 == 0 && tiles >= 200) launch_gemm_h3g_tile<1, 2>(stream, gl, Bh, Bl, M, N, K, slices, kps, es);
        else launch_gemm_h3g_tile<1, 1>(stream, gl, Bh, Bl, M, N, K, slices, kps, es);
        launch_splitk_reduce(stream, slab, slices, M, N, ep);
    }
}

// ---- forward: temporal self-attention, head dim 48 (uu3d_attn.h, uu3d_attn_h3.h).  Which kernel a launch takes is decided HERE and nowhere else. ----
constexpr int kAttnDH = 48;
enum AttnKernel : int { ATTN_AUTO = 0, ATTN_F32_WG = 1, ATTN_HEAD_WAVE = 2, ATTN_H3 = 3,         // = UU3D_ATTN_* of include/uu3d_ops.h
                        ATTN_F32_LONG = 4 };     // internal (no UU3D_ATTN_* value, never forced): attn_long_fwd_kernel<48, false>, a CALL at precision f32 above 128 tokens
// what the choice depends on besides the shape: the call's precision, UU3D_ATTN_F32 / UU3D_ATTN_WG (uu3d_switches.h), and a kernel forced by the caller
struct AttnRule { int precision = UU3D_PREC_F16X3; bool attn_f32 = false, attn_wg = false; int forced = ATTN_AUTO; };
// sequences served by attn_h3_kernel (f16x3 products, online softmax; q / k / v as f16 planes from the QKV epilogue): everything
// the exact-f32 kernels cannot hold (> 128 tokens) and, measured faster, 49-128 tokens as well
// (shorter sequences, h36m_81's 41 tokens: the split epilogue of the QKV projection costs more than the attention gains -- 242.1 k
// sequences/s with the exact-f32 kernels there against 240.2 k)
inline bool attn_is_h3(const AttnRule& r, int L, bool planes_out) { return planes_out && L <= ATTN_H3_MAX_L && (L > 128 || (L > 48 && !r.attn_f32)); }
inline bool attn_h3_any(const AttnRule& r, int L) { return r.precision == UU3D_PREC_F16X3 && L <= ATTN_H3_MAX_L && !r.attn_f32; }
// The kernel family of one launch; ATTN_AUTO (= 0) when the rule, or the forced kernel, has none for the shape.
//   planes_out: the context rows leave as f16 planes;  qfrag: q | k | v arrive in the temporal chain's fragment order
inline int attn_choose(const AttnRule& r, int L, int H, bool planes_out, bool qfrag) {
    const int NT = (L + 15) / 16;
    const bool hw_fits = H % 4 == 0 && NT >= 4 && NT <= 5;
    switch (r.forced) {
        case ATTN_H3: return planes_out && L <= ATTN_H3_MAX_L ? ATTN_H3 : ATTN_AUTO;
        case ATTN_HEAD_WAVE: return !qfrag && hw_fits ? ATTN_HEAD_WAVE : ATTN_AUTO;
        case ATTN_F32_WG: return !qfrag && NT <= 8 ? ATTN_F32_WG : ATTN_AUTO;
        default: break;
    }
    // (the chain's fragment-ordered planes cost no split epilogue: attn_h3_kernel below 49 tokens too)
    if (attn_is_h3(r, L, planes_out) || (qfrag && attn_h3_any(r, L))) return ATTN_H3;
    if (qfrag) return ATTN_AUTO;
    // a call at precision f32 (UU3D_SCHEDULE_EXACT_F32; no planes there) above the register-resident kernels' 128 tokens: the tiled exact-f32
    // forward of the training step without its statistics (uu3d_attn_long.h).  A rule at precision f16x3 has no exact-f32 kernel up there.
    if (r.precision == UU3D_PREC_F32 && !planes_out && L > 128 && L <= ATTN_LONG_MAX_L) return ATTN_F32_LONG;
    // one wave per (sequence, head), four heads per workgroup (attn_head_wave_kernel): whenever the heads come in fours and the
    // K / V tiles of four heads fit the LDS; UU3D_ATTN_WG=1 keeps the workgroup-per-item kernel
    // NT <= 3: more, smaller workgroups hide latency better (measured)
    if (!r.attn_wg && hw_fits) return ATTN_HEAD_WAVE;
    return NT <= 8 ? ATTN_F32_WG : ATTN_AUTO;
}
// the kernel class a profile records for a family (every exact-f32 kernel is "attn_f32")
inline const char* attn_class_name(int kernel) { return kernel == ATTN_H3 ? "attn_h3" : "attn_f32"; }

// One attention launch over B sequences of L tokens, H heads of 48 channels (D = 48 H).
//   attn_h3_kernel: qkv = the hi plane [B L][3 D] halfs with the lo plane directly behind it, or (qfrag) the fragment-ordered buffer; the
//   exact-f32 kernels: qkv = [B L][3 D] floats.
//   split_lo_off != 0: the context rows go out as f16 planes (hi at out, lo split_lo_off halfs further); frag: in the row-panel GEMM's
//   A-fragment order instead of row-major planes (split_lo_off != 0 only)
// Returns UU3D_OK after the launch (the caller reads the launch error), UU3D_ERR_UNSUPPORTED without one; *klass = the kernel class name.
inline int launch_attn_infer(hipStream_t stream, const float* qkv, int D, int B, int L, int H, const uint8_t* mask, float* out, size_t split_lo_off,
                             bool frag, bool qfrag, const AttnRule& rule, const char** klass = nullptr) {
    constexpr int kDH = kAttnDH;
    const int kernel = attn_choose(rule, L, H, split_lo_off != 0, qfrag);
    if (klass) *klass = attn_class_name(kernel);
    if (kernel == ATTN_AUTO) return UU3D_ERR_UNSUPPORTED;
    if (kernel == ATTN_F32_LONG) return launch_attn_long_infer(qkv, 3 * D, D, B, L, H, mask, out, D, stream);     // qkv = [B L][3 D] floats, out = [B L][D] floats
    const int NT = (L + 15) / 16;
    const int items = B * H;
    const dim3 grid(items);
    if (kernel == ATTN_H3) {                                       // qkv = hi plane [B L][3 D] halfs, lo plane behind it
        const int nt = (L + 31) / 32;
        const size_t lds = attn_h3_lds_bytes(L, kDH);
        _Float16* oh = reinterpret_cast<_Float16*>(out);
        const _Float16* qh = reinterpret_cast<const _Float16*>(qkv); const _Float16* ql = qh + (size_t)B * L * 3 * D;
#define UU3D_ATTN_H3_LAUNCH(MW, WPE, MASKED, waves) { allow_lds<attn_h3_kernel<kDH, MW, WPE, MASKED>>(attn_h3_lds_bytes(ATTN_H3_MAX_L, kDH)); \
            hipLaunchKernelGGL((attn_h3_kernel<kDH, MW, WPE, MASKED>), grid, dim3(64 * (waves)), lds, stream, qh, ql, 3 * D, D, L, H, mask, oh, frag ? (size_t)512 : split_lo_off, D, frag ? 1 : 0, qfrag ? 1 : 0); }
        // 4 .. 12 key tiles (dense-351: 11): one wave per query tile, three per SIMD (dense-351: 35.4 vs 36.8 us with 8 waves x 2 tiles)
        if (nt <= 3) { if (mask) UU3D_ATTN_H3_LAUNCH(3, 3, true, nt) else UU3D_ATTN_H3_LAUNCH(3, 3, false, nt) }
        else if (nt <= 12) { if (mask) UU3D_ATTN_H3_LAUNCH(12, 3, true, nt) else UU3D_ATTN_H3_LAUNCH(12, 3, false, nt) }
        else { if (mask) UU3D_ATTN_H3_LAUNCH(8, 2, true, std::min(nt, 8)) else UU3D_ATTN_H3_LAUNCH(8, 2, false, std::min(nt, 8)) }
#undef UU3D_ATTN_H3_LAUNCH
        return UU3D_OK;
    }
    if (kernel == ATTN_HEAD_WAVE) {
        const dim3 hgrid((items + 3) / 4);
#define UU3D_ATTN_HW(nt) case nt: { \
        constexpr size_t lds = attn_head_wave_lds_bytes<nt, kDH>(); \
        if (split_lo_off) { allow_lds<attn_head_wave_kernel<nt, kDH, true>>(lds); \
            hipLaunchKernelGGL((attn_head_wave_kernel<nt, kDH, true>), hgrid, dim3(256), lds, stream, qkv, 3 * D, D, L, H, mask, out, D, frag ? (size_t)512 : split_lo_off, items); } \
        else { allow_lds<attn_head_wave_kernel<nt, kDH, false>>(lds); \
            hipLaunchKernelGGL((attn_head_wave_kernel<nt, kDH, false>), hgrid, dim3(256), lds, stream, qkv, 3 * D, D, L, H, mask, out, D, (size_t)0, items); } \
        } break;
        switch (NT) { UU3D_ATTN_HW(4) UU3D_ATTN_HW(5) default: break; }
#undef UU3D_ATTN_HW
        return UU3D_OK;
    }
#define UU3D_ATTN_CASE(nt) case nt: \
    if (split_lo_off) hipLaunchKernelGGL((attn_f32_kernel<nt, kDH, true>), grid, dim3(64 * nt), 0, stream, qkv, 3 * D, D, L, H, mask, out, D, frag ? (size_t)512 : split_lo_off); \
    else hipLaunchKernelGGL((attn_f32_kernel<nt, kDH, false>), grid, dim3(64 * nt), 0, stream, qkv, 3 * D, D, L, H, mask, out, D, (size_t)0); \
    break;
    switch (NT) {
        UU3D_ATTN_CASE(1) UU3D_ATTN_CASE(2) UU3D_ATTN_CASE(3) UU3D_ATTN_CASE(4)
        UU3D_ATTN_CASE(5) UU3D_ATTN_CASE(6) UU3D_ATTN_CASE(7) UU3D_ATTN_CASE(8)
        default: break;
    }
#undef UU3D_ATTN_CASE
    return UU3D_OK;
}

// ---- forward: the temporal chain (uu3d_tchain16.h).  One launch = the stage set `flags` over every 64-row tile of M token rows; the forward's
// Launcher::tchain and the operator ABI (uu3d_op_tchain) both launch through this: grid, block, LDS bytes and the TChainArgs fill exist once. ----
// W / P: the launch's weight stream and parameter table as uu3d_commit_weights packed them.  Returns false (nothing launched) for a stage set the
// kernel is not instantiated for.  Launches only; the caller reads the launch error.  (A template, so that only a translation unit that calls it
// compiles the five kernels.)
template <class Args = TChainArgs>
bool launch_tchain(hipStream_t stream, int flags, int M, const _Float16* W, const float* P, float qscale, const _Float16* Of, float* X, float* XA,
                          const float* pe, int period, _Float16* Q, _Float16* H, unsigned char* scratch) {
    const int mt = (M + 63) / 64;
    Args a{};
    a.M = M; a.m_tiles = mt; a.period = period; a.qscale = qscale;
    a.Of = Of; a.X = X; a.XA = XA; a.pe = pe; a.W = W; a.P = P; a.Q = Q; a.H = H; a.scratch = scratch;
#define UU3D_T16_LAUNCH(F) case F: { allow_lds<tchain16_kernel<F>>(T16_LDS_TOTAL); \
            hipLaunchKernelGGL(tchain16_kernel<F>, dim3(mt), dim3(512), T16_LDS_TOTAL, stream, a); } return true;
    switch (flags) {
        UU3D_T16_LAUNCH(TC_QKV)
        UU3D_T16_LAUNCH(TC_PROJ | TC_MLP | TC_QKV)
        UU3D_T16_LAUNCH(TC_PROJ | TC_MLP | TC_QKV | TC_PE)
        UU3D_T16_LAUNCH(TC_PROJ | TC_MLP)
        UU3D_T16_LAUNCH(TC_PROJ | TC_FC1_PLANES)
        default: return false;
    }
#undef UU3D_T16_LAUNCH
}

}  // namespace uu3d
