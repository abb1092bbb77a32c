// uu3d_pack.h -- host-side packing of a Dense / Conv1D kernel into the operand the tiled GEMMs read: shared by uu3d_commit_weights
// (uu3d_commit.inc) and the operator ABI (uu3d_op_tiled_pack, uu3d_ops.hip), so that an operator's operand is the commit's operand.
#pragma once
#include <cmath>
#include <cstddef>
#include "uu3d_gemm_h3.h"

namespace uu3d {

// Keras Dense kernel (K, N) -> Bt[Np][Kp] at buf + off, Np = round_up(N,128), Kp = round_up(K,32) (the caller zero-fills); row offset n0.
inline void pack_dense_t(float* buf, size_t off, const float* w, int K, int N, int Kp, int n0) {
    for (int k = 0; k < K; ++k)
        for (int n = 0; n < N; ++n) buf[off + (size_t)(n0 + n) * Kp + k] = w[(size_t)k * N + n];
}

// n floats -> the f16 hi / (lo * 2048) planes of the f16x3 kernels (uu3d_gemm_h3.h).  Returns false at the first value of magnitude >= 65504
// (or non-finite): its hi plane would be Inf (include/uu3d.h, RANGE CONTRACT).
inline bool split_operand_planes(const float* x, size_t n, _Float16* hi, _Float16* lo) {
    for (size_t i = 0; i < n; ++i) {
        if (!(std::fabs(x[i]) < 65504.0f)) return false;
        const _Float16 h = h3_hi(x[i]);
        hi[i] = h; lo[i] = (_Float16)((x[i] - (float)h) * H3_SCALE);
    }
    return true;
}

}  // namespace uu3d
