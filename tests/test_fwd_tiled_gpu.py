"""The forward's TILED GEMMs, operator by operator through uu3d_op_tiled_dense (include/uu3d_ops.h), against float64 numpy computed from the
values the kernel is given (planes read as hi + lo / 2048, made on the host with the project's split of f32 draws; weights: the f32 kernel).
The operator launches through launch_fwd_gemm / launch_fwd_gemm_g (csrc/uu3d_launch.h), as the forward's Launcher::gemm / gemm_g do: a
case here runs the instantiation the forward runs, with the forward's tile choice, DEEP choice and split rule.

Instantiations the forward can launch (call sites of csrc/uu3d_forward.inc: spatial_stage, block_head, temporal_blocks, head1, strided_blocks,
head2), and the cases that reach them (names = test ids):
  loader x epilogue pairs, "rows" kernels (Launcher::gemm: gemm_h3_kernel at precision f16x3, gemm_f32_kernel at f32):
      ALoadPlain x EpBias (head1, head2), x EpBiasResidual (proj_res; fc2_res with out2 / pe2), x EpSpatialToTemporal (s2t)
      ALoadLayerNorm x EpBias (ln_qkv), x EpBiasRelu (ln_fc1), x EpBiasSplitQ (ln_qkv, f16x3 only), x EpBiasReluSplit (ln_fc1, f16x3 only)
      ALoadConv3 x EpConvResidual (s*.conv_res)
    gemm_h3_kernel<1, 1, AL, EP, DEEP 1>        every pair: "*-small-*", the row sweep "rows-M*", "k1/k2/k3-*"
    gemm_h3_kernel<1, 1, AL, EP, DEEP 0>        every pair: "*-wide64-*"   (648 workgroups > gemm_deep_wgs = 640, N = 192)
    gemm_h3_kernel<1, 2, AL, EP, DEEP 1>        every pair: "*-t128deep-*" (M = 5441, N = 384: 516 tiles, 264 workgroups)
    gemm_h3_kernel<1, 2, AL, EP, DEEP 0>        every pair: "*-t128-*"     (M = 13825, N = 384: 672 workgroups)
    gemm_h3_kernel<1, 1, AL, EpSlab, DEEP 1>    every loader: "*-split-*", "last1/2/3-*", "K408-*"
    gemm_h3_kernel<1, 1, AL, EpSlab, DEEP 0>    every loader: "*-splitwide-*" (144 x 6 = 864 workgroups; conv: 48 x 18)
    gemm_f32_kernel<64, 64, AL, EP>, <64, 128, AL, EP>, <64, 64, AL, EpSlab>: the same names with "-f32"
  "planes" kernels (Launcher::gemm_g: gemm_h3g_kernel, LDS-DMA, three buffers):
      GLoadPlain x EpBiasResidual (proj_res, fc2_res), x EpSpatialToTemporal (s2t);  GLoadConv3 x EpConvResidual (s*.conv_res)
    gemm_h3g_kernel<1, 1, GL, EP>               "g-*-small-*", "g-k1/k2/k3-*" (fewer k-tiles than the ring holds), "g-rows-M*", "gconv-*"
    gemm_h3g_kernel<1, 2, GL, EP>               "g-*-t128-*" (M = 2689: 43 row tiles, 258 tiles), "gconv-t128"
    gemm_h3g_kernel<1, 1, GL, EpSlab>           "g-*-split-*", "g-last1/2/3", "gconv-C768-*"
    gemm_h3g_kernel<1, 2, GL, EpSlab>           "g-*-split128" (M = 2113, K = 576: 204 tiles, 4 slices of 5, 5, 5, 3), "gconv-split128"
  splitk_reduce_kernel<EP> for every epilogue above (second stream + PE, pe_next, mask + token included): the split cases.
Split rule: test_split_rule holds uu3d_op_tiled_split (the forward's call: exception on) to the restatement below over both sides of every
boundary; every GPU case asserts its (slices, k-tiles per slice) from the restatement, the boundary cases ("rule-*") literal values too.

References: float64; the convolution as a literal ZeroPadding1D + Conv1D('valid', stride) + MaxPool(1, stride) residual with loops over
taps; s2t as m ? acc + bias : token, + pe[row % period].  Every output is NaN-filled with a guard row (and guard columns where the row
stride allows), the slab carries a guard behind its capacity; each case is launched twice and compared bitwise.

Bounds (none taken from what these kernels measure):
  * exact-f32 kernels: 2e-6 max|ref| (test_bwd_ops_gpu.py's measure for the same MFMA arithmetic); split and unsplit of a case are both
    held to it (not compared bitwise: the order of summation differs);
  * f16x3, K <= 384, unit-scale outputs (max|ref| < 8 asserted): 2e-5 (test_panel_op_gpu.py's bound for one f16x3 layer);
  * f16x3, K > 384: 2e-5 + 2 x the deviation, for that case, of a float32 restatement (f32 operands, f32 accumulation in k order) from
    float64 -- twice, because the kernel rounds in the slab sum as well as in the accumulator; every allowance asserted <= 1e-4.
    CPU-computed deviations, largest per K: K = 408: 3.1e-6, 416: 2.8e-6, 512: 4.6e-6, 544: 4.8e-6, 576: 5.0e-6, 672: 3.9e-6,
    768: 5.3e-6, 2304: 7.0e-6  (allowances 2.6e-5 .. 3.4e-5);
  * plane outputs (EpBiasReluSplit, EpBiasSplitQ): + 2^-20, the representation step derived in test_fwd_ops_gpu.py.
Measured on an MI355X (largest max-abs error of a kernel form, with that case's bound): gemm_h3g 64x64 1.3e-6 unsplit / 8.6e-7 split (of 2.0e-5),
64x128 1.7e-6 of 2.0e-5 / 1.0e-6 of 3.0e-5; gemm_h3 64x64 DEEP 1.3e-6 / 8.7e-7 (of 2.0e-5), not DEEP 1.3e-6 of 2.1e-5 / 1.2e-6 of 3.1e-5, 64x128 DEEP
1.5e-6, not DEEP 1.3e-6 (of 2.0e-5); gemm_f32 64x64 5.6e-6 of 1.0e-5 unsplit, 1.8e-6 of 6.6e-6 split, 64x128 2.5e-6 of 1.6e-5.
223 tests, 431 checked launches (200 cases launched twice, the 31 split exact-f32 cases once more unsplit; the 22 rejected calls launch nothing):
7.3 s for the whole file."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

A_F32, A_LN, A_PLANES, A_CONV_F32, A_CONV_PLANES = range(5)
EP_BIAS, EP_RELU_SPLIT, EP_SPLIT_Q, EP_RESIDUAL, _EP_RESIDUAL_LN, EP_BIAS_RELU, EP_CONV, EP_S2T = range(8)
PREC_F32, PREC_H3 = 0, 1
INVALID = 1
EPS = 1e-5
TOL_H3 = 2e-5
TOL_F32_REL = 2e-6
STEP = 2.0 ** -20
CAP = 1e-4
QSCALE = float(np.float32(1.44269504088896341 / np.sqrt(48.0)))
DEEP_WGS = 640                   # gemm_deep_wgs (uu3d_switches.h)
FULL_SLAB = 1536 * 4096          # floats: room for every split here


def ru(v, m):
    return (v + m - 1) // m * m


def split_rule(M, N, KT, target, slab_floats, exception=True):
    """splitk_rule of csrc/uu3d_launch.h, restated."""
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    slices = 1
    if tiles < 384 and KT >= 8 and not (exception and tiles >= 200 and KT <= 16):
        slices = max(1, min(KT // 4, (target + tiles // 2) // tiles))
    kps = (KT + slices - 1) // slices
    slices = (KT + kps - 1) // kps
    if slices > 1 and slices * M * ru(N, 4) > slab_floats:
        slices, kps = 1, KT
    return slices, kps


def kernel_of(c):
    """The instantiation launch_fwd_gemm / launch_fwd_gemm_g takes for a case, restated: (kernel, TM x TN, DEEP, slices, kps)."""
    KT = ru(c.K, 32) // 32
    tiles = ((c.M + 63) // 64) * ((c.N + 63) // 64)
    slices, kps = split_rule(c.M, c.N, KT, c.target, c.slab)
    if c.src in (A_PLANES, A_CONV_PLANES):
        wide = c.N % 128 == 0 and tiles >= (256 if slices == 1 else 200)
        return "gemm_h3g", 128 if wide else 64, None, slices, kps
    if c.prec == PREC_H3:
        wide = slices == 1 and c.N % 128 == 0 and tiles >= 512
        bn = 128 if wide else 64
        grid = ru((c.M + 63) // 64, 8) * ((c.N + bn - 1) // bn)
        return "gemm_h3", bn, int(grid * slices <= DEEP_WGS), slices, kps
    wide = slices == 1 and c.N % 128 == 0 and c.N <= 512 and tiles >= 512
    return "gemm_f32", 128 if wide else 64, None, slices, kps


class Case:
    def __init__(self, name, src, ep, M, N, K, prec=PREC_H3, target=768, slab=FULL_SLAB, conv=None, opt=True, expect=None, period=None, want_kernel=None):
        self.name, self.src, self.ep, self.M, self.N, self.K, self.prec, self.target, self.slab = name, src, ep, M, N, K, prec, target, slab
        self.conv = conv            # (C, stride, pad_left, pad_right, L_out, B)
        self.opt = opt              # the optional part of the epilogue: out2 / pe2, pe_next, mask + token
        self.expect = expect        # literal (slices, k-tiles per slice)
        self.period = period
        self.want_kernel = want_kernel      # literal (kernel, BN, DEEP)
        if conv is not None:
            Cc, s, pl, pr, Lo, B = conv
            # L_in: the last window ends exactly at the padded end, so that with pad_right > 0 the last output row reads a zero tap
            self.L_in = s * (Lo - 1) + 3 - pl - pr
            assert self.L_in >= 1 and M == B * Lo and K == 3 * Cc


# ---- inputs: made once, read-only ----
def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def h3_split(x):
    """The project's split (uu3d_gemm_h3.h): hi = f16(x), 0 below the smallest normal half; lo = f16((x - hi) * 2048)."""
    x = np.asarray(x, np.float32)
    hi = np.where(np.abs(x) < np.float32(6.103515625e-05), np.float32(0), x).astype(np.float16)
    lo = ((x - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return hi, lo


@functools.lru_cache(maxsize=None)
def _a_rows(R, K):
    rng = np.random.default_rng(17 * R + K)
    x = rng.normal(size=(R, K)).astype(np.float32)
    if R > 3:
        x[3] *= 1e-6                                              # the f16 denormal range of the split
    hi, lo = h3_split(x)
    return _ro(x, hi, lo)


@functools.lru_cache(maxsize=None)
def _weights(K, N):
    rng = np.random.default_rng(1000 * K + N)
    w = (rng.normal(size=(K, N)) / np.sqrt(K)).astype(np.float32)    # Keras (in, out), N(0, 1 / K): unit-scale outputs
    bias = (0.1 * rng.normal(size=N)).astype(np.float32)
    return _ro(w, bias)


@functools.lru_cache(maxsize=None)
def _extras(R, N, period):
    rng = np.random.default_rng(5 * R + N + 31 * period)
    # (one spare row behind each: an index formula that is off by one row or one period reads other values, not past the buffer)
    stream = rng.normal(size=(R + 1, N)).astype(np.float32)          # residual stream / the block's input stream
    pe = (0.1 * rng.normal(size=(period + 1, N))).astype(np.float32)
    token = rng.normal(size=N).astype(np.float32)
    return _ro(stream, pe, token)


@functools.lru_cache(maxsize=None)
def _mask(M, period):
    rng = np.random.default_rng(M + period)
    m = (rng.random(M) < 0.5).astype(np.uint8)
    m[:min(period, M)] = 0                                            # the first sequence entirely masked
    if M > period:
        m[period] = 1
    return _ro(m)


@functools.lru_cache(maxsize=None)
def _ln_params(K):
    rng = np.random.default_rng(7 + K)
    return _ro((1.0 + 0.1 * rng.normal(size=K)).astype(np.float32), (0.1 * rng.normal(size=K)).astype(np.float32))


def _period(c):
    return c.period or (c.conv[4] if c.conv else 7)                  # 7 divides no tile height


def _a_values(c):
    """float64 A operand [M][K] as the kernel is given it (after the loader's LayerNorm / gather)."""
    if c.conv is None:
        x, hi, lo = _a_rows(c.M, c.K)
        if c.src == A_PLANES:
            return hi.astype(np.float64) + lo.astype(np.float64) / 2048.0
        if c.src == A_LN:
            g, b = _ln_params(c.K)
            x = x.astype(np.float64)
            mean = x.mean(-1, keepdims=True)
            var = ((x - mean) ** 2).mean(-1, keepdims=True)
            return (x - mean) / np.sqrt(var + EPS) * g.astype(np.float64) + b.astype(np.float64)
        return x.astype(np.float64)
    Cc, s, pl, pr, Lo, B = c.conv
    x, hi, lo = _a_rows(B * c.L_in, Cc)
    h = (hi.astype(np.float64) + lo.astype(np.float64) / 2048.0) if c.src == A_CONV_PLANES else x.astype(np.float64)
    # ZeroPadding1D((pl, pr)) + the 'valid' windows of Conv1D(kernel 3, stride s): tap j of output t is padded row t s + j
    padded = np.zeros((B, pl + c.L_in + pr, Cc))
    padded[:, pl:pl + c.L_in] = h.reshape(B, c.L_in, Cc)
    assert (padded.shape[1] - 3) // s + 1 == Lo
    g = np.zeros((B, Lo, 3, Cc))
    for t in range(Lo):
        for j in range(3):
            g[:, t, j] = padded[:, t * s + j]
    return g.reshape(B * Lo, 3 * Cc)


@functools.lru_cache(maxsize=None)
def _acc_cached(key):
    c = _CASES[key]
    a = _a_values(c)
    w, _ = _weights(c.K, c.N)
    acc = a @ w.astype(np.float64)
    dev = 0.0
    if c.prec == PREC_H3 and c.K > 384:
        # float32 restatement: f32 operands, f32 accumulation in k order
        a32, w32 = a.astype(np.float32), w
        r = np.zeros((c.M, c.N), np.float32)
        for k in range(c.K):
            r += a32[:, k:k + 1] * w32[k:k + 1, :]
        dev = float(np.abs(r.astype(np.float64) - acc).max())
    return _ro(acc), dev


def _want(c):
    """float64 reference of every output: (main [M][N], out2 or None), and the f32-restatement deviation of the case."""
    acc, dev = _acc_cached(c.name)
    _, bias = _weights(c.K, c.N)
    v = acc + bias.astype(np.float64)
    P = _period(c)
    rows = np.arange(c.M)
    if c.ep == EP_BIAS:
        return v, None, dev
    if c.ep == EP_BIAS_RELU or c.ep == EP_RELU_SPLIT:
        return np.maximum(v, 0.0), None, dev
    if c.ep == EP_SPLIT_Q:
        v = v.copy(); v[:, :c.N // 3] *= QSCALE
        return v, None, dev
    if c.ep == EP_RESIDUAL:
        stream, pe, _ = _extras(c.M, c.N, P)
        y = stream[:c.M].astype(np.float64) + v
        return y, (y + pe.astype(np.float64)[rows % P] if c.opt else None), dev
    if c.ep == EP_S2T:
        _, pe, token = _extras(c.M, c.N, P)
        t = v
        if c.opt:
            t = np.where(_mask(c.M, P)[:, None] != 0, v, token.astype(np.float64)[None, :])
        return t + pe.astype(np.float64)[rows % P], None, dev
    Cc, s, pl, pr, Lo, B = c.conv
    xin, pe, _ = _extras(B * c.L_in, c.N, Lo)
    lo = 1 if (s > 1 and pl == 0) else 0
    ident = np.zeros((B, Lo, c.N))
    x3 = xin[:B * c.L_in].astype(np.float64).reshape(B, c.L_in, c.N)
    for t in range(Lo):
        ident[:, t] = x3[:, t * s + lo]                              # MaxPool1D(1, stride) of the trimmed input stream
    y = ident.reshape(c.M, c.N) + v
    if c.opt:
        y = y + np.tile(pe[:Lo].astype(np.float64), (B, 1))
    return y, None, dev


# ---- device side ----
@pytest.fixture(scope="module")
def lib():
    from uplift_upsample_3dhpe_amd import _capi
    assert _capi.UU3D_ERR_INVALID_ARGUMENT == INVALID and (_capi.UU3D_PREC_F32, _capi.UU3D_PREC_F16X3) == (PREC_F32, PREC_H3)
    assert (_capi.UU3D_EP_BIAS_RELU, _capi.UU3D_EP_CONV_RESIDUAL, _capi.UU3D_EP_S2T) == (EP_BIAS_RELU, EP_CONV, EP_S2T)
    return _capi.load_library()


def _p(t):
    return None if t is None else t.data_ptr()


def _nan(n, dtype=None):
    return torch.full((n,), float("nan"), dtype=dtype or torch.float32, device="cuda")


_dev_cache = {}


def _dev(key, make):
    if key not in _dev_cache:
        _dev_cache[key] = torch.from_numpy(np.array(make())).cuda()                  # (a copy: the cached inputs are read-only)
    return _dev_cache[key]


def _operand(lib, K, N):
    def make():
        w, _ = _weights(K, N)
        op = torch.empty(int(lib.uu3d_op_tiled_operand_bytes(N, K)), dtype=torch.uint8, device="cuda")
        assert op.numel() == 8 * ru(N, 128) * ru(K, 32)
        assert lib.uu3d_op_tiled_pack(np.ascontiguousarray(w).ctypes.data_as(C.c_void_p), K, N, C.c_void_p(op.data_ptr()), None) == 0
        return op
    key = ("op", K, N)
    if key not in _dev_cache:
        _dev_cache[key] = make()
    return _dev_cache[key]


GUARD = 64


class Run:
    """One call of uu3d_op_tiled_dense on NaN-filled, guarded buffers."""

    def __init__(self, lib, c, slab=None, **override):
        from uplift_upsample_3dhpe_amd._capi import Uu3dTiledDenseArgs
        self.c = c
        M, N, K = c.M, c.N, c.K
        P = _period(c)
        a = Uu3dTiledDenseArgs()
        R = M if c.conv is None else c.conv[5] * c.L_in
        Ka = K if c.conv is None else c.conv[0]
        if c.src in (A_PLANES, A_CONV_PLANES):
            a.a_dev = _p(_dev(("ah", R, Ka), lambda: _a_rows(R, Ka)[1])); a.a_lo_dev = _p(_dev(("al", R, Ka), lambda: _a_rows(R, Ka)[2]))
        else:
            xd = _dev(("a", R, Ka), lambda: _a_rows(R, Ka)[0])
            a.a_dev = _p(xd)
            if c.src == A_LN:
                key = ("stats", R, Ka)
                if key not in _dev_cache:
                    st = torch.empty(2 * M, dtype=torch.float32, device="cuda")
                    assert lib.uu3d_op_row_stats(C.c_void_p(xd.data_ptr()), K, K, M, EPS, C.c_void_p(st.data_ptr()), None) == 0
                    _dev_cache[key] = st
                a.ln_stats_dev = _p(_dev_cache[key])
                a.ln_gamma_dev = _p(_dev(("g", K), lambda: _ln_params(K)[0])); a.ln_beta_dev = _p(_dev(("b", K), lambda: _ln_params(K)[1]))
        a.operand_dev = _p(_operand(lib, K, N))
        a.bias_dev = _p(_dev(("bias", K, N), lambda: _weights(K, N)[1]))
        self.ldo = N + 3 if c.ep in (EP_BIAS, EP_BIAS_RELU) else N
        self.planes_out = c.ep in (EP_RELU_SPLIT, EP_SPLIT_Q)
        self.out = _nan((2 * M + 1) * N, torch.float16) if self.planes_out else _nan((M + 1) * self.ldo)
        a.out_dev = _p(self.out)
        self.out2 = None
        Rx = M if c.conv is None else R
        if c.ep == EP_RESIDUAL:
            self.out[:M * N] = _dev(("stream", M, N, P), lambda: _extras(M, N, P)[0])[:M].reshape(-1)     # in place, on a copy of the stream
            if c.opt:
                self.out2 = _nan((M + 1) * N)
                a.out2_dev = _p(self.out2)
        if c.ep == EP_CONV:
            a.xin_dev = _p(_dev(("stream", Rx, N, P), lambda: _extras(Rx, N, P)[0]))
        if (c.ep in (EP_RESIDUAL, EP_CONV) and c.opt) or c.ep == EP_S2T:
            a.pe_dev = _p(_dev(("pe", Rx, N, P), lambda: _extras(Rx, N, P)[1]))
        if c.ep == EP_S2T and c.opt:
            a.mask_dev = _p(_dev(("mask", M, P), lambda: _mask(M, P))); a.token_dev = _p(_dev(("token", M, N, P), lambda: _extras(M, N, P)[2]))
        self.slab_floats = c.slab if slab is None else slab
        self.slab = _nan(self.slab_floats + GUARD)
        a.slab_dev = _p(self.slab); a.slab_floats = self.slab_floats
        a.a_source, a.epilogue, a.precision, a.splitk_target = c.src, c.ep, c.prec, c.target
        a.M, a.N, a.K, a.lda, a.ldo = M, N, K, Ka, self.ldo
        if c.conv is not None:
            a.conv_C, a.conv_stride, a.conv_pad_left, a.conv_L_out, a.conv_L_in = c.conv[0], c.conv[1], c.conv[2], c.conv[4], c.L_in
        a.period, a.qscale = P, QSCALE
        for k, v in override.items():
            setattr(a, k, v)
        self.args = a
        self.status = lib.uu3d_op_tiled_dense(C.byref(a), None)
        torch.cuda.synchronize()

    def check_guards(self):
        c = self.c
        M, N = c.M, c.N
        assert torch.isnan(self.slab[self.slab_floats:]).all(), "the slab was written past its capacity"
        if self.planes_out:
            assert torch.isnan(self.out[2 * M * N:]).all(), "the planes pass 2 M N halfs"
            return
        o = self.out.reshape(M + 1, self.ldo)
        assert torch.isnan(o[M]).all(), "a row past M was written"
        assert torch.isnan(o[:, N:]).all(), "columns past N were written"
        if self.out2 is not None:
            assert torch.isnan(self.out2[M * N:]).all(), "a row of out2 past M was written"

    def values(self):
        c = self.c
        M, N = c.M, c.N
        if self.planes_out:
            o = self.out[:2 * M * N].cpu().numpy().astype(np.float64).reshape(2, M, N)
            return o[0] + o[1] / 2048.0, None
        main = self.out.reshape(M + 1, self.ldo)[:M, :N].cpu().numpy().astype(np.float64)
        return main, (None if self.out2 is None else self.out2[:M * N].cpu().numpy().astype(np.float64).reshape(M, N))

    def bits(self):
        b = [self.out.cpu().numpy().view(np.uint16 if self.planes_out else np.uint32)]
        if self.out2 is not None:
            b.append(self.out2.cpu().numpy().view(np.uint32))
        return b

    def untouched(self, lib):
        ok = bool(torch.isnan(self.slab).all())
        if self.c.ep == EP_RESIDUAL:
            n = self.c.M * self.c.N
            P = _period(self.c)
            ok = ok and np.array_equal(self.out[:n].cpu().numpy(), _extras(self.c.M, self.c.N, P)[0][:self.c.M].reshape(-1)) and bool(torch.isnan(self.out[n:]).all())
        else:
            ok = ok and bool(torch.isnan(self.out).all())
        if self.out2 is not None:
            ok = ok and bool(torch.isnan(self.out2).all())
        return ok


# ---- the cases ----
ROW_PAIRS = [("plain-bias", A_F32, EP_BIAS, True), ("plain-res", A_F32, EP_RESIDUAL, False), ("plain-res2", A_F32, EP_RESIDUAL, True),
             ("plain-s2t", A_F32, EP_S2T, True), ("ln-bias", A_LN, EP_BIAS, True), ("ln-relu", A_LN, EP_BIAS_RELU, True),
             ("ln-splitq", A_LN, EP_SPLIT_Q, True), ("ln-relusplit", A_LN, EP_RELU_SPLIT, True)]
H3_ONLY = (EP_SPLIT_Q, EP_RELU_SPLIT)
# (stride, pad_left, pad_right)
CONV_GEOM = [(1, 1, 1), (2, 0, 0), (3, 1, 1), (3, 0, 0), (2, 1, 0)]


def _conv(name, src, Cc, geom, Lo, B, N, **kw):
    s, pl, pr = geom
    return Case(name, src, EP_CONV, B * Lo, N, 3 * Cc, conv=(Cc, s, pl, pr, Lo, B), **kw)


def _make_cases():
    cs = []
    for prec, tag in ((PREC_H3, "h3"), (PREC_F32, "f32")):
        h3 = prec == PREC_H3
        for nm, src, ep, opt in ROW_PAIRS:
            if not h3 and ep in H3_ONLY:
                continue
            Nq = 192                                                  # (N % 3 == 0 for SplitQ; not a multiple of 128)
            cs.append(Case(f"{nm}-small-{tag}", src, ep, 65, Nq, 384, prec, opt=opt, slab=0, want_kernel=("gemm_h3", 64, 1) if h3 else ("gemm_f32", 64, None)))
            cs.append(Case(f"{nm}-split-{tag}", src, ep, 129, Nq, 384, prec, opt=opt, expect=(3, 4)))
            cs.append(Case(f"{nm}-split96-{tag}", src, ep, 129, Nq, 768, prec, target=96, opt=opt, expect=(6, 4)))
            cs.append(Case(f"{nm}-t128deep-{tag}", src, ep, 5441, 384, 32, prec, opt=opt, want_kernel=("gemm_h3", 128, 1) if h3 else ("gemm_f32", 128, None)))
            if h3:
                cs.append(Case(f"{nm}-t128-{tag}", src, ep, 13825, 384, 32, prec, opt=opt, want_kernel=("gemm_h3", 128, 0)))
                cs.append(Case(f"{nm}-wide64-{tag}", src, ep, 13767, 192, 32, prec, opt=opt, want_kernel=("gemm_h3", 64, 0)))
        # EpSlab, not DEEP: 144 workgroups x 6 slices
        for nm, src, ep in (("plain-bias", A_F32, EP_BIAS), ("ln-bias", A_LN, EP_BIAS)):
            cs.append(Case(f"{nm}-splitwide-{tag}", src, ep, 2753, 192, 768, prec, expect=(6, 4), want_kernel=("gemm_h3", 64, 0) if h3 else ("gemm_f32", 64, None)))
        # rows, N = 51 (3 x 17: one ragged column tile, slab stride 52), K = 408 (Kp = 416: 13 k-tiles, slices of 5, 5, 3)
        for M in (1, 63, 64, 65, 127, 129):
            cs.append(Case(f"rows-M{M}-{tag}", A_F32, EP_BIAS, M, 51, 384, prec, expect=(3, 4)))
            cs.append(Case(f"K408-M{M}-{tag}", A_LN if M % 2 else A_F32, EP_BIAS, M, 51, 408, prec, expect=(3, 5)))
        for kt in (1, 2, 3):
            cs.append(Case(f"k{kt}-{tag}", A_F32, EP_BIAS, 129, 64, 32 * kt, prec, expect=(1, kt)))
        # last slices of 1, 2 and 3 k-tiles: KT = 21 (5 x 5: 5 5 5 5 1), 17 (4 x 5: 5 5 5 2), 13 (3 x 5: 5 5 3)
        for last, K, ex in ((1, 672, (5, 5)), (2, 544, (4, 5)), (3, 416, (3, 5))):
            cs.append(Case(f"last{last}-{tag}", A_F32, EP_RESIDUAL, 129, 64, K, prec, expect=ex))
        # convolution on f32 rows: every geometry, taps off both ends, L_out = 1 and 5 (a row tile spans 13 sequences), ragged M
        for gi, geom in enumerate(CONV_GEOM):
            cs.append(_conv(f"conv-g{gi}-L5-{tag}", A_CONV_F32, 32 if gi % 2 else 64, geom, 5, 27, 64, prec=prec, opt=bool(gi % 2)))
            cs.append(_conv(f"conv-g{gi}-L1-{tag}", A_CONV_F32, 64 if gi % 2 else 32, geom, 1, 70, 64, prec=prec, opt=not gi % 2))
        cs.append(_conv(f"conv-C768-split-{tag}", A_CONV_F32, 768, (3, 1, 1), 5, 27, 64, prec=prec, expect=(18, 4)))
        cs.append(_conv(f"conv-C768-unsplit-{tag}", A_CONV_F32, 768, (3, 1, 1), 5, 27, 64, prec=prec, opt=False, slab=0, expect=(1, 72)))
        cs.append(_conv(f"conv-splitwide-{tag}", A_CONV_F32, 768, (2, 0, 0), 5, 27, 384, prec=prec, expect=(18, 4),
                        want_kernel=("gemm_h3", 64, 0) if h3 else ("gemm_f32", 64, None)))
        cs.append(_conv(f"conv-t128deep-{tag}", A_CONV_F32, 32, (2, 1, 0), 5, 1089, 384, prec=prec, want_kernel=("gemm_h3", 128, 1) if h3 else ("gemm_f32", 128, None)))
        if h3:
            cs.append(_conv(f"conv-t128-{tag}", A_CONV_F32, 32, (3, 1, 1), 5, 2765, 384, prec=prec, opt=False, want_kernel=("gemm_h3", 128, 0)))
            cs.append(_conv(f"conv-wide64-{tag}", A_CONV_F32, 32, (1, 1, 1), 5, 2753, 192, prec=prec, want_kernel=("gemm_h3", 64, 0)))
    # split-rule boundaries, as the forward calls the rule (exception on): literal expectations
    cs += [Case("rule-tiles383", A_F32, EP_BIAS, 24449, 64, 544, expect=(2, 9)), Case("rule-tiles384", A_F32, EP_BIAS, 24513, 64, 544, expect=(1, 17)),
           Case("rule-KT7", A_F32, EP_BIAS, 65, 64, 224, expect=(1, 7)), Case("rule-KT8", A_F32, EP_BIAS, 65, 64, 256, expect=(2, 4)),
           Case("rule-exc-200x16", A_F32, EP_BIAS, 12737, 64, 512, expect=(1, 16)), Case("rule-exc-199x16", A_F32, EP_BIAS, 12736, 64, 512, expect=(4, 4)),
           Case("rule-exc-200x17", A_F32, EP_BIAS, 12737, 64, 544, expect=(4, 5)),
           Case("rule-slab-fits", A_F32, EP_BIAS, 129, 51, 384, slab=3 * 129 * 52, expect=(3, 4)),
           Case("rule-slab-short", A_F32, EP_BIAS, 129, 51, 384, slab=3 * 129 * 52 - 1, expect=(1, 12))]
    # planes: the LDS-DMA kernel
    for nm, ep, opt in (("g-res", EP_RESIDUAL, False), ("g-res2", EP_RESIDUAL, True), ("g-s2t", EP_S2T, True), ("g-s2t-nomask", EP_S2T, False)):
        cs.append(Case(f"{nm}-small-N51", A_PLANES, ep, 65, 51, 384, opt=opt, slab=0, want_kernel=("gemm_h3g", 64, None)))
        cs.append(Case(f"{nm}-split-N51", A_PLANES, ep, 129, 51, 384, opt=opt, expect=(3, 4)))
        cs.append(Case(f"{nm}-split96-K768", A_PLANES, ep, 129, 192, 768, target=96, opt=opt, expect=(6, 4)))
        cs.append(Case(f"{nm}-t128-unsplit", A_PLANES, ep, 2689, 384, 384, opt=opt, expect=(1, 12), want_kernel=("gemm_h3g", 128, None)))
        cs.append(Case(f"{nm}-split128", A_PLANES, ep, 2113, 384, 576, opt=opt, expect=(4, 5), want_kernel=("gemm_h3g", 128, None)))
    for M in (1, 63, 64, 65, 127, 129):
        cs.append(Case(f"g-rows-M{M}", A_PLANES, EP_RESIDUAL, M, 64, 384, opt=bool(M % 2), slab=0 if M % 2 else FULL_SLAB))
    for kt in (1, 2, 3):
        cs.append(Case(f"g-k{kt}", A_PLANES, EP_S2T, 129, 64, 32 * kt, expect=(1, kt)))
    for last, K, ex in ((1, 672, (5, 5)), (2, 544, (4, 5)), (3, 416, (3, 5))):
        cs.append(Case(f"g-last{last}", A_PLANES, EP_RESIDUAL, 129, 64, K, expect=ex))
    cs.append(Case("g-rule-exc-200x16", A_PLANES, EP_RESIDUAL, 12737, 64, 512, opt=False, expect=(1, 16)))
    cs.append(Case("g-rule-exc-199x16", A_PLANES, EP_RESIDUAL, 12736, 64, 512, opt=False, expect=(4, 4)))
    for gi, geom in enumerate(CONV_GEOM):
        cs.append(_conv(f"gconv-g{gi}-L5", A_CONV_PLANES, 32 if gi % 2 else 64, geom, 5, 27, 64, opt=bool(gi % 2)))
        cs.append(_conv(f"gconv-g{gi}-L1", A_CONV_PLANES, 64 if gi % 2 else 32, geom, 1, 70, 64, opt=not gi % 2))
    cs.append(_conv("gconv-C768-split", A_CONV_PLANES, 768, (3, 1, 1), 5, 27, 64, expect=(18, 4)))
    cs.append(_conv("gconv-C768-split96", A_CONV_PLANES, 768, (2, 0, 0), 5, 27, 64, target=96, opt=False, expect=(18, 4)))
    cs.append(_conv("gconv-C768-unsplit", A_CONV_PLANES, 768, (3, 1, 1), 5, 27, 64, opt=False, slab=0, expect=(1, 72)))
    cs.append(_conv("gconv-t128", A_CONV_PLANES, 64, (2, 1, 0), 5, 539, 384, want_kernel=("gemm_h3g", 128, None), expect=(1, 6)))
    cs.append(_conv("gconv-split128", A_CONV_PLANES, 192, (3, 1, 1), 5, 423, 384, want_kernel=("gemm_h3g", 128, None), expect=(4, 5)))
    return cs


CASES = _make_cases()
_CASES = {c.name: c for c in CASES}
assert len(_CASES) == len(CASES)


def _bound(c, want, dev):
    scale = float(np.abs(want).max())
    if c.prec == PREC_F32:
        return TOL_F32_REL * scale
    assert scale < 8.0, "the f16x3 bounds are stated for unit-scale outputs"
    b = TOL_H3 if c.K <= 384 else TOL_H3 + 2.0 * dev
    assert b <= CAP, f"allowance {b:.2e} above the whole model's bound: change the input"
    return b + (STEP if c.ep in H3_ONLY else 0.0)


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_tiled(lib, name):
    c = _CASES[name]
    kern, bn, deep, slices, kps = kernel_of(c)
    if c.expect is not None:
        assert (slices, kps) == c.expect, "the restated rule and the case's literal expectation differ"
    if c.want_kernel is not None:
        assert (kern, bn, deep) == c.want_kernel
    s, k = C.c_int32(), C.c_int32()
    assert lib.uu3d_op_tiled_split(c.M, c.N, c.K, c.target, c.slab, C.byref(s), C.byref(k)) == 0
    assert (s.value, k.value) == (slices, kps), "splitk_rule as the forward calls it and its restatement differ"
    r = Run(lib, c)
    assert r.status == 0
    r.check_guards()
    want, want2, dev = _want(c)
    bound = _bound(c, want, dev)
    got, got2 = r.values()
    assert np.isfinite(got).all()
    err = float(np.abs(got - want).max())
    err2 = 0.0
    if want2 is not None:
        assert np.isfinite(got2).all()
        err2 = float(np.abs(got2 - want2).max())
    print(f"TILED {name}: {kern} 64x{bn} deep={deep} slices={slices} kps={kps} K={c.K}: max-abs {max(err, err2):.3e} bound {bound:.3e} f32-restatement dev {dev:.2e} (scale {np.abs(want).max():.2f})")
    assert err <= bound and err2 <= bound
    # a split wrote exactly its slices of the slab
    if slices > 1:
        used = slices * c.M * ru(c.N, 4)
        assert torch.isnan(r.slab[used:]).all(), "the slab was written past slices * M * round_up(N, 4)"
    else:
        assert torch.isnan(r.slab).all(), "an unsplit launch wrote the slab"
    # two runs: equal bits
    again = Run(lib, c)
    assert all(np.array_equal(a, b) for a, b in zip(r.bits(), again.bits())), "two runs differ"
    # exact f32: the unsplit form of a split case, held to the same bound (another order of summation: not bitwise)
    if c.prec == PREC_F32 and slices > 1:
        u = Run(lib, c, slab=0)
        assert u.status == 0
        u.check_guards()
        g1, g2 = u.values()
        assert float(np.abs(g1 - want).max()) <= bound and (want2 is None or float(np.abs(g2 - want2).max()) <= bound)
        assert float(np.abs(g1 - got).max()) <= 2.0 * bound


def test_split_rule(lib):
    """uu3d_op_tiled_split == the restatement on both sides of every boundary of the rule, targets 768 and 96."""
    s, k = C.c_int32(), C.c_int32()
    n = 0
    for target in (768, 96):
        for N in (51, 64, 192, 384):
            nt = (N + 63) // 64
            for tiles_m in sorted({1, 2, 3, 199 // nt, 199 // nt + 1, 200 // nt + 1, 383 // nt, 383 // nt + 1, 384 // nt + 1}):
                for M in (64 * tiles_m - 63, 64 * tiles_m):
                    for KT in (1, 2, 3, 7, 8, 12, 13, 16, 17, 18, 21, 24, 72):
                        for slab in (0, FULL_SLAB, 3 * M * ru(N, 4), 3 * M * ru(N, 4) - 1):
                            assert lib.uu3d_op_tiled_split(M, N, 32 * KT - (24 if KT == 13 else 0), target, slab, C.byref(s), C.byref(k)) == 0
                            assert (s.value, k.value) == split_rule(M, N, KT, target, slab), (M, N, KT, target, slab)
                            n += 1
    # literal values on each side of each boundary (N = 64: tiles = row tiles)
    assert split_rule(64 * 383, 64, 17, 768, FULL_SLAB) == (2, 9) and split_rule(64 * 384, 64, 17, 768, FULL_SLAB) == (1, 17)      # (KT = 17: past the exception)
    assert split_rule(65, 64, 7, 768, FULL_SLAB) == (1, 7) and split_rule(65, 64, 8, 768, FULL_SLAB) == (2, 4)
    assert split_rule(64 * 200, 64, 16, 768, FULL_SLAB) == (1, 16) and split_rule(64 * 199, 64, 16, 768, FULL_SLAB) == (4, 4)
    assert split_rule(64 * 200, 64, 17, 768, FULL_SLAB) == (4, 5) and split_rule(64 * 200, 64, 16, 768, FULL_SLAB, exception=False) == (4, 4)
    assert split_rule(129, 51, 12, 768, 3 * 129 * 52) == (3, 4) and split_rule(129, 51, 12, 768, 3 * 129 * 52 - 1) == (1, 12)
    assert split_rule(129, 192, 24, 96, FULL_SLAB) == (6, 4)
    print(f"split rule: {n} points")


REJECTED = [
    ("planes at precision f32", "g-res-small-N51", dict(precision=PREC_F32)),
    ("plane loader with EpBias", "g-res-small-N51", dict(epilogue=EP_BIAS)),
    ("SplitQ at precision f32", "ln-splitq-small-h3", dict(precision=PREC_F32)),
    ("ReluSplit from plain rows", "ln-relusplit-small-h3", dict(a_source=A_F32)),
    ("conv epilogue from plain rows", "plain-bias-small-h3", dict(epilogue=EP_CONV)),
    ("conv loader with EpBias", "conv-g0-L5-h3", dict(epilogue=EP_BIAS)),
    ("the panel's Ln epilogue", "plain-res-small-h3", dict(epilogue=_EP_RESIDUAL_LN)),
    ("unknown source", "plain-bias-small-h3", dict(a_source=5)),
    ("K % 32 != 0 on planes", "g-res-small-N51", dict(K=376)),
    ("lda < K", "plain-bias-small-h3", dict(lda=380)),
    ("ldo < N", "plain-bias-small-h3", dict(ldo=100)),
    ("M = 0", "plain-bias-small-h3", dict(M=0)),
    ("no lo plane", "g-res-small-N51", dict(a_lo_dev=None)),
    ("no stats", "ln-bias-small-h3", dict(ln_stats_dev=None)),
    ("period 0", "g-s2t-small-N51", dict(period=0)),
    ("mask without token", "g-s2t-small-N51", dict(token_dev=None)),
    ("M not a multiple of L_out", "conv-g0-L5-h3", dict(M=134)),
    ("identity row past L_in", "conv-g1-L5-h3", dict(conv_L_in=9)),
    ("C % 32 != 0 on planes", "gconv-g0-L5", dict(conv_C=48, K=144)),
    ("K != 3 C", "conv-g0-L5-h3", dict(K=128)),
    ("slab capacity without a slab", "plain-bias-split-h3", dict(slab_dev=None)),
    ("target 0", "plain-bias-split-h3", dict(splitk_target=0)),
]


@pytest.mark.parametrize("why,name,override", REJECTED, ids=[r[0] for r in REJECTED])
def test_tiled_rejects(lib, why, name, override):
    r = Run(lib, _CASES[name], **override)
    assert r.status == INVALID, why
    assert r.untouched(lib), "a rejected call wrote something"
