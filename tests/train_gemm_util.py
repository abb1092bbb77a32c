"""Cases and float64 references of the training step's GEMM forms (uu3d_op_train_dense / _wgrad and the small kernels around them,
include/uu3d_ops.h), shared by tests/test_train_gemm_ops_gpu.py (which runs them) and tests/test_train_gemm_ops_cpu.py (which holds
the references to torch float64 autograd and the cases to their branches).  Nothing here needs a GPU."""
import functools
import os

import numpy as np
import torch

from oracle import dropout_oracle
from tests.bwd_plan_util import _cdiv, _ru, _plan_gemm_nt

TA_PLAIN, TA_LN, TA_GELU, TA_CONV3, TA_CONVT = range(5)
EP_STORE, EP_BIAS, EP_BIAS_RELU, EP_RES_GATE, EP_ADD, EP_RELU_MASK, EP_GELU_GRAD, EP_CONV_RES = range(8)
WEP_STORE, WEP_STORE3 = range(2)
PREC_F32, PREC_H3 = 0, 1
DEEP_WGS = int(os.environ.get("UU3D_GEMM_DEEP_WGS", "640"))      # gemm_deep_wgs (uu3d_switches.h), read as the library reads it
FULL_SLAB = 1536 * 4096
EPS = 1e-5
ULP = 2.0 ** -23
SEED = 0x1234567890ABCDEF

# (stride, pad_left, L_in, L_out) of ZeroPadding1D + Conv1D(kernel 3, 'valid', stride): stride 1 with pad 1 on both sides; stride 3 without
# padding at L_in = 9 and at L_in = 11 (two rows left over; the identity path trims one: lo = 1); stride 2 with one row of padding in front
GEOMS = {"s1p1": (1, 1, 9, 9), "s3p0_L9": (3, 0, 9, 3), "s3p0_L11": (3, 0, 11, 3), "s2p1": (2, 1, 9, 4)}
CONV_B = 3


def pad_right(geom):
    s, pl, Li, Lo = geom
    return (Lo - 1) * s + 3 - pl - Li if s == 1 else 0          # only the stride-1 block pads behind the sequence


def lo_of(geom):
    return 1 if (geom[0] > 1 and geom[1] == 0) else 0


# ---- elementwise pieces, float64 and their torch-float32 restatements ----
def _t(x, dt):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dt)


def gelu(x, dt=torch.float64):
    t = _t(x, dt)
    return (0.5 * t * (1.0 + torch.erf(t * 0.70710678118654752440))).to(torch.float64).numpy()


def gelu_grad(x, dt=torch.float64):
    t = _t(x, dt)
    return (0.5 * (1.0 + torch.erf(t * 0.70710678118654752440)) + t * 0.39894228040143267794 * torch.exp(-0.5 * t * t)).to(torch.float64).numpy()


def layer_norm(x, g, b):
    x = x.astype(np.float64)
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    return (x - mean) / np.sqrt(var + EPS) * g.astype(np.float64) + b.astype(np.float64)


# ---- gathers ----
def conv3_gather(h, B, geom):
    """[B L_out][3 C]: tap j of output t is row t s + j of the zero-padded sequence (ALoadConv3 / TnLoadConv3)."""
    s, pl, Li, Lo = geom
    Cc = h.shape[1]
    padded = np.zeros((B, pl + Li + max(pad_right(geom), 0) + 3, Cc))
    padded[:, pl:pl + Li] = np.asarray(h, np.float64).reshape(B, Li, Cc)
    g = np.zeros((B, Lo, 3, Cc))
    for t in range(Lo):
        for j in range(3):
            g[:, t, j] = padded[:, t * s + j]
    return g.reshape(B * Lo, 3 * Cc)


def convt_gather(dz, B, geom):
    """[B L_in][3 Nn]: row (b, src), tap j reads dz[b, t] with t = (src + pad_left - j) / s where that divides and t < L_out (ALoadConvT)."""
    s, pl, Li, Lo = geom
    Nn = dz.shape[1]
    d3 = np.asarray(dz, np.float64).reshape(B, Lo, Nn)
    g = np.zeros((B, Li, 3, Nn))
    for src in range(Li):
        for j in range(3):
            q = src + pl - j
            if q >= 0 and q % s == 0 and q // s < Lo:
                g[:, src, j] = d3[:, q // s]
    return g.reshape(B * Li, 3 * Nn)


def identity_bwd_ref(dout, B, geom):
    s, pl, Li, Lo = geom
    lo = lo_of(geom)
    D = dout.shape[1]
    d3 = np.asarray(dout, np.float64).reshape(B, Lo, D)
    out = np.zeros((B, Li, D))
    for t in range(Lo):
        out[:, t * s + lo] = d3[:, t]
    return out.reshape(B * Li, D)


# ---- the operand packs (the header comment of repack_kernel, csrc/uu3d_train_kernels.h) ----
def operand_dims(kind, K, N, Cc=0):
    if kind == 1:
        return _ru(N, 128), _ru(K, 32)
    if kind == 4:
        return _ru(K, 64), _ru(N, 32)
    return _ru(Cc, 128), _ru(3 * N, 32)


def pack_ref(w, kind, Cc=0):
    """float32 operand [rows][ld], zero padded, from the Keras (in, out) kernel w[K][N]."""
    K, N = w.shape
    rows, ld = operand_dims(kind, K, N, Cc)
    out = np.zeros((rows, ld), np.float32)
    if kind == 1:
        out[:N, :K] = w.T
    elif kind == 4:
        out[:K, :N] = w
    else:
        for j in range(3):
            out[:Cc, j * N:(j + 1) * N] = w[j * Cc:(j + 1) * Cc]
    return out


def gemm_matrix(w, kind, Cc=0):
    """float64 [K_gemm][N_gemm] the GEMM multiplies its A operand by, for an operand of `kind` made from w."""
    w = w.astype(np.float64)
    if kind == 1:
        return w
    if kind == 4:
        return w.T
    Nn = w.shape[1]
    return w.reshape(3, Cc, Nn).transpose(0, 2, 1).reshape(3 * Nn, Cc)          # [j Nn + n][c] = W[j C + c][n]


# ---- launch_gemm's plan with the DEEP choice (uu3d_launch.h) ----
def plan_nn(M, N, K, slab, h3):
    p = _plan_gemm_nt(M, N, K, slab)
    grid = _ru(_cdiv(M, 64), 8) * _cdiv(N, 64)
    return dict(kernel="gemm_h3" if h3 else "gemm_f32", slices=p["slices"], kps=p["kps"], split=p["slices"] > 1,
                deep=(grid * p["slices"] <= DEEP_WGS) if h3 else None, combine="reduce" if p["slices"] > 1 else None)


# ---- NN cases ----
class NN:
    def __init__(self, name, src, ep, kind, M, N, K, geom=None, **opt):
        self.name, self.src, self.ep, self.kind, self.M, self.N, self.K, self.geom = name, src, ep, kind, M, N, K, geom
        self.opt = opt               # gate, keep, rps, drop, out2, period, scale, pad, deep (expected), zero_from (ADD)
        self.pad = opt.get("pad", 4)
        self.deep = opt.get("deep", True)


def _nn_cases():
    cs = []
    # ALoadGelu x EpBiasResGate: 5 frames x 17 joints
    for K in (64, 256):
        cs.append(NN(f"gelu-gate-K{K}", TA_GELU, EP_RES_GATE, 1, 85, 32, K, gate=True, keep=0.9, rps=17))
        cs.append(NN(f"gelu-gate-drop-K{K}", TA_GELU, EP_RES_GATE, 1, 85, 32, K, gate=True, keep=0.9, rps=17, drop=0.25))
        cs.append(NN(f"gelu-nogate-K{K}", TA_GELU, EP_RES_GATE, 1, 85, 32, K))
    # ALoadPlain x EpBiasResGate with the second stream
    for K in (96, 288):
        cs.append(NN(f"plain-gate-out2-K{K}", TA_PLAIN, EP_RES_GATE, 1, 27, 64, K, gate=True, keep=0.9, rps=9, out2=True, period=9, drop=0.25))
    cs.append(NN("plain-gate-N100-K288", TA_PLAIN, EP_RES_GATE, 1, 85, 100, 288, gate=True, keep=0.8, rps=17))
    # K = 72: the `k < K` tail of the row loaders inside the last k-tile, NaN padding columns right behind it
    cs.append(NN("gelu-gate-K72", TA_GELU, EP_RES_GATE, 1, 85, 32, 72, gate=True, keep=0.9, rps=17))
    cs.append(NN("ln-bias-K72", TA_LN, EP_BIAS, 1, 85, 100, 72))
    cs.append(NN("plain-store-M85-K72", TA_PLAIN, EP_STORE, 4, 85, 100, 72))
    # the LayerNorm-fed forward layers
    for K in (64, 256):
        cs.append(NN(f"ln-bias-K{K}", TA_LN, EP_BIAS, 1, 85, 100, K))
        cs.append(NN(f"ln-relu-K{K}", TA_LN, EP_BIAS_RELU, 1, 85, 40, K))
    # the strided convolution and its transpose: every geometry, 32 channels (unsplit) and 96 (K = 288: split)
    for g, geom in GEOMS.items():
        s, pl, Li, Lo = geom
        for Cc in (32, 96):
            cs.append(NN(f"conv3-{g}-C{Cc}", TA_CONV3, EP_CONV_RES, 1, CONV_B * Lo, 40, 3 * Cc, geom, gate=True, keep=0.9, rps=Lo,
                         drop=0.25 if Cc == 96 else 0.0, pe=(Cc == 32)))
            for scale in (1.0, 1.0 / 0.9):
                cs.append(NN(f"convt-{g}-C{Cc}-{'scaled' if scale != 1.0 else 'unit'}", TA_CONVT, EP_RELU_MASK, 5, CONV_B * Li, 40, 3 * Cc, geom, scale=scale))
    # the input-gradient GEMMs on kind-4 operands
    for M in (85, 133):
        for K in (64, 288):
            cs.append(NN(f"plain-gelugrad-M{M}-K{K}", TA_PLAIN, EP_GELU_GRAD, 4, M, 40, K))
            cs.append(NN(f"plain-relumask-M{M}-K{K}", TA_PLAIN, EP_RELU_MASK, 4, M, 100, K, scale=1.0 / 0.9 if K == 64 else 1.0))
            cs.append(NN(f"plain-store-M{M}-K{K}", TA_PLAIN, EP_STORE, 4, M, 100, K))
        cs.append(NN(f"plain-add-M{M}-head", TA_PLAIN, EP_ADD, 4, M, 96, 64, zero_from=51))
    cs.append(NN("plain-add-M85-K288", TA_PLAIN, EP_ADD, 4, 85, 40, 288))
    # not DEEP: ru(M / 64, 8) * n_tiles * slices > 640
    cs.append(NN("gelu-gate-wide", TA_GELU, EP_RES_GATE, 1, 20500, 64, 256, gate=True, keep=0.9, rps=17, deep=False, pad=0))
    cs.append(NN("ln-bias-wide", TA_LN, EP_BIAS, 1, 20500, 64, 256, deep=False, pad=0))
    cs.append(NN("convt-wide", TA_CONVT, EP_RELU_MASK, 5, 20500, 64, 264, (1, 1, 10, 10), scale=1.0 / 0.9, deep=False, pad=0, B=2050))
    return cs


NN_CASES = _nn_cases()
NN_BY_NAME = {c.name: c for c in NN_CASES}
assert len(NN_BY_NAME) == len(NN_CASES)


@functools.lru_cache(maxsize=None)
def nn_problem(name):
    """Inputs (float32) and float64 references of an NN case.  Keys: a (the loader's rows), w (Keras kernel the operand is packed from),
    pack (kind, K, N, C), bias, aux, pe, gate, init, ref, ref2, branch_zero, acc, factor, ops, extra."""
    c = NN_BY_NAME[name]
    rng = np.random.default_rng(sum(map(ord, name)) * 7919 + c.M)
    M, N, K, o = c.M, c.N, c.K, c.opt
    p = dict(gate=None, pe=None, aux=None, init=None, ref2=None, branch_zero=None, extra=0.0, ln=None)
    B = o.get("B", CONV_B)
    # the A operand
    if c.src in (TA_PLAIN, TA_LN, TA_GELU):
        a = rng.normal(size=(M, K)).astype(np.float32) * (1.5 if c.src == TA_GELU else 1.0)
        if "zero_from" in o:
            a[:, o["zero_from"]:] = 0.0
        A = a.astype(np.float64)
        if c.src == TA_GELU:
            A = gelu(a)
        elif c.src == TA_LN:
            g, b = (1 + 0.1 * rng.normal(size=K)).astype(np.float32), (0.1 * rng.normal(size=K)).astype(np.float32)
            p["ln"] = (g, b)
            A = layer_norm(a, g, b)
    elif c.src == TA_CONV3:
        Cc = K // 3
        a = rng.normal(size=(B * c.geom[2], Cc)).astype(np.float32)
        A = conv3_gather(a, B, c.geom)
    else:
        Nn = K // 3
        a = rng.normal(size=(B * c.geom[3], Nn)).astype(np.float32)
        A = convt_gather(a, B, c.geom)
    # the kernel the operand is packed from, unit-scale products
    if c.kind == 1:
        w = (rng.normal(size=(K, N)) / np.sqrt(K)).astype(np.float32); pack = (1, K, N, 0)
    elif c.kind == 4:
        Nw = o.get("zero_from", K)
        w = (rng.normal(size=(N, Nw)) / np.sqrt(Nw)).astype(np.float32); pack = (4, N, Nw, 0)
    else:
        w = (rng.normal(size=(3 * N, K // 3)) / np.sqrt(K)).astype(np.float32); pack = (5, 3 * N, K // 3, N)
    Wm = gemm_matrix(w, c.kind, N if c.kind == 5 else 0)
    acc = A[:, :Wm.shape[0]] @ Wm
    assert acc.shape == (M, N)
    bias = (0.1 * rng.normal(size=N)).astype(np.float32)
    ld = N + c.pad
    rows = np.arange(M)
    factor, ops = 1.0, 0
    if c.src == TA_GELU:                    # the device's erff is another implementation: twice the float32 restatement's deviation
        p["extra"] += 2.0 * float(np.abs(gelu(a, torch.float32) @ Wm - acc).max())
    if c.src == TA_LN:
        p["extra"] += 5e-6 * float(np.abs(acc).max())
    if c.ep == EP_STORE:
        ref = acc
    elif c.ep in (EP_BIAS, EP_BIAS_RELU):
        ref = acc + bias.astype(np.float64); ops = 1
        if c.ep == EP_BIAS_RELU:
            ref = np.maximum(ref, 0.0)
    elif c.ep in (EP_RES_GATE, EP_CONV_RES):
        y = acc + bias.astype(np.float64)
        zero = np.zeros((M, N), bool)
        if o.get("drop", 0.0) > 0.0:
            f = dropout_oracle.drop_factor((M, ld), o["drop"], SEED, 77)[:, :N].astype(np.float64)     # element index row * ld + col
            y = y * f; zero |= f == 0.0; factor *= float(f.max())
        if o.get("gate"):
            rps = o["rps"]
            gate = (rng.random(_cdiv(M, rps)) < 0.6).astype(np.float32)
            gate[0] = 0.0; gate[-1] = 1.0
            p["gate"] = gate
            keep32 = np.float32(o["keep"])
            y = y / np.float64(keep32) * gate.astype(np.float64)[rows // rps][:, None]
            zero |= (gate[rows // rps] == 0.0)[:, None]; factor /= float(keep32)
        if c.ep == EP_RES_GATE:
            xin = rng.normal(size=(M, N)).astype(np.float32)
            ref = xin.astype(np.float64) + y
            if o.get("out2"):
                pe = (0.1 * rng.normal(size=(o["period"] + 1, N))).astype(np.float32)       # (one spare row: a wrong period reads other values)
                p["pe"] = pe
                p["ref2"] = ref + pe.astype(np.float64)[rows % o["period"]]
                p["identity2"] = xin + pe[rows % o["period"]]           # float32: out2 = out + pe, one rounding
            p["identity"] = xin
        else:
            s, pl, Li, Lo = c.geom
            xin = rng.normal(size=(B * Li, N)).astype(np.float32)
            ident = xin.astype(np.float64).reshape(B, Li, N)[:, [t * s + lo_of(c.geom) for t in range(Lo)]].reshape(M, N)
            ref = ident + y
            if o.get("pe"):
                pe = (0.1 * rng.normal(size=(Lo, N))).astype(np.float32)
                p["pe"] = pe
                ref = ref + np.tile(pe.astype(np.float64), (B, 1))
                p["identity"] = ident.astype(np.float32) + np.tile(pe, (B, 1))      # float32: (identity + 0) + pe, one rounding
            else:
                p["identity"] = ident.astype(np.float32)
        p["aux"] = xin; p["branch_zero"] = zero; ops = 6
    elif c.ep == EP_ADD:
        init = rng.normal(size=(M, N)).astype(np.float32)
        p["init"] = init
        ref = init.astype(np.float64) + acc; ops = 1
    elif c.ep == EP_RELU_MASK:
        H = np.maximum(rng.normal(size=(M, N)), 0.0).astype(np.float32)           # exact zeros in about half the entries
        scale32 = np.float32(o.get("scale", 1.0))
        ref = np.where(H > 0, acc * np.float64(scale32), 0.0)
        p["aux"] = H; p["branch_zero"] = ~(H > 0); factor = float(scale32); ops = 1
    else:
        Hpre = (1.5 * rng.normal(size=(M, N))).astype(np.float32)
        gg = gelu_grad(Hpre)
        ref = acc * gg
        p["aux"] = Hpre; factor = float(np.abs(gg).max()); ops = 1
        p["extra"] += 2.0 * float(np.abs(acc * (gelu_grad(Hpre, torch.float32) - gg)).max())
    # the largest factor the epilogue multiplies the accumulator by, from the case's options alone
    if c.ep in (EP_RES_GATE, EP_CONV_RES):
        want = (float(np.float32(1.0) / (np.float32(1.0) - np.float32(o["drop"]))) if o.get("drop", 0.0) > 0.0 else 1.0) / (float(np.float32(o["keep"])) if o.get("gate") else 1.0)
        assert abs(factor - want) <= 1e-6 * want, (name, factor, want)
    elif c.ep == EP_RELU_MASK:
        assert factor == float(np.float32(o.get("scale", 1.0))), (name, factor)
    elif c.ep == EP_GELU_GRAD:
        assert 1.0 <= factor <= 1.13, (name, factor)               # max of gelu' is 1.1289 (at h = sqrt(2))
    else:
        assert factor == 1.0, (name, factor)
    p.update(a=a, w=w, pack=pack, bias=bias, ref=ref, acc=acc, factor=factor, ops=ops, ld=ld, B=B)
    return p


def nn_bound(c, p, prec):
    """None of it from what the kernels measure: the accumulator's allowance (exact f32: 2e-6 max|acc|; f16x3: 2e-5 at unit scale, K <= 384)
    times the largest factor the epilogue multiplies by, 2^-23 max|ref| per further float32 operation, and the CPU-computed terms of
    nn_problem (GELU restatement, LayerNorm bar)."""
    amax = float(np.abs(p["acc"]).max())
    if prec == PREC_F32:
        allow = 2e-6 * amax
    else:
        assert amax < 8.0 and c.K <= 384, "the f16x3 bound is stated for unit-scale accumulators and K <= 384"
        allow = 2e-5
    scale = max(float(np.abs(p["ref"]).max()), float(np.abs(p["ref2"]).max()) if p["ref2"] is not None else 0.0)
    b = allow * max(p["factor"], 1.0) + p["ops"] * ULP * scale + p["extra"]
    assert b <= 1e-4, f"allowance {b:.2e} above the whole model's bound: change the input"
    return b


# ---- TN cases ----
class TN:
    def __init__(self, name, src, ep, R, P, Q, h3=1, geom=None, slab=None, expect=None, pad=4, B=CONV_B):
        self.name, self.src, self.ep, self.R, self.P, self.Q, self.h3, self.geom, self.slab, self.expect, self.pad, self.B = \
            name, src, ep, R, P, Q, h3, geom, slab, expect, pad, B


def _tn_cases():
    cs = []
    for d, kern in ((32, "tn_f32"), (128, "tn_h3"), (160, "tn_h3")):
        cs.append(TN(f"ln-store3-d{d}-R70", TA_LN, WEP_STORE3, 70, d, 3 * d, expect=dict(kernel=kern, slices=1, combine=None)))
        cs.append(TN(f"ln-store3-d{d}-R600", TA_LN, WEP_STORE3, 600, d, 3 * d, expect=dict(kernel=kern, combine="reduce")))
    cs.append(TN("ln-store-P32-Q64", TA_LN, WEP_STORE, 85, 32, 64, expect=dict(kernel="tn_f32", slices=1)))
    cs.append(TN("ln-store-P128-Q256", TA_LN, WEP_STORE, 600, 128, 256, expect=dict(kernel="tn_h3", combine="reduce")))
    cs.append(TN("ln-store-P128-Q256-f32", TA_LN, WEP_STORE, 600, 128, 256, h3=0, expect=dict(kernel="tn_f32", combine="reduce")))
    cs.append(TN("gelu-store-R85", TA_GELU, WEP_STORE, 85, 64, 32, expect=dict(kernel="tn_f32", slices=1, combine=None)))
    cs.append(TN("gelu-store-R680", TA_GELU, WEP_STORE, 680, 64, 32, expect=dict(kernel="tn_f32", slices=5, combine="reduce")))
    cs.append(TN("gelu-store-skinny", TA_GELU, WEP_STORE, 8200, 64, 32, pad=0, expect=dict(kernel="tn_f32", KT=257, slices=52, combine="reduce16")))
    for g, geom in GEOMS.items():
        cs.append(TN(f"conv3-{g}-C32", TA_CONV3, WEP_STORE, CONV_B * geom[3], 96, 32, geom=geom, expect=dict(kernel="tn_f32", slices=1)))
        cs.append(TN(f"conv3-{g}-C64", TA_CONV3, WEP_STORE, CONV_B * geom[3], 192, 128, geom=geom, expect=dict(kernel="tn_h3", slices=1)))
    cs.append(TN("conv3-s3p0_L11-C64-split", TA_CONV3, WEP_STORE, 67 * 3, 192, 128, geom=GEOMS["s3p0_L11"], B=67, expect=dict(kernel="tn_h3", combine="reduce")))
    cs.append(TN("ln-store3-d128-small-slab", TA_LN, WEP_STORE3, 600, 128, 384, slab=2 * 128 * 384,
                 expect=dict(kernel="tn_h3", wanted=9, slices=2, combine="reduce")))
    cs.append(TN("gelu-store-small-slab", TA_GELU, WEP_STORE, 680, 64, 32, slab=3 * 64 * 32, expect=dict(kernel="tn_f32", wanted=5, slices=3, combine="reduce")))
    return cs


TN_CASES = _tn_cases()
TN_BY_NAME = {c.name: c for c in TN_CASES}
assert len(TN_BY_NAME) == len(TN_CASES)


@functools.lru_cache(maxsize=None)
def tn_problem(name):
    c = TN_BY_NAME[name]
    rng = np.random.default_rng(sum(map(ord, name)) * 104729 + c.R)
    R, P, Q = c.R, c.P, c.Q
    p = dict(ln=None, extra=0.0)
    if c.src == TA_CONV3:
        Cc = P // 3
        a = rng.normal(size=(c.B * c.geom[2], Cc)).astype(np.float32)
        A = conv3_gather(a, c.B, c.geom)
    else:
        a = rng.normal(size=(R, P)).astype(np.float32) * (1.5 if c.src == TA_GELU else 1.0)
        A = a.astype(np.float64)
        if c.src == TA_LN:
            g, b = (1 + 0.1 * rng.normal(size=P)).astype(np.float32), (0.1 * rng.normal(size=P)).astype(np.float32)
            p["ln"] = (g, b)
            A = layer_norm(a, g, b)
        elif c.src == TA_GELU:
            A = gelu(a)
    b = (rng.normal(size=(R, Q)) * np.exp(rng.uniform(-14, 0, size=(R, 1)))).astype(np.float32)      # rows from 1e-6 to 1 (gradient-sized entries)
    ref = A.T @ b.astype(np.float64)
    scale = float(np.abs(ref).max())
    bar = 2e-6 * scale                                         # test_gemm_tn_branches / test_gemm_tn_h3_branches
    if c.src == TA_LN:
        bar += 5e-6 * scale                                    # the LayerNorm bar of test_bwd_ops_edges_gpu.py
    if c.src == TA_GELU:
        bar += 2.0 * float(np.abs(gelu(a, torch.float32).T @ b.astype(np.float64) - ref).max())
    p.update(a=a, b=b, ref=ref, bar=bar)
    return p
