"""Shared by tests/test_tchain_emulation_cpu.py and tests/test_tchain_ops_gpu.py: the weights, the inputs, the float64 restatement of the
temporal chain's stages from the NAMED weights, and a numpy emulation of the kernel's arithmetic (csrc/uu3d_tchain16.h).  Everything is made
once and read-only."""
import functools

import numpy as np

import uplift_upsample_3dhpe_amd as pkg
from tests import util

K, HT = 384, 768
EPS = 1e-5
H3 = 2048.0
QSCALE = float(np.float32(1.44269504088896341) / np.sqrt(np.float32(48.0)))      # Launcher::attn_qscale(): log2(e) / sqrt(d_h) in float32
TC_PROJ, TC_MLP, TC_QKV, TC_FC1_PLANES, TC_PE = 1, 2, 4, 8, 16
FORMS = {"qkv": TC_QKV, "proj_mlp_qkv": TC_PROJ | TC_MLP | TC_QKV, "proj_mlp_qkv_pe": TC_PROJ | TC_MLP | TC_QKV | TC_PE,
         "proj_mlp": TC_PROJ | TC_MLP, "proj_fc1_planes": TC_PROJ | TC_FC1_PLANES}
M_SWEEP = (1, 15, 16, 17, 48, 49, 63, 64, 65, 129, 191)
POOL = 191
PERIOD = 41                     # config/h36m_81.json: 41 tokens
TOL = 2e-5                      # tests/test_panel_op_gpu.py, tests/test_fwd_ops_gpu.py: one LayerNorm + Dense layer, unit-scale outputs
TOL_X = 6e-5                    # three Dense layers behind one another: projection, fc1, fc2

# context channel that element c' = 16 u + 8 g + j of an attention-output row holds when q | k | v came in the chain's fragment order
# (include/uu3d_ops.h, UU3D_ATTN_IN_QFRAG): 16 u + 8 (j >> 2) + 4 g + (j & 3)
_c = np.arange(K)
TRUE_CH = 16 * (_c >> 4) + 8 * ((_c & 7) >> 2) + 4 * ((_c >> 3) & 1) + (_c & 3)
TRUE_CH.setflags(write=False)


def config(strided):
    cfg = util.load_config("h36m_81")
    cfg.TEMPORAL_TRANSFORMER_BLOCKS = 2
    if not strided:
        cfg.STRIDES, cfg.PADDINGS = [], []
    return cfg


def block(strided, i):
    return ("strided_temporal_block_" if strided else "temporal_block_") + str(i + 1)


@functools.lru_cache(maxsize=None)
def weights(strided):
    """init_weights with the chain's tensors redrawn so that every stage output is at unit scale: kernels 0.05 N(0, 1) for K = 384 and
    0.036 N(0, 1) for K = 768, biases 0.1 N(0, 1), gamma 1 +- 0.1, beta 0.1 N(0, 1), the first strided PE at unit scale."""
    arch = pkg.arch_from_config(config(strided))
    w = pkg.init_weights(arch, seed=5, perturb=0.1)
    rng = np.random.default_rng(77)
    blocks = [block(False, 0), block(False, 1)] + ([block(True, 0)] if strided else [])
    for p in blocks:
        for name in list(w):
            if not name.startswith(p + "/"):
                continue
            leaf, shape = name.rsplit("/", 1)[1], w[name].shape
            if "strided_conv" in name:
                continue
            if leaf == "kernel":
                w[name] = ((0.05 if shape[-2] == K else 0.036) * rng.normal(size=shape)).astype(np.float32)
            elif leaf == "gamma":
                w[name] = (1.0 + 0.1 * rng.normal(size=shape)).astype(np.float32)
            else:
                w[name] = (0.1 * rng.normal(size=shape)).astype(np.float32)
    if strided:
        name = "strided_temporal_pe_1/positional_encoding_weights"
        assert w[name].shape == (PERIOD, K)
        w[name] = rng.normal(size=w[name].shape).astype(np.float32)
    for a in w.values():
        a.setflags(write=False)
    return w


def split(a):
    """h3_split as the kernel's conversions give it (f16 denormal results flushed): hi = f16(a), lo = f16((a - hi) * 2048)."""
    a = np.asarray(a, np.float32)
    tiny = np.float16(2.0 ** -14)

    def cvt(v):
        h = v.astype(np.float16)
        return np.where(np.abs(h) < tiny, np.float16(0), h).astype(np.float16)

    hi = cvt(a)
    return hi, cvt((a - hi.astype(np.float32)) * np.float32(H3))


def planes_value(hi, lo):
    return hi.astype(np.float64) + lo.astype(np.float64) / H3


@functools.lru_cache(maxsize=None)
def pool():
    """(x, o_hi, o_lo): POOL residual rows as _rows of tests/test_fwd_ops_gpu.py draws them (a per-row offset and scale; row 3 scaled by 1e-6), row 5
    scaled by 30; POOL unit-scale attention-output rows as f16 planes.  The case of M rows takes the first M."""
    rng = np.random.default_rng(1000 + POOL)
    x = (rng.normal(size=(POOL, 1)) + (0.5 + np.abs(rng.normal(size=(POOL, 1)))) * rng.normal(size=(POOL, K))).astype(np.float32)
    x[3, :] *= 1e-6
    x[5, :] *= 30.0
    o_hi, o_lo = split(rng.normal(size=(POOL, K)).astype(np.float32))
    for a in (x, o_hi, o_lo):
        a.setflags(write=False)
    return x, o_hi, o_lo


# ---- float64, from the named weights ----
def f64(a):
    return np.asarray(a, np.float64)


def layer_norm64(x, g, b):
    x = f64(x)
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    return (x - mean) / np.sqrt(var + EPS) * f64(g) + f64(b)


def ref_proj(w, p, x, o_val):
    """x + context Wp + bp; o_val: the attention-output rows in the order the chain reads them (TRUE_CH)."""
    return f64(x) + f64(o_val) @ f64(w[p + "/attn/projection/kernel"])[TRUE_CH] + f64(w[p + "/attn/projection/bias"])


def ref_fc1(w, p, x1):
    y = layer_norm64(x1, w[p + "/norm2/gamma"], w[p + "/norm2/beta"])
    return np.maximum(y @ f64(w[p + "/mlp/fc1/kernel"]).reshape(K, HT) + f64(w[p + "/mlp/fc1/bias"]), 0.0)


def ref_mlp(w, p, x1):
    return f64(x1) + ref_fc1(w, p, x1) @ f64(w[p + "/mlp/fc2/kernel"]) + f64(w[p + "/mlp/fc2/bias"])


def ref_qkv(w, p, x):
    """[q qscale | k | v] of LayerNorm 1 (x): the unscaled wq, the scale applied at the end."""
    y = layer_norm64(x, w[p + "/norm1/gamma"], w[p + "/norm1/beta"])
    parts = []
    for nm in ("wq", "wk", "wv"):
        r = y @ f64(w[p + "/attn/" + nm + "/kernel"])
        if p + "/attn/" + nm + "/bias" in w:
            r = r + f64(w[p + "/attn/" + nm + "/bias"])
        parts.append(r * (QSCALE if nm == "wq" else 1.0))
    return np.concatenate(parts, axis=1)


# ---- the kernel's arithmetic in numpy float32 (csrc/uu3d_tchain16.h, csrc/uu3d_commit.inc) ----
def _fold(Wk, b, g, be, qcols=0):
    """commit: W' = diag(gamma) W, b' = b + beta W (f64 sums), q's scale folded into the first qcols columns; then the operand's hi / lo planes."""
    Wk, b = np.asarray(Wk, np.float32), np.asarray(b, np.float32)
    if g is not None:
        b = (f64(b) + f64(be) @ f64(Wk)).astype(np.float32)
        Wk = np.asarray(g, np.float32)[:, None] * Wk
    if qcols:
        b, Wk = b.copy(), Wk.copy()
        b[:qcols] *= np.float32(QSCALE)
        Wk[:, :qcols] *= np.float32(QSCALE)
    return split(Wk) + (b,)


def _mm(ah, al, bh, bl, drop):
    """hi.hi + (hi.lo + lo.hi) / 2048 with float32 accumulators; drop: "hl" (token hi x weight lo) or "lh" leaves that product out."""
    ah, al, bh, bl = (v.astype(np.float32) for v in (ah, al, bh, bl))
    a0 = ah @ bh
    a1 = np.zeros_like(a0)
    if drop != "hl":
        a1 = a1 + ah @ bl
    if drop != "lh":
        a1 = a1 + al @ bh
    return a0 + a1 * np.float32(1.0 / H3)


def _ln(x):
    x = np.asarray(x, np.float32)
    mean = x.sum(-1, keepdims=True, dtype=np.float32) * np.float32(1.0 / K)
    d = x - mean
    var = (d * d).sum(-1, keepdims=True, dtype=np.float32) * np.float32(1.0 / K)
    return split(d * (np.float32(1.0) / np.sqrt(var + np.float32(EPS))))


STAGES = ("proj", "fc1", "fc2", "qkv")


def emulate(w, p, p_next, x, o_hi, o_lo, planes_form=False, drop=None, term="hl"):
    """One PROJ | MLP | QKV launch (planes_form: PROJ | FC1_PLANES) on float32 rows x and the attention-output planes.  drop: the stage whose
    cross term `term` is left out.  Returns float64 dict: x1 (x + projection), and x2, qkv (as hi + lo / 2048), or h (planes_form)."""
    def d(stage):
        return term if drop == stage else None

    bh, bl, bias = _fold(np.asarray(w[p + "/attn/projection/kernel"])[TRUE_CH], w[p + "/attn/projection/bias"], None, None)
    x1 = np.asarray(x, np.float32) + (_mm(o_hi, o_lo, bh, bl, d("proj")) + bias)
    out = {"x1": f64(x1)}
    bh, bl, bias = _fold(np.asarray(w[p + "/mlp/fc1/kernel"]).reshape(K, HT), w[p + "/mlp/fc1/bias"], w[p + "/norm2/gamma"], w[p + "/norm2/beta"])
    ah, al = _ln(x1)
    hid = split(np.maximum(_mm(ah, al, bh, bl, d("fc1")) + bias, np.float32(0)))
    if planes_form:
        out["h"] = planes_value(*hid)
        return out
    bh, bl, bias = _fold(w[p + "/mlp/fc2/kernel"], w[p + "/mlp/fc2/bias"], None, None)
    x2 = x1
    for half in range(2):                                     # x += relu(fc1)[half] . W2[half] (+ b2 with the second half)
        s = slice(half * K, (half + 1) * K)
        y = _mm(hid[0][:, s], hid[1][:, s], bh[s], bl[s], d("fc2"))
        x2 = x2 + (y + bias if half else y)
    out["x2"] = f64(x2)
    Wk = np.concatenate([np.asarray(w[p_next + "/attn/" + nm + "/kernel"]) for nm in ("wq", "wk", "wv")], axis=1)
    b = np.concatenate([np.asarray(w.get(p_next + "/attn/" + nm + "/bias", np.zeros(K, np.float32))) for nm in ("wq", "wk", "wv")])
    bh, bl, bias = _fold(Wk, b, w[p_next + "/norm1/gamma"], w[p_next + "/norm1/beta"], qcols=K)
    ah, al = _ln(x2)
    out["qkv"] = planes_value(*split(_mm(ah, al, bh, bl, d("qkv")) + bias))
    out["qkv_in"] = f64(x2)
    return out
