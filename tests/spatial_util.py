"""The spatial stack (UpliftUpsampleTransformer.spatial_transformation up to, not including, spatial_to_temporal_fc: u_u_t.py:313-330,
vit.TransformerBlock / MultiHeadAttention / MLP of vision_transformer.py:46-68,92-156,176-195, as SURVEY.md cites them) stated twice for
the tests of the spatial kernels:

  spatial_ref64    plain numpy float64, written here from those lines, for any J, d_s, head count and hidden width;
  spatial_torch    the lines ``oracle.uplift_oracle.forward_torch`` runs for this stage (its own dense / transformer_block / layer_norm /
                   gelu_exact), at the dtype asked: float64 = the second statement of the reference, float32 = the float32 oracle whose
                   deviation from float64 scales the bounds of tests/test_spatial_ops_gpu.py.

tests/test_spatial_ref_cpu.py holds the two float64 statements to each other at 1e-12 before any kernel is judged.  Inputs and the
generic configurations of the GPU tests live here too, so that the CPU test covers exactly the dims the GPU tests use."""
import functools
import math

import numpy as np

_erf = np.frompyfunc(math.erf, 1, 1)


def _layer_norm64(x, gamma, beta, eps):
    """Keras LayerNormalization, non-fused path: biased moments over the last axis."""
    mean = x.mean(axis=-1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=-1, keepdims=True)
    inv = gamma / np.sqrt(var + eps)
    return x * inv + (beta - mean * inv)


def spatial_ref64(weights, frames, heads):
    """frames (F, J, 2) -> S (F, J d_s), float64 throughout.  The depth, d_s and the hidden width come from the weights."""
    w = {k: np.asarray(v, np.float64) for k, v in weights.items() if k.startswith(("keypoint_embedding/", "spatial_"))}
    x = np.asarray(frames, np.float64)
    F, J, _ = x.shape
    x = x @ w["keypoint_embedding/kernel"] + w["keypoint_embedding/bias"]                    # Dense(2 -> d_s), u_u_t.py:321
    x = x + w["spatial_pe/positional_encoding_weights"]                                      # :322-323
    d = x.shape[-1]
    dh = d // heads
    depth = 0
    while f"spatial_block_{depth + 1}/norm1/gamma" in w:
        depth += 1
    for i in range(depth):
        p = f"spatial_block_{i + 1}"
        y = _layer_norm64(x, w[p + "/norm1/gamma"], w[p + "/norm1/beta"], 1e-5)

        def proj(name):
            t = y @ w[f"{p}/attn/{name}/kernel"]
            if f"{p}/attn/{name}/bias" in w:
                t = t + w[f"{p}/attn/{name}/bias"]
            return t.reshape(F, J, heads, dh).transpose(0, 2, 1, 3)                           # (F, heads, J, d_h)

        q, k, v = proj("wq"), proj("wk"), proj("wv")
        logits = np.einsum("fhid,fhjd->fhij", q, k) / math.sqrt(dh)
        e = np.exp(logits - logits.max(axis=-1, keepdims=True))
        attn = e / e.sum(axis=-1, keepdims=True)
        o = np.einsum("fhij,fhjd->fhid", attn, v).transpose(0, 2, 1, 3).reshape(F, J, d)
        x = x + (o @ w[p + "/attn/projection/kernel"] + w[p + "/attn/projection/bias"])
        z = _layer_norm64(x, w[p + "/norm2/gamma"], w[p + "/norm2/beta"], 1e-5)
        z = z @ w[p + "/mlp/fc1/kernel"] + w[p + "/mlp/fc1/bias"]
        z = 0.5 * z * (1.0 + _erf(z / math.sqrt(2.0)).astype(np.float64))                     # keras gelu, approximate=False
        x = x + (z @ w[p + "/mlp/fc2/kernel"] + w[p + "/mlp/fc2/bias"])
    x = _layer_norm64(x, w["spatial_norm/gamma"], w["spatial_norm/beta"], 1e-6)              # :329
    return x.reshape(F, J * d)                                                               # "(b n) p c -> b n (p c)"


def spatial_torch(weights, frames, heads, dtype):
    """The same stage through the oracle's own functions, the lines forward_torch runs (oracle/uplift_oracle.py:232-240)."""
    import torch
    from oracle import uplift_oracle as O
    p = {k: O._t(np.array(v), dtype) for k, v in weights.items() if k.startswith(("keypoint_embedding/", "spatial_"))}
    x = O._t(np.array(frames), dtype)                          # (copies: the cached inputs are read-only arrays)
    F, J, _ = x.shape
    x = O.dense(x, p["keypoint_embedding/kernel"], p["keypoint_embedding/bias"])
    x = x + p["spatial_pe/positional_encoding_weights"]
    i = 0
    while f"spatial_block_{i + 1}/norm1/gamma" in p:
        x, _ = O.transformer_block(p, f"spatial_block_{i + 1}", x, heads, O.gelu_exact, None, None, None, 0, inner=False)
        i += 1
    x = O.layer_norm(x, p["spatial_norm/gamma"], p["spatial_norm/beta"], 1e-6)
    assert x.dtype == dtype
    return x.reshape(F, -1).numpy()


def f32_deviation(weights, frames, heads, ref64=None):
    """max |float32 oracle - float64| on S for these inputs: the scale of float32 rounding through the stack, computed on the CPU."""
    import torch
    if ref64 is None:
        ref64 = spatial_ref64(weights, frames, heads)
    return float(np.abs(spatial_torch(weights, frames, heads, torch.float32).astype(np.float64) - ref64).max())


# ---- inputs ----
EDGE_NAMES = ("zero", "tiny", "x30", "same_joints", "joint_1e3")


def edge_frames(J, seed=0):
    """The fixed edge frames, (5, J, 2) float32, in the order of EDGE_NAMES: all zero; scaled by 1e-6 (reaches the f16 denormal flush of the
    hi / lo split); scaled by 30; every joint identical (uniform attention up to the PE); one joint at 1e3."""
    rng = np.random.default_rng(1000 + seed)
    base = rng.uniform(-1, 1, size=(5, J, 2)).astype(np.float32)
    base[0] = 0.0
    base[1] *= np.float32(1e-6)
    base[2] *= np.float32(30.0)
    base[3] = base[3, 0]
    base[4, J // 2] = np.float32(1e3)
    return base


def make_frames(F, J, seed):
    """F frames uniform in [-1, 1], (F, J, 2) float32."""
    return np.random.default_rng(seed).uniform(-1, 1, size=(F, J, 2)).astype(np.float32)


# ---- configurations ----
# name: (J, d_s, d_t, heads, MLP ratio, spatial depth): the smallest dims that reach each branch of spatial_generic_kernel
GENERIC = {
    "compiled_dt256": (17, 32, 256, 8, 2.0, 4),    # the compiled spatial function on a generic handle (d_t != 384); hg 7 < 8 heads
    "j16": (16, 32, 64, 8, 2.0, 2),                # even J: J | 1 = 17 is the logit pitch
    "j5_heads2": (5, 16, 64, 2, 2.0, 2),           # fewer rows than SG_ROWS-groups fill, d_h 8
    "j13_heads3": (13, 24, 96, 3, 2.0, 2),         # 3 heads, d_h 8
    "ratio4": (17, 32, 64, 8, 4.0, 2),             # h_s = 128 > 3 d_s = 96 decides the row pitch of W
    "j32_ds128": (32, 128, 128, 8, 4.0, 2),        # 32 x 33 logits per head: head group 1 < 8 heads; d_h 16
    "depth1": (17, 16, 64, 4, 2.0, 1),             # one block
}


def generic_config(name):
    """The config of a GENERIC case (the recipe of tests/test_generic_dims_gpu.py: h36m_81 with other dims)."""
    from tests import util
    J, d_s, d_t, heads, ratio, depth = GENERIC[name]
    cfg = util.load_config("h36m_81")
    cfg.NUM_KEYPOINTS, cfg.SPATIAL_EMBED_DIM, cfg.TEMPORAL_EMBED_DIM, cfg.NUM_HEADS = J, d_s, d_t, heads
    cfg.SEQUENCE_LENGTH, cfg.STRIDES, cfg.PADDINGS, cfg.MLP_RATIO = 9, [3, 3], None, ratio
    cfg.SPATIAL_TRANSFORMER_BLOCKS, cfg.TEMPORAL_TRANSFORMER_BLOCKS = depth, 1
    cfg.MASK_STRIDE = None
    cfg.ROOT_KEYTPOINT = min(int(cfg.ROOT_KEYTPOINT), J - 1)
    return cfg


@functools.lru_cache(maxsize=None)
def arch_and_weights(name, seed, perturb):
    """(config, arch, weights) of "h36m_351" or a GENERIC case, built once; the weight arrays are read-only."""
    import uplift_upsample_3dhpe_amd as pkg
    from tests import util
    cfg = util.load_config(name) if name == "h36m_351" else generic_config(name)
    arch = pkg.arch_from_config(cfg)
    assert arch.compiled_dims == (name == "h36m_351")
    w = pkg.init_weights(arch, seed=seed, perturb=perturb)
    for a in w.values():
        a.setflags(write=False)
    return cfg, arch, w
