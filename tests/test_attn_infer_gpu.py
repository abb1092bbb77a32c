"""The forward's temporal attention kernels, every instantiation on its own through uu3d_op_attn_infer (include/uu3d_ops.h), against plain
float64 softmax attention (vit.MHA.scaled_dot_product_attention, vision_transformer.py:99-130):

  * attn_h3_kernel<48, MAXW, WPE, MASKED>, (3,3) / (12,3) / (8,2) with and without a mask, at every length edge of its 32-key tiles, its
    one-wave-per-tile and generic K / V loaders, the two-tile query loop (385 .. 416 tokens), both sides of the key-step skip
    (L mod 32 <= 16), row-major and fragment-ordered input and output, the XCD remap (16 workgroups) and the identity mapping (12);
  * attn_head_wave_kernel<4 | 5, 48, SPLIT>;
  * attn_f32_kernel<1 .. 8, 48, SPLIT>;
  * UU3D_ATTN_AUTO, the forward's rule, bit for bit against the forced kernel the rule names.
The operator launches through launch_attn_infer (csrc/uu3d_launch.h), as the forward's Launcher::attn does.

Reference: float64, from the values the kernel is given -- f32 rows for the exact-f32 kernels (logits q . k / sqrt(48), base e), hi + lo / 2048
of the two f16 planes for attn_h3_kernel (q prescaled by log2(e) / sqrt(48): the logits are the exp2 argument), so that the split of the
input is no part of the error.  Masked keys get probability exactly 0; a sequence with every key masked is the uniform mean of v (the
contract of uu3d_ops.h), stated as such: -1e9 in float64 would keep the logit differences.  Plane outputs are read as hi + lo / 2048.
Every output buffer is NaN-filled, row-major ones carry a guard row, fragment-ordered ones a guard tile; rows past B L of the last 32-row
panel must still be NaN.

Logit regimes (f32 draws, v unit normal; logit = noise of standard deviation 0.5 + a term r[key] along one direction per head):
  unit   q, k unit normal: standard deviation 1;
  ramp   r rises linearly from -10 to +10 nats over the sequence: the running maximum grows in every 32-key tile of every query;
  front  r = +10 in the first tile, -5 .. -15 (15 to 25 nats below) behind it;
  spike  r = +10 for one key of the last tile, -10 elsewhere.
|logit| <= 32 in log2 units is asserted for every case, < 16 where a sequence is fully masked (unit regime only: the f32 sums -1e9 + logit
of the kernels and of the reference round the logit away only well below their rounding steps of 64 / 128).
Masks: none; a random half with the last sequence fully masked (unit only); the first 40 keys masked (L > 40: the running maximum
jumps by 1e9; L <= 40: fully masked, unit only); only the last key attended.

Bounds (none of them taken from what these kernels measure):
  * exact-f32 kernels, unit regime: test_bwd_ops_gpu.py's measure for uu3d_op_attn_fwd, max-abs <= 5e-6 max|ref|; SPLIT output adds the
    plane representation step 2^-20 below 8 derived in test_fwd_ops_gpu.py (magnitude asserted);
  * attn_h3_kernel, unit regime: 2e-5 max-abs on unit-scale outputs, the bound for one f16x3 layer (test_panel_op_gpu.py);
  * ramp, front, spike: the unit bound + twice the deviation of a float32 numpy restatement (f32 logits, f32 softmax, f32 product) from the
    float64 reference for that case -- the reference's own error at that logit magnitude; twice because a kernel rounds in its accumulator
    chain as well as in the softmax.  The allowance is asserted <= 1e-4 for every case.
    Largest deviation of the restatement over the cases below (CPU): ramp 5.1e-6, front 4.9e-6, spike 2.9e-6 on attn_h3_kernel's inputs
    (allowances up to 3.0e-5, 3.0e-5, 2.6e-5); ramp 5.5e-6, front 3.5e-6, spike 3.1e-6 on the exact-f32 kernels' (up to ~3.2e-5 with
    5e-6 max|ref| and the plane step).
  * run to run: identical bits; OUT_PLANES and OUT_FRAG of one case: identical values after unpacking; IN_PLANES and IN_QFRAG of one case:
    identical bits, the row-major planes holding the channels of each 16-channel group in the lane order fragment-ordered rows arrive in
    (test_h3_fragment_forms says why).
Measured on an MI355X, max-abs over the cases of a kernel and regime (1056 checked launches, each run twice, 171 tests, 6 s):
              unit      ramp      front     spike
  h3          1.63e-6   3.77e-6   2.25e-6   1.65e-6
  head_wave   1.02e-6   5.18e-6   2.79e-6   7.17e-7
  f32_wg      1.18e-6   6.34e-6   3.67e-6   3.47e-6"""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DH = 48
AUTO, F32_WG, HEAD_WAVE, H3 = range(4)
IN_F32, IN_PLANES, IN_QFRAG = range(3)
OUT_F32, OUT_PLANES, OUT_FRAG = range(3)
KNAME = {AUTO: "auto", F32_WG: "f32_wg", HEAD_WAVE: "head_wave", H3: "h3"}
INVALID, UNSUPPORTED = 1, 2
TOL_F32_REL = 5e-6              # test_bwd_ops_gpu.py: uu3d_op_attn_fwd, relative to max|ref|
PLANE_STEP = 2.0 ** -20         # hi / lo representation step below 8 (test_fwd_ops_gpu.py)
TOL_H3 = 2e-5                   # test_panel_op_gpu.py: one f16x3 layer, unit-scale outputs
ALLOWANCE_MAX = 1e-4
QSCALE = np.float32(1.44269504088896341 / np.sqrt(48.0))
LOG2E = 1.44269504088896341

L_H3 = [1, 16, 17, 31, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 128, 129, 351, 384, 385, 400, 401, 416]
L_H3_FRAG = [1, 33, 48, 49, 97, 129, 385, 416]
L_HW = [49, 63, 64, 65, 71, 80]
L_F32 = [1, 15, 16, 17, 48, 49, 64, 65, 112, 113, 127, 128]
L_AUTO = [41, 48, 49, 71, 80, 81, 128, 129]
# (regime, mask); fully masked sequences (half; first40 at L <= 40) in the unit regime only
COMBOS = [("unit", "none"), ("unit", "half"), ("unit", "first40"), ("unit", "last"), ("ramp", "none"), ("ramp", "first40"),
          ("front", "none"), ("front", "first40"), ("spike", "none"), ("spike", "first40")]


COMBOS_LONG = [("unit", "half"), ("unit", "last"), ("ramp", "none"), ("ramp", "first40"), ("front", "first40"), ("spike", "none")]


def _combos(L):
    """Every combination up to 129 tokens (fully masked sequences in the unit regime only); six of them beyond, where the float64
    reference of a case is what this module's time goes to."""
    return [(r, m) for r, m in (COMBOS if L <= 129 else COMBOS_LONG) if r == "unit" or m == "none" or L > 40]


@pytest.fixture(scope="module")
def lib():
    from uplift_upsample_3dhpe_amd import _capi
    assert (_capi.UU3D_ERR_INVALID_ARGUMENT, _capi.UU3D_ERR_UNSUPPORTED) == (INVALID, UNSUPPORTED)
    assert (_capi.UU3D_ATTN_AUTO, _capi.UU3D_ATTN_F32_WG, _capi.UU3D_ATTN_HEAD_WAVE, _capi.UU3D_ATTN_H3) == (AUTO, F32_WG, HEAD_WAVE, H3)
    assert (_capi.UU3D_ATTN_IN_F32, _capi.UU3D_ATTN_IN_PLANES, _capi.UU3D_ATTN_IN_QFRAG) == (IN_F32, IN_PLANES, IN_QFRAG)
    assert (_capi.UU3D_ATTN_OUT_F32, _capi.UU3D_ATTN_OUT_PLANES, _capi.UU3D_ATTN_OUT_FRAG) == (OUT_F32, OUT_PLANES, OUT_FRAG)
    return _capi.load_library()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _hp(a):
    return a.ctypes.data_as(C.c_void_p)


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                  # (a copy: the cached inputs are read-only)


def _nan(n, dtype):
    return torch.full((n,), float("nan"), dtype=dtype, device="cuda")


# ---- inputs and references: made once per case, shared, never modified ----
def _structure(regime, L):
    """r[key], nats: the part of the logit every query shares."""
    j = np.arange(L)
    if regime == "ramp":
        return -10.0 + 20.0 * j / max(L - 1, 1) if L > 1 else np.zeros(1)
    if regime == "front":
        return np.where(j < 32, 10.0, -5.0 - 10.0 * ((j * 7) % 11) / 10.0)
    if regime == "spike":
        last = 32 * ((L - 1) // 32)
        return np.where(j == last + (L - 1 - last) // 2, 10.0, -10.0)
    raise ValueError(regime)


@functools.lru_cache(maxsize=None)
def _qkv(regime, B, L, H):
    """f32 rows [B L][3 D] = [q | k | v]; logits are q . k / sqrt(48) per head."""
    rng = np.random.default_rng([{"unit": 0, "ramp": 1, "front": 2, "spike": 3}[regime], B, L, H])
    q, k, v = (rng.normal(size=(B, L, H, DH)) for _ in range(3))
    if regime != "unit":
        u = rng.normal(size=(H, DH))
        u /= np.linalg.norm(u, axis=-1, keepdims=True)
        # noise orthogonal to u, scaled for a logit standard deviation of 0.5; along u: q carries 1, k carries r[key] sqrt(48)
        q = np.sqrt(0.5) * (q - (q * u).sum(-1, keepdims=True) * u) + u
        k = np.sqrt(0.5) * (k - (k * u).sum(-1, keepdims=True) * u) + (_structure(regime, L) * np.sqrt(DH))[None, :, None, None] * u
    x = np.concatenate([a.reshape(B * L, H * DH) for a in (q, k, v)], axis=1).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _mask(kind, B, L):
    """(B, L) uint8, 1 = attend; None: no mask."""
    if kind == "none":
        return None
    m = np.ones((B, L), np.uint8)
    if kind == "half":
        rng = np.random.default_rng([77, B, L])
        m = (rng.random((B, L)) < 0.5).astype(np.uint8)
        m[np.arange(B), rng.integers(0, L, size=B)] = 1                # at least one key each ...
        if B > 1:
            m[B - 1] = 0                                                  # ... but the last sequence: fully masked
    elif kind == "first40":
        m[:, :40] = 0
    elif kind == "last":
        m[:, :L - 1] = 0
    m.setflags(write=False)
    return m


def _split(x):
    hi = x.astype(np.float16)
    lo = ((x - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return hi, lo


@functools.lru_cache(maxsize=None)
def _planes(regime, B, L, H):
    """attn_h3_kernel's input: q prescaled in f32, then hi = f16(x), lo = f16((x - hi) * 2048); [B L][3 D] each."""
    x = _qkv(regime, B, L, H).copy()
    x[:, :H * DH] *= QSCALE
    hi, lo = _split(x)
    for a in (hi, lo):
        a.setflags(write=False)
    return hi, lo


@functools.lru_cache(maxsize=None)
def _logits(family, regime, B, L, H, dtype):
    """(logits [B][H][L][L] in the kernel's exponent base, v [B][H][L][48]) in `dtype`, from the values the kernel family is given."""
    D = H * DH
    if family == "h3":
        hi, lo = _planes(regime, B, L, H)
        x = hi.astype(np.float32) + lo.astype(np.float32) / np.float32(2048.0)       # exact in f32: 22 significant bits
    else:
        x = _qkv(regime, B, L, H)
    q, k, v = (x[:, i * D:(i + 1) * D].astype(dtype).reshape(B, L, H, DH).transpose(0, 2, 1, 3) for i in range(3))
    if family != "h3":
        q = (q * dtype(1.0 / np.sqrt(48.0))).astype(dtype)
    return np.matmul(q, k.transpose(0, 1, 3, 2)).astype(dtype), np.ascontiguousarray(v)


def _attention(family, regime, mask, B, L, H, dtype):
    """softmax attention in `dtype`: [B L][D].  Masked keys: probability 0; all keys of a sequence masked: the mean of v."""
    t, v = _logits(family, regime, B, L, H, dtype)
    keep = np.ones((B, 1, 1, L), bool) if mask is None else mask.astype(bool)[:, None, None, :]
    dead = ~keep.any(-1, keepdims=True)                                   # fully masked sequences: uniform
    t = np.where(keep, t, dtype(-np.inf))
    t = np.where(dead, dtype(0), t).astype(dtype)
    t = t - t.max(-1, keepdims=True)
    p = (np.exp2(t) if family == "h3" else np.exp(t)).astype(dtype)
    p = (p / p.sum(-1, keepdims=True, dtype=dtype)).astype(dtype)
    return np.matmul(p, v).astype(dtype).transpose(0, 2, 1, 3).reshape(B * L, H * DH)


@functools.lru_cache(maxsize=None)
def _ref(family, regime, mask_kind, B, L, H):
    """(float64 reference [B L][D], allowance beyond the unit-regime bound) for the inputs of one kernel family ("f32" rows or "h3" planes)."""
    mask = _mask(mask_kind, B, L)
    ref = _attention(family, regime, mask, B, L, H, np.float64)
    tmax = float(np.abs(_logits(family, regime, B, L, H, np.float64)[0]).max()) * (1.0 if family == "h3" else LOG2E)
    assert tmax <= 32.0, f"|logit| = {tmax} log2 units"
    if mask is not None and not mask.any(-1).all():
        assert regime == "unit" and tmax < 16.0, "fully masked sequences: unit regime, |logit| < 16"
    extra = 0.0
    if regime != "unit":
        extra = 2.0 * float(np.abs(_attention(family, regime, mask, B, L, H, np.float32).astype(np.float64) - ref).max())
    ref.setflags(write=False)
    return ref, extra


def _bound(family, split, regime, mask_kind, B, L, H):
    ref, extra = _ref(family, regime, mask_kind, B, L, H)
    if family == "h3":
        tol = TOL_H3 + extra
    else:
        tol = TOL_F32_REL * max(np.abs(ref).max(), 1e-30) + extra
        if split:
            assert np.abs(ref).max() < 8.0                                 # PLANE_STEP holds below 8
            tol += PLANE_STEP
    assert tol <= ALLOWANCE_MAX, f"allowance {tol:.3e}: shrink the regime's spread"
    return tol


_dev_cache = {}


def _cached(key, make):
    if key not in _dev_cache:
        _dev_cache[key] = make()
    return _dev_cache[key]


@functools.lru_cache(maxsize=None)
def _lane_order(lib_id):
    """perm[p]: the channel (of 16) that position p of a 16-channel group holds when v arrived fragment-ordered -- read off the producer's
    layout through uu3d_op_attn_qf_pack: piece (group u, plane) of token 0 is [lane = 32 g][8] at (((u * 2 + plane) * 64 + 32 g) * 8 halfs."""
    lib = _libs[lib_id]
    hi = (np.arange(1152) & 15).astype(np.float16).reshape(1, 1152)
    lo = np.zeros((1, 1152), np.float16)
    frag = np.full(int(lib.uu3d_op_attn_qf_bytes(1)) // 2, np.nan, np.float16)
    assert lib.uu3d_op_attn_qf_pack(_hp(hi), _hp(lo), 1, _hp(frag)) == 0
    perms = [np.concatenate([frag[((u * 2) * 64 + 32 * g) * 8:][:8] for g in range(2)]).astype(np.int64) for u in (0, 48, 71)]
    perm = perms[0]
    assert all(np.array_equal(perm, q) for q in perms)
    assert sorted(perm) == list(range(16))
    return perm


_libs = {}


class Run:
    """One call of uu3d_op_attn_infer on NaN-filled, guarded output."""

    def __init__(self, lib, kernel, in_layout, out_layout, regime, mask_kind, B, L, H, lane_rows=False):
        _libs[id(lib)] = lib
        self.lib, self.B, self.L, self.H, self.D = lib, B, L, H, H * DH
        self.in_layout, self.out_layout = in_layout, out_layout
        self.lane_rows = lane_rows or in_layout == IN_QFRAG            # the channels of a 16-channel group reach the kernel in lane order
        D, M = self.D, B * L
        if in_layout == IN_F32:
            xd = _cached(("f32", regime, B, L, H), lambda: _dev(_qkv(regime, B, L, H)))
        elif in_layout == IN_PLANES and lane_rows:
            # row-major planes holding, group by group, what the fragment-ordered buffer holds: the operands of uu3d_op_attn_qf_pack's layout
            def permuted():
                perm = _lane_order(id(lib))
                return _dev(np.concatenate([np.ascontiguousarray(a.reshape(B * L, -1, 16)[..., perm]).reshape(-1) for a in _planes(regime, B, L, H)]))
            xd = _cached(("lane rows", regime, B, L, H), permuted)
        elif in_layout == IN_PLANES:
            xd = _cached(("planes", regime, B, L, H), lambda: _dev(np.concatenate([a.reshape(-1) for a in _planes(regime, B, L, H)])))
        else:
            def pack():
                hi, lo = _planes(regime, B, L, H)
                frag = np.full(int(lib.uu3d_op_attn_qf_bytes(M)) // 2, np.nan, np.float16)
                assert lib.uu3d_op_attn_qf_pack(_hp(np.ascontiguousarray(hi)), _hp(np.ascontiguousarray(lo)), M, _hp(frag)) == 0
                return _dev(frag)
            assert D == 384
            xd = _cached(("qfrag", regime, B, L, H), pack)
        mask = _mask(mask_kind, B, L)
        md = None if mask is None else _cached(("mask", mask_kind, B, L), lambda: _dev(mask.reshape(-1)))
        if out_layout == OUT_F32:
            self.out = _nan((M + 1) * D, torch.float32)
        elif out_layout == OUT_PLANES:
            self.out = _nan((2 * M + 1) * D, torch.float16)
        else:
            self.a_halfs = int(lib.uu3d_op_panel_a_bytes(M)) // 2
            self.out = _nan(self.a_halfs + 32 * 384 * 2, torch.float16)
        self.status = lib.uu3d_op_attn_infer(_p(xd), in_layout, D, B, L, H, _p(md), kernel, _p(self.out), out_layout, None)
        torch.cuda.synchronize()

    def untouched(self):
        return bool(torch.isnan(self.out).all())

    def value(self):
        """(float64 [B L][D], raw bits) of the context rows; guards checked."""
        M, D = self.B * self.L, self.D
        if self.out_layout == OUT_F32:
            assert torch.isnan(self.out[M * D:]).all(), "rows past B L were written"
            o = self.out[:M * D].cpu().numpy()
            return o.astype(np.float64).reshape(M, D), o.view(np.uint32).reshape(M, D)
        if self.out_layout == OUT_PLANES:
            assert torch.isnan(self.out[2 * M * D:]).all(), "the planes pass 2 B L D halfs"
            o = self.out[:2 * M * D].cpu().numpy().reshape(2, M, D)
        else:
            assert torch.isnan(self.out[self.a_halfs:]).all(), "the fragments pass uu3d_op_panel_a_bytes(B L)"
            Mp = (M + 31) // 32 * 32
            frag = np.ascontiguousarray(self.out[:self.a_halfs].cpu().numpy())
            hi = np.empty((Mp, 384), np.float32); lo = np.empty((Mp, 384), np.float32)
            assert self.lib.uu3d_op_panel_a_unpack(_hp(frag), Mp, _hp(hi), _hp(lo)) == 0
            assert np.isnan(hi[M:]).all() and np.isnan(lo[M:]).all(), "fragment rows past B L were written"
            o = np.stack([hi[:M], lo[:M]]).astype(np.float16)              # (the values are halfs: exact)
        if self.lane_rows:                                                  # undo the lane order v carried to the output
            perm = _lane_order(id(self.lib))
            real = np.empty_like(o)
            real.reshape(2, M, D // 16, 16)[..., perm] = o.reshape(2, M, D // 16, 16)
            o = real
        o = np.ascontiguousarray(o)
        return o[0].astype(np.float64) + o[1].astype(np.float64) / 2048.0, o.view(np.uint16)


MEASURED = {}                   # (kernel, regime) -> max error seen (every case prints its own: pytest -s)


def _check(lib, kernel, in_layout, out_layout, regime, mask_kind, B, L, H, lane_rows=False):
    """float64 parity, guards and run-to-run identity of one case; returns (value, bits)."""
    family = "f32" if in_layout == IN_F32 else "h3"
    r = Run(lib, kernel, in_layout, out_layout, regime, mask_kind, B, L, H, lane_rows)
    assert r.status == 0
    got, bits = r.value()
    assert np.isfinite(got).all()
    ref, _ = _ref(family, regime, mask_kind, B, L, H)
    tol = _bound(family, out_layout != OUT_F32, regime, mask_kind, B, L, H)
    err = float(np.abs(got - ref).max())
    key = (KNAME[kernel], regime)
    MEASURED[key] = max(MEASURED.get(key, 0.0), err)
    print(f"attn {KNAME[kernel]} in{in_layout}{'L' if lane_rows else ''} out{out_layout} {regime}/{mask_kind} B={B} L={L} H={H}: max-abs {err:.3e} (allowed {tol:.3e}, scale {np.abs(ref).max():.2f})")
    assert err <= tol
    again = Run(lib, kernel, in_layout, out_layout, regime, mask_kind, B, L, H, lane_rows)
    assert again.status == 0 and np.array_equal(bits, again.value()[1]), "two runs differ"
    return got, bits


# ---- attn_h3_kernel ----
@pytest.mark.parametrize("L", L_H3)
def test_h3_row_major(lib, L):
    """H = 8: 8 or 16 workgroups, the XCD remap.  B = 2 up to 129 tokens and wherever a sequence is fully masked, B = 1 beyond (the float64
    reference of 16 heads x 416 x 416 logits per case is what this module's time goes to)."""
    for regime, mask_kind in _combos(L):
        _check(lib, H3, IN_PLANES, OUT_PLANES, regime, mask_kind, 2 if L <= 129 or mask_kind == "half" else 1, L, 8)


@pytest.mark.parametrize("L", L_H3)
def test_h3_identity_mapping(lib, L):
    """H = 4, D = 192, B = 3: 12 workgroups take the identity mapping."""
    for regime, mask_kind in [("unit", "half"), ("ramp", "none")] + ([("spike", "first40")] if L > 40 else []):
        _check(lib, H3, IN_PLANES, OUT_PLANES, regime, mask_kind, 3, L, 4)


@pytest.mark.parametrize("L", L_H3_FRAG)
def test_h3_fragment_forms(lib, L):
    """Fragment-ordered output against row-major planes of the same case, and fragment-ordered input against row-major planes: identical
    bits.  Fragment-ordered q | k | v hand the kernel the channels of every 16-channel group in lane order, and the bits of an MFMA dot
    product depend on the order of its terms (measured at 33 tokens: max-abs 5.15e-7 against 5.00e-7 from float64), so the row-major launch that
    fragment-ordered input is compared with holds the same values in that order -- both are held to float64 in the true channel order.
    B L is a multiple of 32 only at L = 416: a ragged last panel everywhere else."""
    B = 3 if L <= 129 else 2
    for regime, mask_kind in [("unit", "half"), ("ramp", "none")] + ([("front", "first40")] if L > 40 else []):
        _, base = _check(lib, H3, IN_PLANES, OUT_PLANES, regime, mask_kind, B, L, 8)
        _, frag = _check(lib, H3, IN_PLANES, OUT_FRAG, regime, mask_kind, B, L, 8)
        assert np.array_equal(frag, base), "fragment-ordered output differs from row-major planes"
        _, lane = _check(lib, H3, IN_PLANES, OUT_PLANES, regime, mask_kind, B, L, 8, lane_rows=True)
        for o in (OUT_PLANES, OUT_FRAG):
            _, bits = _check(lib, H3, IN_QFRAG, o, regime, mask_kind, B, L, 8)
            assert np.array_equal(bits, lane), f"fragment-ordered input (output form {o}) differs from the same rows in row-major planes"


# ---- attn_head_wave_kernel ----
@pytest.mark.parametrize("H,B", [(4, 3), (8, 2)])
@pytest.mark.parametrize("L", L_HW)
def test_head_wave(lib, L, H, B):
    for regime, mask_kind in _combos(L):
        a, _ = _check(lib, HEAD_WAVE, IN_F32, OUT_F32, regime, mask_kind, B, L, H)
        b, _ = _check(lib, HEAD_WAVE, IN_F32, OUT_PLANES, regime, mask_kind, B, L, H)
        assert np.abs(a - b).max() <= PLANE_STEP, "SPLIT on / off differ by more than the representation step"


def test_head_wave_fragment_output(lib):
    for regime, mask_kind in [("unit", "half"), ("ramp", "first40")]:
        _, planes = _check(lib, HEAD_WAVE, IN_F32, OUT_PLANES, regime, mask_kind, 3, 71, 8)
        _, frag = _check(lib, HEAD_WAVE, IN_F32, OUT_FRAG, regime, mask_kind, 3, 71, 8)
        assert np.array_equal(planes, frag)


# ---- attn_f32_kernel ----
@pytest.mark.parametrize("H,B", [(4, 3), (8, 2)])
@pytest.mark.parametrize("L", L_F32)
def test_f32_wg(lib, L, H, B):
    for regime, mask_kind in _combos(L):
        a, _ = _check(lib, F32_WG, IN_F32, OUT_F32, regime, mask_kind, B, L, H)
        b, _ = _check(lib, F32_WG, IN_F32, OUT_PLANES, regime, mask_kind, B, L, H)
        assert np.abs(a - b).max() <= PLANE_STEP, "SPLIT on / off differ by more than the representation step"


@pytest.mark.parametrize("L", [17, 65, 128])
def test_f32_wg_fragment_output(lib, L):
    _, planes = _check(lib, F32_WG, IN_F32, OUT_PLANES, "unit", "half", 3, L, 8)
    _, frag = _check(lib, F32_WG, IN_F32, OUT_FRAG, "unit", "half", 3, L, 8)
    assert np.array_equal(planes, frag)


# ---- UU3D_ATTN_AUTO: the forward's rule (attn_choose at precision f16x3, no switch set), stated here on its own ----
def _rule(L, in_layout, out_layout):
    """The kernel the forward launches for a layout pair (plane output), or minus the status of a pair it never forms."""
    if in_layout == IN_QFRAG:
        return H3                                              # (the chain's planes: attn_h3_kernel below 49 tokens too)
    h3 = out_layout != OUT_F32 and 48 < L <= 416
    if h3 != (in_layout == IN_PLANES):
        return -INVALID
    if h3:
        return H3
    if L > 128:
        return -UNSUPPORTED
    return HEAD_WAVE if 49 <= L <= 80 else F32_WG            # (H = 8: the heads come in fours)


@pytest.mark.parametrize("in_layout,out_layout", [(IN_F32, OUT_F32), (IN_F32, OUT_PLANES), (IN_PLANES, OUT_PLANES), (IN_PLANES, OUT_FRAG), (IN_QFRAG, OUT_FRAG), (IN_QFRAG, OUT_PLANES)])
@pytest.mark.parametrize("L", L_AUTO)
def test_auto_is_the_forced_kernel(lib, L, in_layout, out_layout):
    want = _rule(L, in_layout, out_layout)
    auto = Run(lib, AUTO, in_layout, out_layout, "unit", "half", 2, L, 8)
    if want < 0:
        assert auto.status == -want and auto.untouched()
        return
    assert auto.status == 0
    forced = Run(lib, want, in_layout, out_layout, "unit", "half", 2, L, 8)
    assert forced.status == 0
    assert np.array_equal(auto.value()[1], forced.value()[1]), f"auto is not {KNAME[want]}"

# ---- host guards: rejected before any launch, output untouched ----
REJECTED = [
    ("f32_wg with plane input", F32_WG, IN_PLANES, OUT_PLANES, 2, 64, 8, None, INVALID),
    ("f32_wg with fragment input", F32_WG, IN_QFRAG, OUT_PLANES, 2, 64, 8, None, INVALID),
    ("head_wave with plane input", HEAD_WAVE, IN_PLANES, OUT_PLANES, 2, 64, 8, None, INVALID),
    ("head_wave with fragment input", HEAD_WAVE, IN_QFRAG, OUT_FRAG, 2, 64, 8, None, INVALID),
    ("h3 with f32 input", H3, IN_F32, OUT_PLANES, 2, 64, 8, None, INVALID),
    ("h3 with f32 output", H3, IN_PLANES, OUT_F32, 2, 64, 8, None, INVALID),
    ("h3 with fragment input, f32 output", H3, IN_QFRAG, OUT_F32, 2, 64, 8, None, INVALID),
    ("head_wave at 48 tokens", HEAD_WAVE, IN_F32, OUT_F32, 2, 48, 8, None, INVALID),
    ("head_wave at 81 tokens", HEAD_WAVE, IN_F32, OUT_PLANES, 2, 81, 8, None, INVALID),
    ("head_wave with 2 heads", HEAD_WAVE, IN_F32, OUT_F32, 2, 64, 2, None, INVALID),
    ("head_wave with 6 heads", HEAD_WAVE, IN_F32, OUT_F32, 2, 64, 6, None, INVALID),
    ("f32_wg at 129 tokens", F32_WG, IN_F32, OUT_F32, 2, 129, 8, None, UNSUPPORTED),
    ("f32_wg at 129 tokens, planes out", F32_WG, IN_F32, OUT_PLANES, 2, 129, 8, None, UNSUPPORTED),
    ("h3 at 417 tokens", H3, IN_PLANES, OUT_PLANES, 1, 417, 8, None, UNSUPPORTED),
    ("auto at 417 tokens", AUTO, IN_PLANES, OUT_PLANES, 1, 417, 8, None, UNSUPPORTED),
    ("fragment input with D = 192", H3, IN_QFRAG, OUT_PLANES, 2, 64, 4, None, INVALID),
    ("fragment output with D = 192", H3, IN_PLANES, OUT_FRAG, 2, 64, 4, None, INVALID),
    ("fragment output with D = 192 (f32_wg)", F32_WG, IN_F32, OUT_FRAG, 2, 64, 4, None, INVALID),
    ("fragment output with D = 768 (head_wave)", HEAD_WAVE, IN_F32, OUT_FRAG, 1, 64, 16, None, INVALID),
    ("no sequence", H3, IN_PLANES, OUT_PLANES, 0, 64, 8, None, INVALID),
    ("no token", F32_WG, IN_F32, OUT_F32, 2, 0, 8, None, INVALID),
    ("no head", F32_WG, IN_F32, OUT_F32, 2, 64, 0, 0, INVALID),
    ("D is not 48 H", H3, IN_PLANES, OUT_PLANES, 2, 64, 8, 400, INVALID),
    ("unknown kernel", 4, IN_F32, OUT_F32, 2, 64, 8, None, INVALID),
    ("unknown input layout", F32_WG, 3, OUT_F32, 2, 64, 8, None, INVALID),
    ("unknown output layout", F32_WG, IN_F32, 3, 2, 64, 8, None, INVALID),
]


@pytest.mark.parametrize("why,kernel,in_layout,out_layout,B,L,H,D,status", REJECTED, ids=[r[0] for r in REJECTED])
def test_rejects(lib, why, kernel, in_layout, out_layout, B, L, H, D, status):
    # buffers of a legal shape (2 x 128 tokens, 8 heads, planes or rows as the call names them) only have to exist: rejected before any launch
    xd = _cached(("reject", in_layout), lambda: torch.zeros(max(int(lib.uu3d_op_attn_qf_bytes(512)), 512 * 3 * 768 * 4), dtype=torch.uint8, device="cuda"))
    out = _nan(2 * (512 + 32) * 768 * 2, torch.float16)
    st = lib.uu3d_op_attn_infer(_p(xd), in_layout, D if D is not None else H * DH, B, L, H, None, kernel, _p(out), out_layout, None)
    torch.cuda.synchronize()
    assert st == status, why
    assert torch.isnan(out).all(), "a rejected call wrote something"


def test_rejects_null_and_misaligned(lib):
    xd = torch.zeros(2 * 64 * 1152 + 8, dtype=torch.float32, device="cuda")
    out = _nan(2 * 64 * 384 + 8, torch.float32)
    assert lib.uu3d_op_attn_infer(None, IN_F32, 384, 2, 64, 8, None, F32_WG, _p(out), OUT_F32, None) == INVALID
    assert lib.uu3d_op_attn_infer(_p(xd), IN_F32, 384, 2, 64, 8, None, F32_WG, None, OUT_F32, None) == INVALID
    assert lib.uu3d_op_attn_infer(C.c_void_p(xd.data_ptr() + 4), IN_F32, 384, 2, 64, 8, None, F32_WG, _p(out), OUT_F32, None) == INVALID
    assert lib.uu3d_op_attn_infer(_p(xd), IN_F32, 384, 2, 64, 8, None, F32_WG, C.c_void_p(out.data_ptr() + 8), OUT_F32, None) == INVALID
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    assert lib.uu3d_op_attn_qf_bytes(0) == 0 and lib.uu3d_op_attn_qf_bytes(1) == lib.uu3d_op_attn_qf_bytes(128) == 4 * 72 * 2 * 512 * 2
    assert lib.uu3d_op_attn_qf_bytes(129) == 2 * lib.uu3d_op_attn_qf_bytes(128)
    assert lib.uu3d_op_attn_qf_pack(None, None, 1, None) == INVALID
