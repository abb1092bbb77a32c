"""GPU: the inference instantiation of the tiled exact-f32 attention (csrc/uu3d_attn_long.h, attn_long_fwd_kernel<48, false>) on its own,
through uu3d_op_attn_long_infer (include/uu3d_ops.h) -- the kernel an exact-f32 forward call takes for its attention layers of 129 .. 416
tokens.  It is the training instantiation without the statistics, so O must carry the same BITS as uu3d_op_attn_long_fwd writes; float64
softmax attention is the yardstick, the <= 128-token kernels a second opinion where they exist."""
import ctypes as C

import numpy as np
import pytest

from tests import util  # noqa: F401

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# tests/test_long_sequence_training_gpu.py holds the training forward (and the two exact-f32 families against each other) to
# max |O - ref| <= 5e-6 * max |ref|: _close(out, ..., 5e-6)
OUT_REL = 5e-6
LONG = [129, 144, 191, 192, 193, 257, 351, 416]     # first ragged tile / whole tile, workgroup not full / the 64-row chunk's edges / the limit
SHORT = [1, 16, 64, 128]                            # uu3d_op_attn_fwd exists there
MASKS = ["none", "alternate", "one_sequence_all_masked", "single_live_key_in_last_tile"]
PAD_ROWS = 3


@pytest.fixture(scope="module")
def lib():
    from uplift_upsample_3dhpe_amd import _capi
    return _capi.load_library()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _mask(kind, B, L, rng):
    """-> ((B, L) bool, 1 = live key) or None, and the index of the all-masked sequence or None."""
    if kind == "none":
        return None, None
    if kind == "alternate":
        m = np.zeros((B, L), bool); m[:, ::2] = True
        return m, None
    m = rng.random((B, L)) < 0.5
    m[:, 0] = True
    if kind == "one_sequence_all_masked":
        m[B - 1] = False
        return m, B - 1
    m[0] = False; m[0, L - 1] = True                # one live key, in the last (possibly ragged) tile
    return m, None


def _reference(qkv, m, B, L, H):
    """Float64 softmax attention on the device -> (B L, D) float64."""
    D = 48 * H
    t = qkv.double()
    q, k, v = [t[:, i * D:(i + 1) * D].reshape(B, L, H, 48).permute(0, 2, 1, 3) for i in range(3)]
    logits = torch.matmul(q, k.transpose(-1, -2)) / np.sqrt(48.0)
    if m is not None:
        logits = logits + (1.0 - m.double())[:, None, None, :] * -1e9
    return torch.matmul(torch.softmax(logits, -1), v).permute(0, 2, 1, 3).reshape(B * L, D)


def _infer(lib, qkv, md, B, L, H, ldo, ld=None):
    D = 48 * H
    out = torch.full((B * L + PAD_ROWS, ldo), float("nan"), device="cuda")
    assert lib.uu3d_op_attn_long_infer(_p(qkv), 3 * D if ld is None else ld, D, B, L, H, _p(md), _p(out), ldo, None) == 0
    torch.cuda.synchronize()
    return out


def _train(lib, qkv, md, B, L, H, ldo, ld=None):
    D = 48 * H
    out = torch.full((B * L + PAD_ROWS, ldo), float("nan"), device="cuda")
    stats = torch.full((B, H, L, 2), float("nan"), device="cuda")
    assert lib.uu3d_op_attn_long_fwd(_p(qkv), 3 * D if ld is None else ld, D, B, L, H, _p(md), _p(out), ldo, _p(stats), None) == 0
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("B,H", [(1, 1), (3, 8)])
@pytest.mark.parametrize("L", SHORT + LONG)
def test_inference_instantiation(lib, L, B, H):
    D = 48 * H
    rng = np.random.default_rng(1000 * L + 10 * B + H)
    qkv = torch.from_numpy(rng.normal(size=(B * L, 3 * D)).astype(np.float32)).cuda()
    worst = 0.0
    for kind in MASKS:
        m, dead = _mask(kind, B, L, rng)
        md = None if m is None else torch.from_numpy(m.astype(np.uint8)).cuda()
        ref = _reference(qkv, None if m is None else torch.from_numpy(m).cuda(), B, L, H)
        live = torch.ones(B * L, dtype=torch.bool, device="cuda")
        if dead is not None:        # every logit rounds to exactly -1e9 in f32: uniform attention, which float64 does not reproduce
            live[dead * L:(dead + 1) * L] = False
        scale = ref[live].abs().max().item() if bool(live.any()) else 1.0
        for ldo in (D, D + 8):
            out = _infer(lib, qkv, md, B, L, H, ldo)
            # the padding columns and the rows behind the last are untouched; everything else is written
            assert bool(torch.isnan(out[B * L:]).all()) and bool(torch.isnan(out[:, D:]).all())
            o = out[:B * L, :D]
            assert bool(torch.isfinite(o).all())
            # the claim: the bits of the training instantiation
            assert torch.equal(o, _train(lib, qkv, md, B, L, H, ldo)[:B * L, :D])
            # run to run
            assert torch.equal(out[:B * L, :D], _infer(lib, qkv, md, B, L, H, ldo)[:B * L, :D])
            if bool(live.any()):
                err = (o.double() - ref)[live].abs().max().item() / scale
                worst = max(worst, err)
                assert err <= OUT_REL, (kind, ldo, err)
            if dead is not None:
                v = qkv[dead * L:(dead + 1) * L, 2 * D:]
                mean_v = v.double().mean(0, keepdim=True).expand(L, D)
                assert (o[dead * L:(dead + 1) * L].double() - mean_v).abs().max().item() <= OUT_REL * mean_v.abs().max().item()
                # exactly uniform: every query row of the sequence is the same row, bit for bit
                assert torch.equal(o[dead * L:(dead + 1) * L], o[dead * L:dead * L + 1].expand(L, D))
            if L <= 128:
                short = torch.full((B * L, ldo), float("nan"), device="cuda")
                assert lib.uu3d_op_attn_fwd(_p(qkv), 3 * D, D, B, L, H, 48, _p(md), _p(short), ldo, None) == 0
                torch.cuda.synchronize()
                dev = (o - short[:, :D]).abs().max().item()
                assert dev <= OUT_REL * short[:, :D].abs().max().item(), (kind, ldo, dev)
    print(f"L = {L} B = {B} H = {H}: worst relative error against float64 {worst:.2e}")


def test_padded_input_rows(lib):
    """ld > 3 D (q | k | v rows inside a wider buffer), masked, at a ragged length: the same bits as the packed rows give."""
    B, L, H = 2, 193, 8
    D = 48 * H
    rng = np.random.default_rng(5)
    packed = torch.from_numpy(rng.normal(size=(B * L, 3 * D)).astype(np.float32)).cuda()
    wide = torch.full((B * L, 3 * D + 12), float("nan"), device="cuda")
    wide[:, :3 * D] = packed
    m, _ = _mask("alternate", B, L, rng)
    md = torch.from_numpy(m.astype(np.uint8)).cuda()
    a = _infer(lib, packed, md, B, L, H, D)
    b = _infer(lib, wide, md, B, L, H, D, ld=3 * D + 12)
    assert torch.equal(a[:B * L], b[:B * L]) and bool(torch.isfinite(a[:B * L]).all())


def test_host_guards_reject_before_any_launch(lib):
    from uplift_upsample_3dhpe_amd import _capi
    B, H, D = 1, 8, 384
    qkv = torch.zeros(420 * (3 * D + 4) + 8, device="cuda")
    out = torch.full((420 * (D + 8) + 8,), float("nan"), device="cuda")

    def call(L=129, D_=D, ld=3 * D, ldo=D, qoff=0, ooff=0, B_=B, H_=H):
        q = C.c_void_p(qkv.data_ptr() + 4 * qoff)
        o = C.c_void_p(out.data_ptr() + 4 * ooff)
        st = lib.uu3d_op_attn_long_infer(q, ld, D_, B_, L, H_, None, o, ldo, None)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), "a rejected call wrote to out"
        return st

    assert call(D_=32 * H) == _capi.UU3D_ERR_UNSUPPORTED                  # head dim 32
    assert call(D_=D + 48) == _capi.UU3D_ERR_UNSUPPORTED                  # D != 48 H
    assert call(L=0) == _capi.UU3D_ERR_UNSUPPORTED
    assert call(L=417) == _capi.UU3D_ERR_UNSUPPORTED
    assert call(qoff=1) == _capi.UU3D_ERR_INVALID_ARGUMENT                # pointers that are not 16-byte aligned
    assert call(ooff=2) == _capi.UU3D_ERR_INVALID_ARGUMENT
    assert call(ld=3 * D + 2) == _capi.UU3D_ERR_INVALID_ARGUMENT          # rows that are not
    assert call(ldo=D + 1) == _capi.UU3D_ERR_INVALID_ARGUMENT
    assert call(B_=0) == _capi.UU3D_ERR_INVALID_ARGUMENT
    assert lib.uu3d_op_attn_long_infer(None, 3 * D, D, B, 129, H, None, _p(out), D, None) == _capi.UU3D_ERR_INVALID_ARGUMENT
    assert lib.uu3d_op_attn_long_infer(_p(qkv), 3 * D, D, B, 416, H, None, _p(out), D, None) == 0      # the limit itself is taken
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:416 * D]).all()) and bool(torch.isnan(out[416 * D:]).all())
