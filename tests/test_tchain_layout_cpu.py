"""HOST layout helpers of the temporal chain's operator (include/uu3d_ops.h), each of which goes through the producer's own index function:
uu3d_op_tchain_xs_pack / _xs_unpack (tchain16_xs_index), uu3d_op_panel_a_pack / _a_unpack (panel_a_index), uu3d_op_attn_qf_pack / _qf_unpack
(tchain_qf_index).  pack then unpack is the identity, and each index function is a bijection onto its buffer: distinct elements packed over the
whole tiles reach every element of the buffer exactly once."""
import ctypes as C

import numpy as np
import pytest

from uplift_upsample_3dhpe_amd import _capi

MS = [1, 33, 64, 129]
INVALID = _capi.UU3D_ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _distinct_halfs(n):
    """n distinct finite f16 values (n <= 63488)."""
    bits = np.arange(n, dtype=np.uint16)
    bits = np.where(bits >= 0x7C00, bits + 0x0400, bits).astype(np.uint16)      # step over +inf / NaN into the negative range
    bits = np.where(bits >= 0xFC00, bits + 0x0400, bits).astype(np.uint16)
    v = bits.view(np.float16)
    assert np.isfinite(v).all() and len(np.unique(bits)) == n
    return v


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("slot", [0, 1])
def test_xs_pack_unpack(lib, M, slot):
    tiles = (M + 63) // 64
    n = int(lib.uu3d_op_tchain_scratch_bytes(M)) // 4
    assert n == tiles * 2 * 64 * 384 + 16384 // 4
    x = np.random.default_rng(M).normal(size=(M, 384)).astype(np.float32)
    s = np.full(n, np.nan, np.float32)
    assert lib.uu3d_op_tchain_xs_pack(_p(x), M, slot, M, _p(s)) == 0
    assert np.isfinite(s).sum() == M * 384                                          # the live rows' elements and nothing else
    lo, hi = slot * tiles * 64 * 384, (slot + 1) * tiles * 64 * 384
    assert np.isnan(s[:lo]).all() and np.isnan(s[hi:]).all()
    back = np.full((M, 384), np.nan, np.float32)
    assert lib.uu3d_op_tchain_xs_unpack(_p(s), M, slot, M, _p(back)) == 0
    assert np.array_equal(back, x)
    # bijection onto the slot: whole tiles of distinct values fill it exactly
    R = tiles * 64
    full = np.arange(R * 384, dtype=np.float32).reshape(R, 384)
    s[:] = np.nan
    assert lib.uu3d_op_tchain_xs_pack(_p(full), M, slot, R, _p(s)) == 0
    assert np.array_equal(np.sort(s[lo:hi]), full.ravel()) and np.isnan(s[:lo]).all() and np.isnan(s[hi:]).all()
    # the layout's own statement (csrc/uu3d_tchain16.h): [tile][chunk 12][wave = 4 hh + q][lane = t + 16 g][r 4], channel = 32 c + 16 hh + 4 g + r, row = 16 q + t
    row, ch = min(M - 1, 37), 213
    c, hh, g, r, q, t = ch >> 5, (ch >> 4) & 1, (ch >> 2) & 3, ch & 3, (row >> 4) & 3, row & 15
    assert s[lo + (((c * 8 + 4 * hh + q) * 64 + t + 16 * g) * 4 + r)] == full[row, ch]


def test_xs_rejects(lib):
    x = np.zeros((64, 384), np.float32)
    s = np.zeros(int(lib.uu3d_op_tchain_scratch_bytes(1)) // 4, np.float32)
    assert lib.uu3d_op_tchain_scratch_bytes(0) == 0 and lib.uu3d_op_tchain_scratch_bytes(64) == lib.uu3d_op_tchain_scratch_bytes(1)
    assert lib.uu3d_op_tchain_scratch_bytes(65) == 2 * (lib.uu3d_op_tchain_scratch_bytes(1) - 16384) + 16384
    for args in ((None, 1, 0, 1, _p(s)), (_p(x), 1, 0, 1, None), (_p(x), 0, 0, 1, _p(s)), (_p(x), 1, 2, 1, _p(s)), (_p(x), 1, -1, 1, _p(s)),
                 (_p(x), 1, 0, 0, _p(s)), (_p(x), 1, 0, 65, _p(s))):
        assert lib.uu3d_op_tchain_xs_pack(*args) == INVALID
    assert lib.uu3d_op_tchain_xs_unpack(_p(s), 1, 0, 65, _p(x)) == INVALID and lib.uu3d_op_tchain_xs_unpack(None, 1, 0, 1, _p(x)) == INVALID
    assert lib.uu3d_op_panel_a_pack(None, _p(x), 1, _p(s)) == INVALID and lib.uu3d_op_panel_a_pack(_p(x), _p(x), 0, _p(s)) == INVALID
    assert lib.uu3d_op_attn_qf_unpack(None, 1, _p(x), _p(x)) == INVALID and lib.uu3d_op_attn_qf_unpack(_p(s), 0, _p(x), _p(x)) == INVALID


@pytest.mark.parametrize("M", MS)
def test_panel_a_pack_unpack(lib, M):
    n = int(lib.uu3d_op_panel_a_bytes(M)) // 2
    rng = np.random.default_rng(M)
    hi = rng.normal(size=(M, 384)).astype(np.float16).astype(np.float32)
    lo = rng.normal(size=(M, 384)).astype(np.float16).astype(np.float32)
    f = np.full(n, np.nan, np.float16)
    assert lib.uu3d_op_panel_a_pack(_p(hi), _p(lo), M, _p(f)) == 0
    assert np.isfinite(f).sum() == 2 * M * 384
    bh, bl = np.full((M, 384), np.nan, np.float32), np.full((M, 384), np.nan, np.float32)
    assert lib.uu3d_op_panel_a_unpack(_p(f), M, _p(bh), _p(bl)) == 0
    assert np.array_equal(bh, hi) and np.array_equal(bl, lo)
    # bijection: the two planes of whole 32-row panels, distinct values, fill the buffer exactly
    R = (M + 31) // 32 * 32
    assert n == 2 * R * 384
    v = _distinct_halfs(2 * 32 * 384).astype(np.float32)
    for p0 in range(0, R, 32):                                                       # (a panel at a time: f16 has 63488 finite values)
        hi_p = np.zeros((R, 384), np.float32)
        lo_p = np.zeros((R, 384), np.float32)
        hi_p[p0:p0 + 32] = v[:32 * 384].reshape(32, 384)
        lo_p[p0:p0 + 32] = v[32 * 384:].reshape(32, 384)
        f[:] = np.nan
        assert lib.uu3d_op_panel_a_pack(_p(hi_p), _p(lo_p), R, _p(f)) == 0
        panel = f[p0 * 768:(p0 + 32) * 768].astype(np.float32)
        assert np.array_equal(np.sort(panel), np.sort(v)) and np.isfinite(f).all()
    # the layout's own statement (csrc/uu3d_gemm_panel.h): [panel][16-deep slice][plane][lane = row % 32 + 32 (k / 8 % 2)][8]
    row, k = M - 1, 205
    at = ((((row >> 5) * 24 + (k >> 4)) * 2) * 64 + ((k >> 3) & 1) * 32 + (row & 31)) * 8 + (k & 7)
    assert f[at] == np.float16(hi_p[row, k]) and f[at + 512] == np.float16(lo_p[row, k])


@pytest.mark.parametrize("M", MS)
def test_attn_qf_pack_unpack(lib, M):
    n = int(lib.uu3d_op_attn_qf_bytes(M)) // 2
    rng = np.random.default_rng(M)
    hi, lo = rng.normal(size=(M, 1152)).astype(np.float16), rng.normal(size=(M, 1152)).astype(np.float16)
    f = np.full(n, np.nan, np.float16)
    assert lib.uu3d_op_attn_qf_pack(_p(hi), _p(lo), M, _p(f)) == 0
    assert np.isfinite(f).sum() == 2 * M * 1152
    bh, bl = np.full((M, 1152), np.nan, np.float16), np.full((M, 1152), np.nan, np.float16)
    assert lib.uu3d_op_attn_qf_unpack(_p(f), M, _p(bh), _p(bl)) == 0
    assert np.array_equal(bh, hi) and np.array_equal(bl, lo)
    # bijection: whole 128-row tiles fill the buffer exactly (a 16-row group at a time: 2 x 16 x 1152 distinct halfs)
    R = (M + 127) // 128 * 128
    assert n == 2 * R * 1152
    v = _distinct_halfs(2 * 16 * 1152 + 1)[1:]                                       # (without +0: the other rows are zero-filled)
    seen = np.zeros(n, np.int32)
    for r0 in range(0, R, 16):
        hi_p, lo_p = np.zeros((R, 1152), np.float16), np.zeros((R, 1152), np.float16)
        hi_p[r0:r0 + 16] = v[:16 * 1152].reshape(16, 1152)
        lo_p[r0:r0 + 16] = v[16 * 1152:].reshape(16, 1152)
        f[:] = np.nan
        assert lib.uu3d_op_attn_qf_pack(_p(hi_p), _p(lo_p), R, _p(f)) == 0
        assert np.isfinite(f).all()
        nz = f.view(np.uint16) != 0
        seen += nz
        assert nz.sum() == len(v) and len(np.unique(f.view(np.uint16)[nz])) == len(v)
    assert (seen == 1).all()                                                         # every element belongs to exactly one (row, channel, plane)
