"""Backward building blocks (include/uu3d_ops.h) at the small shapes where their host dispatch (csrc/uu3d_launch.h) changes kernel,
split factor or combine: ragged tiles, leading dimensions wider than the rows, reduced scratch, masks, and the refusals of the ABI.

Every case runs in one harness: inputs sit in buffers whose padding columns hold NaN (a kernel that reads padding poisons its result),
outputs in NaN buffers with padding columns and one sentinel row before and after (which must stay bitwise untouched), every element
inside must come back finite, and two runs must agree bitwise.  References are float64.  Each case asserts, through a restatement of the
host plan arithmetic, that its shape really selects the branch it is named after."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 5
NAN = float("nan")
GUARD = 1024                       # floats behind a reduced scratch buffer that must stay untouched


@pytest.fixture(scope="module")
def lib():
    from uplift_upsample_3dhpe_amd import _capi
    return _capi.load_library()


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _close(a, b, rel):
    scale = max(np.abs(b).max(), 1e-30)
    err = np.abs(a - b).max()
    print(f"max-abs error {err:.3e} scale {scale:.3e} relative {err / scale:.3e} bar {rel:.3e}")
    assert err <= rel * scale, (err, scale, err / scale, rel)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _in(a, ld):
    """Rows of `a` in a device buffer of row stride ld, NaN in the padding columns."""
    a = np.asarray(a, dtype=np.float32)
    buf = np.full((a.shape[0], ld), np.nan, dtype=np.float32)
    buf[:, :a.shape[1]] = a
    return _d(buf)


class _Out:
    """rows x width result inside a NaN buffer of row stride ld with one sentinel row before and after."""

    def __init__(self, rows, width, ld=None, init=None):
        self.rows, self.width, self.ld = rows, width, ld or width
        self.buf = torch.full((rows + 2, self.ld), NAN, device="cuda")
        if init is not None:
            self.buf[1:-1, :width] = _d(np.asarray(init, dtype=np.float32).reshape(rows, width))
        self.before = self.buf.clone()

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + 4 * self.ld)

    def untouched(self):
        assert torch.equal(_bits(self.buf), _bits(self.before)), "a refused call wrote to its output"

    def result(self):
        assert torch.equal(_bits(self.buf[0]), _bits(self.before[0])), "sentinel row before the result was written"
        assert torch.equal(_bits(self.buf[-1]), _bits(self.before[-1])), "sentinel row after the result was written"
        if self.ld > self.width:
            assert torch.equal(_bits(self.buf[:, self.width:]), _bits(self.before[:, self.width:])), "padding columns were written"
        inner = self.buf[1:-1, :self.width]
        assert bool(torch.isfinite(inner).all()), "non-finite element in the result"
        return inner.cpu().numpy().copy()


class _Scratch:
    """n floats of NaN scratch followed by a guard that must stay untouched (n None: the full operator scratch)."""
    _full = None

    def __init__(self, lib, n=None):
        if n is None:
            n = int(lib.uu3d_op_scratch_floats())
            if _Scratch._full is None:
                _Scratch._full = torch.empty(n + GUARD, device="cuda")
            self.buf = _Scratch._full
        else:
            self.buf = torch.empty(n + GUARD, device="cuda")
        self.n = n
        self.buf.fill_(NAN)
        self.guard = self.buf[n:].clone()

    @property
    def ptr(self):
        return _p(self.buf)

    def check(self):
        assert torch.equal(_bits(self.buf[self.n:]), _bits(self.guard)), "scratch was written beyond scratch_floats"

    def untouched(self):
        assert bool(torch.isnan(self.buf).all()), "a refused call wrote to scratch"


def _twice(run):
    """run() -> tuple of arrays; both runs must agree bitwise."""
    a, b = run(), run()
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int32), y.view(np.int32)), "two runs differ"
    return a


from tests.bwd_plan_util import _cdiv, _ru, _plan_gemm_tn, _plan_gemm_nt, _plan_colsum, _plan_ln_bwd, _plan_attn      # noqa: F401  (the restated host plans)


# ---------------------------------------------------------------------------------------------------------------------------------
# gemm_tn
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tn_problem(R, P, Q, scaled):
    rng = np.random.default_rng(1000 * R + 10 * P + Q)
    a = rng.normal(size=(R, P)).astype(np.float32)
    b = rng.normal(size=(R, Q))
    if scaled:
        b = b * np.exp(rng.uniform(-14, 0, size=(R, 1)))          # rows from 1e-6 to 1 (gradient-sized entries)
    b = b.astype(np.float32)
    return a, b, a.astype(np.float64).T @ b.astype(np.float64)


def _run_tn(lib, fn, a, b, pad, scratch_floats):
    R, P = a.shape
    Q = b.shape[1]
    ad, bd = _in(a, P + pad), _in(b, Q + 2 * pad)

    def run():
        c, sc = _Out(P, Q, Q + pad), _Scratch(lib, scratch_floats)
        assert fn(_p(ad), P + pad, _p(bd), Q + 2 * pad, R, P, Q, c.ptr, Q + pad, sc.ptr, sc.n, None) == OK
        out = c.result()
        sc.check()
        return (out,)
    return _twice(run)[0]


TN_CASES = [
    # id, (R, P, Q), pad, scratch floats (None: full), expected plan
    ("unsplit_R1", (1, 4, 4), 0, None, dict(KT=1, slices=1, combine=None)),
    ("unsplit_KT1_ragged", (31, 4, 8), 0, None, dict(KT=1, slices=1, combine=None)),
    ("two_slices_ragged_everywhere", (257, 68, 132), 0, None, dict(KT=9, tiles=6, slices=2, kps=5, combine="reduce")),
    ("two_slices_ragged_everywhere_strided", (257, 68, 132), 4, None, dict(KT=9, tiles=6, slices=2, kps=5, combine="reduce")),
    ("skinny_reduce16", (8211, 32, 32), 0, None, dict(KT=257, tiles=1, slices=52, kps=5, combine="reduce16")),
    ("scratch_cuts_8_to_3", (1000, 64, 64), 0, 3 * 64 * 64, dict(wanted=8, slices=3, kps=11, combine="reduce")),
    ("scratch_cuts_to_direct_store", (1000, 64, 64), 0, 64 * 64, dict(wanted=8, slices=1, combine=None)),
    ("strided_unsplit", (100, 36, 20), 8, None, dict(KT=4, slices=1, combine=None)),
]


@pytest.mark.parametrize("shape,pad,scratch,expect", [c[1:] for c in TN_CASES], ids=[c[0] for c in TN_CASES])
def test_gemm_tn_branches(lib, shape, pad, scratch, expect):
    R, P, Q = shape
    plan = _plan_gemm_tn(R, P, Q, scratch if scratch is not None else int(lib.uu3d_op_scratch_floats()))
    assert plan["kernel"] == "tn_f32" and {k: plan[k] for k in expect} == expect, plan
    a, b, ref = _tn_problem(R, P, Q, False)
    _close(_run_tn(lib, lib.uu3d_op_gemm_tn, a, b, pad, scratch), ref, 2e-6)


TNH_CASES = [
    ("fallback_narrow_P", (300, 124, 256), 0, None, dict(kernel="tn_f32", slices=2)),
    ("fallback_narrow_Q", (300, 256, 124), 0, None, dict(kernel="tn_f32", slices=2)),
    ("one_k_tile_unsplit", (20, 128, 128), 0, None, dict(kernel="tn_h3", KT=1, slices=1, combine=None)),
    ("two_k_tiles_unsplit", (40, 128, 128), 0, None, dict(kernel="tn_h3", KT=2, slices=1, combine=None)),
    ("strided_ragged", (777, 132, 200), 4, None, dict(kernel="tn_h3", tiles=4, slices=9, kps=3, combine="reduce")),
    ("slab_for_two_slices", (777, 128, 256), 0, 2 * 128 * 256, dict(kernel="tn_h3", wanted=12, slices=2, kps=13, combine="reduce")),
]


@pytest.mark.parametrize("shape,pad,scratch,expect", [c[1:] for c in TNH_CASES], ids=[c[0] for c in TNH_CASES])
def test_gemm_tn_h3_branches(lib, shape, pad, scratch, expect):
    R, P, Q = shape
    if "UU3D_TNH_WGS" not in os.environ:                     # the expected slice counts are those of the default workgroup target
        plan = _plan_gemm_tn(R, P, Q, scratch if scratch is not None else int(lib.uu3d_op_scratch_floats()), h3=True)
        assert {k: plan[k] for k in expect} == expect, plan
    a, b, ref = _tn_problem(R, P, Q, True)
    got = _run_tn(lib, lib.uu3d_op_gemm_tn_h3, a, b, pad, scratch)
    _close(got, ref, 2e-6)
    if expect["kernel"] == "tn_f32":                         # the fallback IS the exact-f32 operator
        exact = _run_tn(lib, lib.uu3d_op_gemm_tn, a, b, pad, scratch)
        assert np.array_equal(got.view(np.int32), exact.view(np.int32))


def test_gemm_tn_refusals(lib):
    a, b, _ = _tn_problem(31, 4, 8, False)
    ad, bd = _in(a, 8), _in(b, 8)
    for fn in (lib.uu3d_op_gemm_tn, lib.uu3d_op_gemm_tn_h3):
        for lda, ldb, R, P, Q, ldc in [(8, 8, 31, 4, 8, 4), (8, 4, 31, 4, 8, 8), (0, 8, 31, 4, 8, 8), (8, 8, 31, 4, 6, 8),
                                       (6, 8, 31, 4, 8, 8), (8, 8, 0, 4, 8, 8)]:
            c, sc = _Out(4, 8), _Scratch(lib, 64)
            assert fn(_p(ad), lda, _p(bd), ldb, R, P, Q, c.ptr, ldc, sc.ptr, sc.n, None) == INVALID
            c.untouched(); sc.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------
# gemm_nt
# ---------------------------------------------------------------------------------------------------------------------------------
NT_CASES = [
    ("one_row", (1, 64, 32), 0, None, dict(KT=1, slices=1)),
    ("split_ragged_M", (65, 64, 384), 0, None, dict(KT=12, slices=3, kps=4)),
    ("two_k_tiles_unsplit", (777, 128, 64), 0, None, dict(KT=2, slices=1)),
    ("strided_split", (213, 384, 768), 8, None, dict(KT=24, slices=6, kps=4)),
    ("scratch_below_two_slabs_unsplit", (65, 64, 384), 0, 2 * 65 * 64 - 1, dict(wanted=3, slices=1, kps=12)),
]


@pytest.mark.parametrize("shape,pad,scratch,expect", [c[1:] for c in NT_CASES], ids=[c[0] for c in NT_CASES])
def test_gemm_nt_branches(lib, shape, pad, scratch, expect):
    M, N, K = shape
    plan = _plan_gemm_nt(M, N, K, scratch if scratch is not None else int(lib.uu3d_op_scratch_floats()))
    assert {k: plan[k] for k in expect} == expect, plan
    rng = np.random.default_rng(7 + M)
    a = rng.normal(size=(M, K)).astype(np.float32); w = rng.normal(size=(N, K)).astype(np.float32)
    ad, wd = _in(a, K + pad), _d(w)

    def run():
        c, sc = _Out(M, N, N + pad), _Scratch(lib, scratch)
        assert lib.uu3d_op_gemm_nt(_p(ad), K + pad, _p(wd), K, M, N, K, c.ptr, N + pad, sc.ptr, sc.n, None) == OK
        out = c.result()
        sc.check()
        return (out,)
    _close(_twice(run)[0], a.astype(np.float64) @ w.astype(np.float64).T, 2e-6)


@pytest.mark.parametrize("M,N,K,lda,ldw,ldc", [(5, 96, 64, 64, 64, 96), (5, 64, 48, 48, 48, 64), (5, 64, 64, 64, 68, 64),
                                               (5, 64, 64, 60, 64, 64), (5, 64, 64, 66, 64, 64), (5, 64, 64, 64, 64, 60), (0, 64, 64, 64, 64, 64)],
                         ids=["N_96", "K_48", "ldw_not_K", "lda_below_K", "lda_not_x4", "ldc_below_N", "M_0"])
def test_gemm_nt_refusals(lib, M, N, K, lda, ldw, ldc):
    ad, wd = torch.ones(8, 128, device="cuda"), torch.ones(128, 128, device="cuda")
    c, sc = _Out(8, 128), _Scratch(lib, 4096)
    assert lib.uu3d_op_gemm_nt(_p(ad), lda, _p(wd), ldw, M, N, K, c.ptr, ldc, sc.ptr, sc.n, None) == INVALID
    c.untouched(); sc.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------
# colsum
# ---------------------------------------------------------------------------------------------------------------------------------
COLSUM_CASES = [
    # id, R, C, ldx, period, masked, want, accumulate, expected plan
    ("colsum4_one_slice", 63, 8, 8, 0, False, 0, 0, dict(kernel="colsum4", slices=1, cgs=2, combine=16)),
    ("colsum4_129_slices_reduce64", 8256, 8, 8, 0, False, 0, 0, dict(kernel="colsum4", slices=129, combine=64)),
    ("colsum4_two_column_blocks_strided", 300, 260, 264, 0, False, 0, 0, dict(kernel="colsum4", cgs=64, xb=2, slices=4)),
    ("generic_C_not_x4", 300, 30, 30, 0, False, 0, 0, dict(kernel="generic", slices=2)),
    ("generic_ldx_33", 300, 32, 33, 0, False, 0, 0, dict(kernel="generic", slices=2)),
    ("generic_128_slices_reduce64", 16389, 5, 5, 0, False, 0, 0, dict(kernel="generic", slices=128, combine=64)),
    ("masked_want0", 300, 32, 32, 0, True, 0, 0, dict(kernel="generic", slices=2)),
    ("masked_want1_accumulate", 300, 32, 32, 0, True, 1, 1, dict(kernel="generic", slices=2)),
    ("period4_one_slice", 3 * 7, 8, 8, 7, False, 0, 0, dict(kernel="period4", slices=1)),
    ("period4_strided", 37 * 5, 64, 68, 5, False, 0, 0, dict(kernel="period4", slices=9)),
    ("period4_accumulate", 37 * 5, 64, 64, 5, False, 0, 1, dict(kernel="period4", slices=9)),
    ("generic_period_ragged_R", 5 * 7 + 3, 8, 8, 7, False, 0, 0, dict(kernel="generic", slices=1)),
    ("generic_period_masked_accumulate", 64 * 3, 12, 12, 3, True, 0, 1, dict(kernel="generic", slices=1)),
    ("generic_period_masked_want1_two_slices", 100 * 3, 12, 16, 3, True, 1, 0, dict(kernel="generic", slices=2)),
]


@pytest.mark.parametrize("R,Cc,ldx,period,masked,want,acc,expect", [c[1:] for c in COLSUM_CASES], ids=[c[0] for c in COLSUM_CASES])
def test_colsum_branches(lib, R, Cc, ldx, period, masked, want, acc, expect):
    plan = _plan_colsum(ldx, R, Cc, period, masked, int(lib.uu3d_op_scratch_floats()))
    assert {k: plan[k] for k in expect} == expect, plan
    rng = np.random.default_rng(R * 31 + Cc)
    P = max(period, 1)
    x = rng.normal(size=(R, Cc)).astype(np.float32)
    m = (rng.random(R) < 0.4) if masked else None
    init = rng.normal(size=(P, Cc)).astype(np.float32) if acc else None
    rows = np.ones(R, dtype=bool) if m is None else (m == bool(want))
    ref = np.zeros((P, Cc))
    np.add.at(ref, np.arange(R)[rows] % P, x[rows].astype(np.float64))
    if acc:
        ref += init.astype(np.float64)
    xd, md = _in(x, ldx), (None if m is None else _d(m.astype(np.uint8) * 3))     # any non-zero byte is "set"

    def run():
        out, sc = _Out(P, Cc, init=init), _Scratch(lib)
        assert lib.uu3d_op_colsum(_p(xd), ldx, R, Cc, period, _p(md), want, out.ptr, acc, sc.ptr, sc.n, None) == OK
        res = out.result()
        sc.check()
        return (res,)
    _close(_twice(run)[0], ref, 2e-6)


@pytest.mark.parametrize("R,Cc,period", [(300, 32, 0), (21, 8, 7), (38, 8, 7)], ids=["colsum4", "period4", "generic_period"])
def test_colsum_workspace_refusal(lib, R, Cc, period):
    P = max(period, 1)
    assert _plan_colsum(Cc, R, Cc, period, False, P * Cc - 1)["kernel"] is None
    xd = torch.ones(R, Cc, device="cuda")
    out, sc = _Out(P, Cc), _Scratch(lib, P * Cc - 1)
    assert lib.uu3d_op_colsum(_p(xd), Cc, R, Cc, period, None, 0, out.ptr, 0, sc.ptr, sc.n, None) == WORKSPACE
    out.untouched(); sc.untouched()
    assert lib.uu3d_op_colsum(_p(xd), Cc - 1, R, Cc, period, None, 0, out.ptr, 0, sc.ptr, sc.n, None) == INVALID      # ldx < C
    out.untouched(); sc.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------
# row_stats + ln_bwd
# ---------------------------------------------------------------------------------------------------------------------------------
EPS = 1e-5
LN_KERNEL = {4: "wide<2>", 16: "wide<2>", 32: "narrow<8>", 48: "wide<2>", 64: "narrow<16>", 384: "wide<2>", 512: "wide<2>",
             516: "wide<4>", 1024: "wide<4>"}


def _ln_formula(x, dy, g, dt):
    """LayerNorm statistics and backward written out (the formulas at the head of the kernels in uu3d_bwd.h), every step in dtype dt."""
    x, dy, g = x.astype(dt), dy.astype(dt), g.astype(dt)
    mean = x.mean(-1, keepdims=True, dtype=dt)
    var = ((x - mean) ** 2).mean(-1, keepdims=True, dtype=dt)
    rstd = (1 / np.sqrt(var + dt(EPS))).astype(dt)
    xh = (x - mean) * rstd
    gg = dy * g
    dx = rstd * (gg - gg.mean(-1, keepdims=True, dtype=dt) - xh * (gg * xh).mean(-1, keepdims=True, dtype=dt))
    return dict(mean=mean[:, 0], rstd=rstd[:, 0], dx=dx, dg=(dy * xh).sum(0, dtype=dt), db=dy.sum(0, dtype=dt))


@functools.lru_cache(maxsize=None)
def _ln_problem(M, D, offset):
    rng = np.random.default_rng(100 * D + M)
    if offset:
        x = (100.0 + 1e-2 * rng.normal(size=(M, D))).astype(np.float32)      # mean 100, standard deviation 1e-2
    else:
        x = (rng.normal(size=(M, D)) * 2 + 0.5).astype(np.float32)
    dy = rng.normal(size=(M, D)).astype(np.float32)
    g = (1 + 0.1 * rng.normal(size=D)).astype(np.float32)
    ref = _ln_formula(x, dy, g, np.float64)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True); gt = torch.tensor(g, dtype=torch.float64, requires_grad=True)
    bt = torch.zeros(D, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.layer_norm(xt, (D,), gt, bt, EPS).backward(torch.tensor(dy, dtype=torch.float64))
    auto = dict(dx=xt.grad.numpy(), dg=gt.grad.numpy(), db=bt.grad.numpy())
    for k in auto:                                                             # the written-out formula IS autograd of LayerNorm
        assert np.abs(auto[k] - ref[k]).max() <= 1e-9 * max(np.abs(auto[k]).max(), 1e-30)
        ref[k] = auto[k]
    bars = {k: 5e-6 for k in ref}
    if offset:
        # Cancellation in x - mean: plain float32 is itself far from float64 here.  Bar = max(5e-6, 4 x the float32 formula's error), the
        # factor 4 covering another summation order.  Measured float32 error relative to max-abs -> bar, for M = 133:
        #   D = 32:  mean 9.5e-8, rstd 3.3e-7, dbeta 1.9e-7 -> 5e-6 each; dx 2.67e-4 -> 1.07e-3; dgamma 3.83e-4 -> 1.53e-3
        #   D = 384: mean 1.5e-7, rstd 1.0e-6, dbeta 3.7e-7 -> 5e-6 each; dx 8.33e-5 -> 3.33e-4; dgamma 5.31e-4 -> 2.12e-3
        f32 = _ln_formula(x, dy, g, np.float32)
        for k in ref:
            e32 = np.abs(f32[k].astype(np.float64) - ref[k]).max() / max(np.abs(ref[k]).max(), 1e-30)
            bars[k] = max(5e-6, 4 * e32)
            print(f"float32 error of {k}: {e32:.3e} -> bar {bars[k]:.3e}")
    return x, dy, g, ref, bars


def _run_ln(lib, M, D, pad, acc, scratch_floats=None, offset=False):
    x, dy, g, ref, bars = _ln_problem(M, D, offset)
    ld = D + pad
    xd, dyd, gd = _in(x, ld), _in(dy, ld), _d(g)
    init = np.random.default_rng(5).normal(size=(M, D)).astype(np.float32) if acc else None

    def run():
        stats, dx, dgb = _Out(M, 2), _Out(M, D, ld, init=init), _Out(2, D)       # dbeta right behind dgamma: one combine launch
        sc = _Scratch(lib, scratch_floats)
        assert lib.uu3d_op_row_stats(_p(xd), ld, D, M, EPS, stats.ptr, None) == OK
        st = stats.result()
        dbeta = C.c_void_p(dgb.ptr.value + 4 * D)
        assert lib.uu3d_op_ln_bwd(_p(xd), _p(dyd), stats.ptr, _p(gd), ld, D, M, dx.ptr, acc, dgb.ptr, dbeta, sc.ptr, sc.n, None) == OK
        sc.check()
        return st, dx.result(), dgb.result()
    st, dx, dgb = _twice(run)
    _close(st[:, 0], ref["mean"], bars["mean"])
    _close(st[:, 1], ref["rstd"], bars["rstd"])
    _close(dx.astype(np.float64) - (init.astype(np.float64) if acc else 0.0), ref["dx"], bars["dx"])
    _close(dgb[0], ref["dg"], bars["dg"])
    _close(dgb[1], ref["db"], bars["db"])
    return dx, dgb


@pytest.mark.parametrize("M", [1, 5, 133])
@pytest.mark.parametrize("D", sorted(LN_KERNEL))
def test_layernorm_kernels(lib, D, M):
    plan = _plan_ln_bwd(D, D, M, int(lib.uu3d_op_scratch_floats()))
    assert plan["kernel"] == LN_KERNEL[D] and plan["wgs"] == {1: 1, 5: 1}.get(M, plan["wgs"]), plan
    if M == 133:
        assert plan["wgs"] > 1, plan                               # more than one workgroup's partials to combine
    for acc in (0, 1):
        _run_ln(lib, M, D, 0, acc)


@pytest.mark.parametrize("D", [32, 64, 384, 1024])
def test_layernorm_strided(lib, D):
    assert _plan_ln_bwd(D, D + 4, 133, int(lib.uu3d_op_scratch_floats()))["kernel"] == LN_KERNEL[D]
    _run_ln(lib, 133, D, 4, 1)
    _run_ln(lib, 133, D, 4, 0)


@pytest.mark.parametrize("D", [32, 384])
def test_layernorm_offset_input(lib, D):
    """Rows with mean 100 and standard deviation 1e-2 (the bar: see _ln_problem)."""
    _run_ln(lib, 133, D, 0, 0, offset=True)


def test_layernorm_small_scratch_doubles_rows_per_wave(lib):
    M, D, small = 4096, 384, 100 * 768
    full = _plan_ln_bwd(D, D, M, int(lib.uu3d_op_scratch_floats()))
    plan = _plan_ln_bwd(D, D, M, small)
    assert (full["rows"], full["wgs"]) == (2, 512) and (plan["kernel"], plan["rows"], plan["wgs"]) == ("wide<2>", 16, 64), (full, plan)
    dx_full, _ = _run_ln(lib, M, D, 0, 0)
    dx_small, _ = _run_ln(lib, M, D, 0, 0, scratch_floats=small)
    assert np.array_equal(dx_full.view(np.int32), dx_small.view(np.int32))      # dx does not depend on the grouping of rows
    narrow = _plan_ln_bwd(32, 32, 4096, 3 * 64)
    assert (narrow["kernel"], narrow["first"], narrow["rows"], narrow["wgs"]) == ("narrow<8>", 4, 64, 2), narrow
    _run_ln(lib, 4096, 32, 0, 0, scratch_floats=3 * 64)
    one = _plan_ln_bwd(384, 384, 133, 2 * 384)                                 # exactly one workgroup's partials fit
    assert (one["rows"], one["wgs"]) == (64, 1), one
    _run_ln(lib, 133, 384, 0, 1, scratch_floats=2 * 384)


@pytest.mark.parametrize("D", [32, 384, 1024])
def test_layernorm_refusals(lib, D):
    M = 5
    xd = torch.ones(M, D + 8, device="cuda"); gd = torch.ones(D, device="cuda")

    def call(ld, D_, M_, scratch_floats):
        stats, dx, dgb = _Out(M, 2, init=np.ones((M, 2))), _Out(M, D, D + 8), _Out(2, D)
        sc = _Scratch(lib, scratch_floats)
        r = lib.uu3d_op_ln_bwd(_p(xd), _p(xd), stats.ptr, _p(gd), ld, D_, M_, dx.ptr, 0, dgb.ptr, C.c_void_p(dgb.ptr.value + 4 * D),
                               sc.ptr, sc.n, None)
        dx.untouched(); dgb.untouched(); sc.untouched()
        return r
    assert _plan_ln_bwd(D, D, M, 2 * D - 1)["kernel"] is None
    assert call(D, D, M, 2 * D - 1) == WORKSPACE
    assert call(D, D, M, 0) == WORKSPACE
    assert call(D, D, 0, 4096) == INVALID
    assert call(D, D, -1, 4096) == INVALID
    assert call(D - 4, D, M, 4096) == INVALID             # ld < D
    assert call(D + 1, D, M, 4096) == INVALID             # ld % 4 != 0
    assert call(D, 0, M, 4096) == INVALID
    assert call(D + 8, D + 2, M, 4096) == INVALID         # D % 4 != 0
    stats = _Out(M, 2)
    for ld, D_, M_ in [(D, D, 0), (D - 4, D, M), (D + 1, D, M), (D, 0, M), (2048, 1028, M)]:
        assert lib.uu3d_op_row_stats(_p(xd), ld, D_, M_, EPS, stats.ptr, None) == INVALID
        stats.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------------------
def _attn_torch(qkv, dout, m, B, L, H, dh, dt, collapse):
    """out and d qkv of softmax(q k^T / sqrt(dh) + (1 - mask) * -1e9) v in dtype dt.  collapse: sequences (all keys masked) whose logits
    are replaced by equal values with the gradient kept -- what adding -1e9 does to them in float32."""
    D = H * dh
    t = torch.tensor(qkv, dtype=dt, requires_grad=True)
    q, k, v = [t[:, i * D:(i + 1) * D].reshape(B, L, H, dh).permute(0, 2, 1, 3) for i in range(3)]
    logits = torch.matmul(q, k.transpose(-1, -2)) / torch.sqrt(torch.tensor(float(dh), dtype=dt))
    if m is not None:
        if collapse is not None and collapse.any():
            keep = torch.tensor(~collapse, dtype=dt)[:, None, None, None]
            logits = logits - (1 - keep) * logits.detach()
        logits = logits + (1.0 - torch.tensor(m.astype(np.float64), dtype=dt))[:, None, None, :] * -1e9
    o = torch.matmul(torch.softmax(logits, -1), v).permute(0, 2, 1, 3).reshape(B * L, D)
    o.backward(torch.tensor(dout, dtype=dt))
    return o.detach().numpy().astype(np.float64), t.grad.numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def _attn_problem(B, L, H, dh, masked, scale):
    """Masked problems: sequence 0 has every key masked, sequence 1 exactly one key unmasked, the others about half of them."""
    rng = np.random.default_rng(10000 * dh + 100 * L + 10 * B + H + (5 if masked else 0))
    D = H * dh
    qkv = rng.normal(size=(B * L, 3 * D)).astype(np.float32)
    qkv[:, :2 * D] *= scale
    dout = rng.normal(size=(B * L, D)).astype(np.float32)
    m = None
    if masked:
        m = rng.random((B, L)) < 0.5
        m[:, 0] |= ~m.any(1)
        if scale == 1.0:                                   # (with large logits -1e9 no longer collapses a fully masked row)
            m[0] = False
        if B > 1:
            m[1] = False; m[1, L // 2] = True
    dead = None if m is None else ~m.any(1)
    out, grad = _attn_torch(qkv, dout, m, B, L, H, dh, torch.float64, dead)
    bars = [5e-6, 2e-5]
    if dead is not None and dead.any():
        # float64 autograd keeps the logit differences of a fully masked sequence; its dQ and dK rows come from float32 autograd of the formula
        _, g32 = _attn_torch(qkv, dout, m, B, L, H, dh, torch.float32, None)
        for b in np.nonzero(dead)[0]:
            grad[b * L:(b + 1) * L, :2 * D] = g32[b * L:(b + 1) * L, :2 * D]
            mean_v = qkv[b * L:(b + 1) * L, 2 * D:].astype(np.float64).mean(0)
            assert np.abs(out[b * L:(b + 1) * L] - mean_v).max() < 1e-12          # the plain mean of V
    if masked and B > 1:
        assert np.array_equal(out[L:2 * L], np.broadcast_to(qkv[L + L // 2, 2 * D:].astype(np.float64), (L, D)))   # that key's V row
    if scale != 1.0:
        # Logits of size ~ scale^2: a float32 rounding of a logit moves its weight by ~ 60 * 6e-8.  Bar = max(project bar, 4 x the error of
        # the float32 formula on the CPU).  Measured float32 error relative to max-abs, forward / backward -> bars (B = 3, H = 8, dh = 48):
        #   L = 33: 8.0e-6 / 1.03e-5 -> 3.2e-5 / 4.1e-5;  masked 6.7e-6 / 6.4e-6 -> 2.7e-5 / 2.6e-5
        #   L = 71: 8.7e-6 / 8.3e-6 -> 3.5e-5 / 3.3e-5;   masked 1.08e-5 / 4.4e-6 -> 4.3e-5 / 2.0e-5
        o32, g32 = _attn_torch(qkv, dout, m, B, L, H, dh, torch.float32, None)
        e = [np.abs(o32 - out).max() / np.abs(out).max(), np.abs(g32 - grad).max() / np.abs(grad).max()]
        bars = [max(5e-6, 4 * e[0]), max(2e-5, 4 * e[1])]
        print(f"float32 error forward {e[0]:.3e} backward {e[1]:.3e} -> bars {bars[0]:.3e} {bars[1]:.3e}")
    return qkv, dout, m, out, grad, bars


def _run_attn(lib, B, L, H, dh, masked, pad=0, scale=1.0, backward=True):
    qkv, dout, m, out_ref, grad_ref, bars = _attn_problem(B, L, H, dh, masked, scale)
    D = H * dh
    ld, ldo = 3 * D + pad, D + pad
    qd, dod = _in(qkv, ld), _in(dout, ldo)
    md = None if m is None else _d(m.astype(np.uint8) * 255)

    def run():
        out = _Out(B * L, D, ldo)
        assert lib.uu3d_op_attn_fwd(_p(qd), ld, D, B, L, H, dh, _p(md), out.ptr, ldo, None) == OK
        res = (out.result(),)
        if backward:
            dqkv = _Out(B * L, 3 * D, ld)
            assert lib.uu3d_op_attn_bwd(_p(qd), _p(dod), ld, D, B, L, H, dh, _p(md), dqkv.ptr, ldo, None) == OK
            res += (dqkv.result(),)
        return res
    res = _twice(run)
    _close(res[0], out_ref, bars[0])
    if backward:
        _close(res[1], grad_ref, bars[1])
    return res


DH4_B = {1: 3, 5: 3, 17: 3, 33: 4, 96: 3}          # B * 8 heads is no multiple of the 128 / L pairs a workgroup packs


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("L", sorted(DH4_B))
def test_attention_head_dim_4(lib, monkeypatch, L, masked):
    monkeypatch.delenv("UU3D_ATTN_BWD_GENERIC", raising=False)
    B, H = DH4_B[L], 8
    plan = _plan_attn(True, L, 4, masked)
    assert plan["kernel"] == ("small_bwd<17>" if (L == 17 and not masked) else "generic_bwd<4>"), plan
    assert plan["pack"] == 128 // L and (plan["pack"] == 1 or (B * H) % plan["pack"] != 0), plan
    _run_attn(lib, B, L, H, 4, masked, pad=4 if L in (17, 33) else 0)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
def test_attention_head_dim_4_forward_128(lib, masked):
    assert _plan_attn(False, 128, 4, masked) == dict(kernel="generic_fwd<4>", pack=1)
    _run_attn(lib, 3, 128, 8, 4, masked, backward=False)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("L,NT", [(1, 1), (16, 1), (17, 2), (33, 3), (48, 3), (64, 4), (65, 5), (96, 6)])
def test_attention_head_dim_48_mfma(lib, monkeypatch, L, NT, masked):
    monkeypatch.delenv("UU3D_ATTN_BWD_GENERIC", raising=False)
    assert _plan_attn(True, L, 48, masked)["kernel"] == "mfma<%d,48>" % NT
    _run_attn(lib, 3, L, 8, 48, masked, pad=4 if masked else 0)          # strided once per NT


@pytest.mark.parametrize("H,L", [(1, 33), (3, 64)])
def test_attention_head_dim_48_head_counts(lib, monkeypatch, H, L):
    monkeypatch.delenv("UU3D_ATTN_BWD_GENERIC", raising=False)
    _run_attn(lib, 3, L, H, 48, True, pad=4)


@pytest.mark.parametrize("L", [33, 71])
def test_attention_head_dim_48_generic_backward(lib, monkeypatch, L):
    """attn_generic_bwd_kernel<48> behind UU3D_ATTN_BWD_GENERIC, which the ops ABI reads at every call (read_switches() in
    uu3d_op_attn_bwd): against float64 and against the MFMA kernel."""
    monkeypatch.delenv("UU3D_ATTN_BWD_GENERIC", raising=False)
    assert _plan_attn(True, L, 48, True)["kernel"] == "mfma<%d,48>" % _cdiv(L, 16)
    _, mfma = _run_attn(lib, 3, L, 8, 48, True, pad=4)
    monkeypatch.setenv("UU3D_ATTN_BWD_GENERIC", "1")
    assert _plan_attn(True, L, 48, True, generic=True)["kernel"] == "generic_bwd<48>"
    _, gen = _run_attn(lib, 3, L, 8, 48, True, pad=4)
    _run_attn(lib, 3, L, 8, 48, False)
    _close(gen, mfma, 2e-5)
    assert not np.array_equal(gen.view(np.int32), mfma.view(np.int32))          # the switch took: another kernel, another rounding
    assert _plan_attn(True, 17, 4, False, generic=True)["kernel"] == "generic_bwd<4>"      # and keeps L = 17 off the unrolled kernel
    _run_attn(lib, 3, 17, 8, 4, False)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("L", [33, 71])
def test_attention_large_logits(lib, monkeypatch, L, masked):
    """q and k scaled by 8: logits of size ~ 60, softmax rows close to one-hot (the bars: see _attn_problem)."""
    monkeypatch.delenv("UU3D_ATTN_BWD_GENERIC", raising=False)
    _run_attn(lib, 3, L, 8, 48, masked, scale=8.0)


def test_attention_refusals(lib):
    B, L, H, dh = 2, 5, 8, 48
    D = H * dh
    qd = torch.ones(B * 129, 3 * D + 4, device="cuda"); dod = torch.ones(B * 129, D + 4, device="cuda")
    out, dqkv = _Out(B * 129, D, D + 4), _Out(B * 129, 3 * D, 3 * D + 4)

    def fwd(ld=3 * D, D_=D, B_=B, L_=L, H_=H, dh_=dh, ldo=D):
        r = lib.uu3d_op_attn_fwd(_p(qd), ld, D_, B_, L_, H_, dh_, None, out.ptr, ldo, None)
        out.untouched()
        return r

    def bwd(ld=3 * D, D_=D, B_=B, L_=L, H_=H, dh_=dh, ldo=D):
        r = lib.uu3d_op_attn_bwd(_p(qd), _p(dod), ld, D_, B_, L_, H_, dh_, None, dqkv.ptr, ldo, None)
        dqkv.untouched()
        return r
    for f in (fwd, bwd):
        assert f(D_=D - 48) == INVALID                     # D != H * head_dim
        assert f(H_=7) == INVALID
        assert f(dh_=4) == INVALID
        assert f(dh_=16) == INVALID
        assert f(ld=3 * D - 4) == INVALID                  # ld < 3 D
        assert f(ld=3 * D + 2) == INVALID                  # rows move as 16-byte pieces
        assert f(ldo=D - 4) == INVALID
        assert f(ldo=D + 1) == INVALID
        assert f(B_=0) == INVALID
        assert f(H_=0, D_=0) == INVALID
        assert f(L_=0) == INVALID
    assert bwd(L_=97) == UNSUPPORTED
    assert fwd(L_=129) == UNSUPPORTED
    assert bwd(L_=129) == UNSUPPORTED
