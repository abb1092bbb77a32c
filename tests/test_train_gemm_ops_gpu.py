"""The training step's GEMM forms, operator by operator (include/uu3d_ops.h, TRAINING GEMMS), against float64 references built from the
same float32 inputs (tests/train_gemm_util.py; tests/test_train_gemm_ops_cpu.py holds those references to torch float64 autograd).  Every
entry launches through the step's own host dispatch (launch_gemm, launch_gemm_tn, launch_colsum, launch_ln_bwd_rows / _combine), on
operands made by repack_kernel itself (uu3d_op_train_pack).  The harness is that of tests/test_bwd_ops_edges_gpu.py: NaN in the padding
columns of the inputs, NaN-filled outputs with padding columns and a sentinel row before and after, a guard behind slab and scratch, every
element inside finite, two launches compared bitwise, and each case asserts its branch from the restated plan (tests/bwd_plan_util.py).

Branch census (loader x epilogue; each at f32 = gemm_f32_kernel<64, 64> and f16x3 = gemm_h3_kernel<1, 1, ., ., DEEP 1> unless noted; "split":
the kernel runs with EpSlab and the epilogue inside splitk_reduce_kernel<EP>), by test id of test_train_dense:
  ALoadGelu x EpBiasResGate        unsplit gelu-*-K64, gelu-gate-K72 (K tail), split gelu-*-K256 (gate / gate + Dropout / no gate); DEEP 0 + EpSlab: gelu-gate-wide
  ALoadPlain x EpBiasResGate       unsplit plain-gate-out2-K96, split plain-gate-out2-K288 (out2 + pe2[row % period]), plain-gate-N100-K288
  ALoadLayerNorm x EpBias / Relu   unsplit ln-*-K64, ln-bias-K72 (K tail), split ln-*-K256; DEEP 0 + EpSlab: ln-bias-wide
  ALoadConv3 x EpConvResidual      unsplit conv3-<geometry>-C32 (with pe_next), split conv3-<geometry>-C96 (with Dropout), gate always
  ALoadConvT x EpReluMask          unsplit convt-<geometry>-C32-*, split convt-<geometry>-C96-* (scale 1 and 1 / 0.9); DEEP 0 + EpSlab: convt-wide
  ALoadPlain x EpGeluGrad, x EpReluMask, x EpStore (kind-4 planes)   unsplit plain-*-K64, plain-store-M85-K72 (K tail), split plain-*-K288, M = 85 and 133
  ALoadPlain x EpAdd               unsplit plain-add-M*-head (51 of 64 columns), split plain-add-M85-K288
test_train_wgrad (launch_gemm_tn):
  TnLoadLayerNorm x EpStore3       gemm_tn_kernel ln-store3-d32-R70 / -R600 (split, reduce); gemm_tn_h3_kernel d128 (segments on tile edges) and
                                   d160 (a segment boundary inside a tile), R70 unsplit, R600 split; reduced slab: ln-store3-d128-small-slab
  TnLoadLayerNorm x EpStore        ln-store-P32-Q64 (f32 kernel), ln-store-P128-Q256 (h3, split), -f32 (h3 flag off)
  TnLoadGelu x EpStore             gelu-store-R85 (unsplit), -R680 (reduce), -skinny (splitk_reduce16_kernel), -small-slab
  TnLoadConv3 x EpStore            conv3-<geometry>-C32 (f32 kernel), -C64 (h3 kernel), conv3-s3p0_L11-C64-split
test_colsum3 (colsum4_kernel + reduce_partials_kernel into ReduceOut), test_ln_bwd_ex (ln_bwd_narrow_kernel<8> / ln_bwd_kernel<2> with res and
LnBwdGated), test_identity_bwd, test_scale_rows, test_pack (repack_kernel kinds 1, 4, 5 with the planes), the refusals.

Bounds (tests/train_gemm_util.py: nn_bound, tn_problem; none from what these kernels measure): exact f32 2e-6 max|acc|; f16x3 through launch_gemm
2e-5 at unit scale (max|acc| < 8 asserted, K <= 384); times the largest factor a multiplying epilogue applies, + 2^-23 max|ref| per further
float32 operation; GELU forms + twice the deviation of a torch-float32 restatement; LayerNorm loaders + 5e-6 max|ref|; launch_gemm_tn 2e-6 max|ref|
on gradient-sized B rows; every allowance <= 1e-4.  Where the reference is exactly zero (gate 0, H <= 0, dropped elements, rows not selected or
masked) the result is compared for equality.
Measured on an MI355X (largest max-abs error of a kernel form, with that case's bound): gemm_f32 unsplit 1.6e-6 of 1.7e-5, split 2.4e-6 of
1.8e-5; gemm_h3 DEEP unsplit 8.4e-7 of 3.5e-5, DEEP split 9.5e-7 of 3.4e-5, not DEEP split 1.1e-6 of 2.8e-5; gemm_tn_kernel unsplit 3.2e-6 of
2.1e-5, reduce 9.6e-6 of 4.8e-5, reduce16 1.8e-5 of 1.2e-4 (the three largest: the TnLoadGelu cases, results of scale 10 .. 60); gemm_tn_h3_kernel
unsplit 3.8e-7 of 3.6e-6, split 1.6e-6 of 2.6e-5; pack: hi + lo / 2048 reproduces the operand to 1.2e-7.  209 tests, 4.0 s for the whole file.
Sensitivity, on scratch builds with one value changed (no address moves): EpReluMask without `* scale` fails the 22 "-scaled" ReluMask cases; gelu_grad
returning gelu the 8 plain-gelugrad cases; `p.x >= 0.f` the 42 ReluMask cases (exact zeros); EpBiasResGate without `/ keep` the 18 gated cases;
identity_bwd without `q % stride == 0` the three strided geometries (stride 1 is a copy either way); TnLoadLayerNorm without its mean term the 10
TnLoadLayerNorm cases.  `seg - 1` in EpStore3's middle segment would store one element past the middle tensor and was not run: each segment sits in
its own sentinel-framed buffer, where a shift by one column compares every element with its neighbour and writes the row behind the result."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests import train_gemm_util as U                                                                     # noqa: E402
from tests.bwd_plan_util import _plan_gemm_tn, _plan_colsum, _plan_ln_bwd                                   # noqa: E402
from tests.test_bwd_ops_edges_gpu import (_Out, _Scratch, _in, _d, _p, _close, _twice, _bits, lib, NAN, GUARD,   # noqa: E402,F401
                                          OK, INVALID, WORKSPACE, EPS)


def _slab(n):
    t = torch.full((n + GUARD,), NAN, device="cuda")
    return t


_ops = {}


def _operand(lib, w, kind, Cc=0):
    """The block uu3d_op_train_pack makes from w on the device (cached per weight)."""
    key = (w.ctypes.data, kind, Cc)
    if key not in _ops:
        K, N = w.shape
        nbytes = int(lib.uu3d_op_train_operand_bytes(kind, K, N, Cc))
        rows, ld = U.operand_dims(kind, K, N, Cc)
        assert nbytes == 8 * rows * ld
        op = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        wd = _d(w)
        assert lib.uu3d_op_train_pack(_p(wd), kind, K, N, Cc, _p(op), None) == OK
        assert bool((op[nbytes:] == 0xA5).all()), "the pack wrote past the block"
        _ops[key] = (op, w)
    return _ops[key][0]


# ---------------------------------------------------------------------------------------------------------------------------------
# pack
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,K,N,Cc", [(1, 51, 40, 0), (4, 51, 40, 0), (5, 72, 40, 24), (1, 33, 129, 0), (4, 65, 33, 0)])
def test_pack(lib, kind, K, N, Cc):
    rng = np.random.default_rng(kind * 1000 + K + N)
    w = (np.exp2(rng.uniform(-6, 1, size=(K, N))) * rng.choice([-1.0, 1.0], size=(K, N))).astype(np.float32)    # 2^-6 <= |w| <= 2: no lo half is subnormal
    rows, ld = U.operand_dims(kind, K, N, Cc)
    n = rows * ld
    raw = _operand(lib, w, kind, Cc)[:8 * n].cpu().numpy()
    f32 = raw[:4 * n].view(np.float32).reshape(rows, ld)
    hi = raw[4 * n:6 * n].view(np.float16).reshape(rows, ld).astype(np.float64)
    lo = raw[6 * n:].view(np.float16).reshape(rows, ld).astype(np.float64)
    want = U.pack_ref(w, kind, Cc)
    assert np.array_equal(f32.view(np.int32), want.view(np.int32)), "the f32 operand is not the formula of repack_kernel bit for bit (padding: +0.0)"
    pad = want == 0
    assert pad.sum() == n - K * N and not hi[pad].any() and not lo[pad].any(), "padding of the planes is not zero"
    err = np.abs(hi + lo / 2048.0 - want.astype(np.float64)).max()
    print(f"pack kind {kind}: planes reproduce the operand to {err:.3e} (step 2^-20 = {2.0 ** -20:.3e} at |w| <= 2: {2.0 ** -19:.3e})")
    assert err <= 2.0 ** -20 * 2.0
    assert lib.uu3d_op_train_operand_bytes(kind, 0, N, Cc) == 0 and lib.uu3d_op_train_operand_bytes(2, K, N, Cc) == 0
    assert lib.uu3d_op_train_operand_bytes(5, K, N, Cc + 1) == 0
    assert lib.uu3d_op_train_pack(None, kind, K, N, Cc, _p(raw_dev := torch.zeros(8, device="cuda")), None) == INVALID
    assert lib.uu3d_op_train_pack(_p(raw_dev), 3, K, N, Cc, _p(raw_dev), None) == INVALID and not raw_dev.any()


# ---------------------------------------------------------------------------------------------------------------------------------
# launch_gemm
# ---------------------------------------------------------------------------------------------------------------------------------
class DenseRun:
    """One call of uu3d_op_train_dense on NaN-padded inputs and NaN-filled, sentinel-framed outputs."""

    def __init__(self, lib, c, prec, slab_floats=U.FULL_SLAB, **override):
        from uplift_upsample_3dhpe_amd._capi import Uu3dTrainDenseArgs
        p = U.nn_problem(c.name)
        o, M, N, K, ld = c.opt, c.M, c.N, c.K, p["ld"]
        a = Uu3dTrainDenseArgs()
        conv = c.src in (U.TA_CONV3, U.TA_CONVT)
        lda = p["a"].shape[1] + (0 if conv else c.pad)
        self.keep = [_in(p["a"], lda)]
        a.a_dev = self.keep[0].data_ptr()
        if c.src == U.TA_LN:
            st = torch.empty(M, 2, device="cuda")
            assert lib.uu3d_op_row_stats(_p(self.keep[0]), lda, K, M, EPS, _p(st), None) == OK
            g, b = _d(p["ln"][0]), _d(p["ln"][1])
            self.keep += [st, g, b]
            a.ln_stats_dev, a.ln_gamma_dev, a.ln_beta_dev = st.data_ptr(), g.data_ptr(), b.data_ptr()
        kind, Kw, Nw, Cc = p["pack"]
        a.operand_dev = _operand(lib, p["w"], kind, Cc).data_ptr()
        bias = _d(p["bias"]); self.keep.append(bias); a.bias_dev = bias.data_ptr()
        self.out = _Out(M, N, ld, init=p["init"])
        a.out_dev = self.out.ptr.value
        self.out2 = None
        if p["ref2"] is not None:
            self.out2 = _Out(M, N, ld); a.out2_dev = self.out2.ptr.value
        if p["aux"] is not None:
            aux = _in(p["aux"], ld); self.keep.append(aux); a.aux_dev = aux.data_ptr()
        if p["pe"] is not None:
            pe = _in(p["pe"], ld); self.keep.append(pe); a.pe_dev = pe.data_ptr()
        if p["gate"] is not None:
            gate = _d(p["gate"]); self.keep.append(gate); a.gate_dev = gate.data_ptr()
        self.slab_floats = slab_floats
        self.slab = _slab(slab_floats)
        a.slab_dev, a.slab_floats = self.slab.data_ptr(), slab_floats
        a.drop_seed, a.drop_site, a.drop_rate = U.SEED, 77, o.get("drop", 0.0)
        a.a_source, a.epilogue, a.precision, a.operand_kind = c.src, c.ep, prec, c.kind
        a.M, a.N, a.K, a.lda, a.ldo = M, N, K, lda, ld
        if conv:
            s, pl, Li, Lo = c.geom
            a.conv_C, a.conv_stride, a.conv_pad_left, a.conv_L_in, a.conv_L_out = p["a"].shape[1], s, pl, Li, Lo
        a.rps, a.period, a.keep, a.scale = o.get("rps", 1), o.get("period", 1), o.get("keep", 1.0), o.get("scale", 1.0)
        for k, v in override.items():
            setattr(a, k, v)
        self.args = a
        self.status = lib.uu3d_op_train_dense(C.byref(a), None)
        torch.cuda.synchronize()

    def results(self, slices):
        used = slices * self.args.M * ((self.args.N + 3) // 4 * 4) if slices > 1 else 0
        assert bool(torch.isnan(self.slab[used:]).all()), "the slab was written past its slices (or by an unsplit launch)"
        res = (self.out.result(),)
        if self.out2 is not None:
            res += (self.out2.result(),)
        return res

    def untouched(self):
        self.out.untouched()
        if self.out2 is not None:
            self.out2.untouched()
        assert bool(torch.isnan(self.slab).all()), "a refused call wrote the slab"


@pytest.mark.parametrize("prec", [U.PREC_F32, U.PREC_H3], ids=["f32", "h3"])
@pytest.mark.parametrize("name", [c.name for c in U.NN_CASES])
def test_train_dense(lib, name, prec):
    c = U.NN_BY_NAME[name]
    p = U.nn_problem(name)
    plan = U.plan_nn(c.M, c.N, c.K, U.FULL_SLAB, prec == U.PREC_H3)
    assert plan["split"] == (c.K >= 256), plan                     # unsplit below 8 k-tiles, EpSlab + splitk_reduce_kernel<EP> from there
    if prec == U.PREC_H3:
        assert plan["deep"] == c.deep, plan
    bound = U.nn_bound(c, p, prec)

    def run():
        r = DenseRun(lib, c, prec)
        assert r.status == OK
        return r.results(plan["slices"])
    res = _twice(run)
    got = res[0].astype(np.float64)
    err = float(np.abs(got - p["ref"]).max())
    err2 = float(np.abs(res[1].astype(np.float64) - p["ref2"]).max()) if p["ref2"] is not None else 0.0
    print(f"TRAIN-NN {name} {plan['kernel']} slices={plan['slices']} deep={plan['deep']}: max-abs {max(err, err2):.3e} bound {bound:.3e} (scale {np.abs(p['ref']).max():.2f})")
    assert err <= bound and err2 <= bound
    z = p["branch_zero"]
    if z is not None and c.ep == U.EP_RELU_MASK:
        assert z.any() and np.array_equal(res[0][z].view(np.int32), np.zeros(int(z.sum()), np.int32)), "H <= 0 must give exactly +0.0"
    elif z is not None and "identity" in p:
        # a zero branch (gate 0 / dropped) leaves the identity stream exactly: xin, or float32(xin + pe) where a positional encoding is added
        assert z.any() == bool(c.opt.get("gate") or c.opt.get("drop"))
        assert np.array_equal(res[0][z].view(np.int32), p["identity"][z].view(np.int32)), "a zero branch must leave the identity stream exactly"
        if p["ref2"] is not None:
            assert np.array_equal(res[1][z].view(np.int32), p["identity2"][z].view(np.int32)), "a zero branch must leave identity + pe in the second stream exactly"
    if prec == U.PREC_F32 and plan["split"]:                       # the unsplit form of the same case: same bound, another order of summation
        u = DenseRun(lib, c, prec, slab_floats=0)
        assert u.status == OK
        assert float(np.abs(u.results(1)[0].astype(np.float64) - p["ref"]).max()) <= bound


DENSE_REFUSED = [
    ("null a", "gelu-gate-K64", dict(a_dev=None)),
    ("null operand", "gelu-gate-K64", dict(operand_dev=None)),
    ("null residual", "gelu-gate-K64", dict(aux_dev=None)),
    ("null bias", "ln-bias-K64", dict(bias_dev=None)),
    ("null stats", "ln-bias-K64", dict(ln_stats_dev=None)),
    ("null H", "plain-relumask-M85-K64", dict(aux_dev=None)),
    ("lda not x4", "gelu-gate-K64", dict(lda=70)),
    ("lda < K", "gelu-gate-K64", dict(lda=60)),
    ("ldo < N", "gelu-gate-K64", dict(ldo=28)),
    ("K not x4", "plain-store-M85-K64", dict(K=62)),
    ("gelu loader with EpStore", "gelu-gate-K64", dict(epilogue=U.EP_STORE)),
    ("gelu loader on a kind-4 operand", "gelu-gate-K64", dict(operand_kind=4)),
    ("LayerNorm loader with EpAdd", "ln-bias-K64", dict(epilogue=U.EP_ADD)),
    ("conv-transpose with EpGeluGrad", "convt-s2p1-C32-unit", dict(epilogue=U.EP_GELU_GRAD)),
    ("conv3 with EpBias", "conv3-s2p1-C32", dict(epilogue=U.EP_BIAS)),
    ("plain rows with EpBias", "plain-store-M85-K64", dict(epilogue=U.EP_BIAS)),
    ("unknown source", "plain-store-M85-K64", dict(a_source=5)),
    ("unknown precision", "plain-store-M85-K64", dict(precision=2)),
    ("K != 3 C", "convt-s2p1-C32-unit", dict(K=92)),
    ("M not a multiple of L_in", "convt-s2p1-C32-unit", dict(M=26)),
    ("identity row past L_in", "conv3-s3p0_L9-C32", dict(conv_L_in=7)),
    ("gate with keep 0", "gelu-gate-K64", dict(keep=0.0)),
    ("gate with rps 0", "gelu-gate-K64", dict(rps=0)),
    ("drop rate 1", "gelu-gate-drop-K64", dict(drop_rate=1.0)),
    ("out2 without pe", "plain-gate-out2-K96", dict(pe_dev=None)),
    ("slab capacity without a slab", "gelu-gate-K256", dict(slab_dev=None)),
    ("M = 0", "plain-store-M85-K64", dict(M=0)),
]


@pytest.mark.parametrize("why,name,override", DENSE_REFUSED, ids=[r[0] for r in DENSE_REFUSED])
def test_train_dense_refusals(lib, why, name, override):
    r = DenseRun(lib, U.NN_BY_NAME[name], U.PREC_H3, **override)
    assert r.status == INVALID, why
    r.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------
# launch_gemm_tn
# ---------------------------------------------------------------------------------------------------------------------------------
class WgradRun:
    def __init__(self, lib, c, **override):
        from uplift_upsample_3dhpe_amd._capi import Uu3dTrainWgradArgs
        p = U.tn_problem(c.name)
        R, P, Q = c.R, c.P, c.Q
        a = Uu3dTrainWgradArgs()
        conv = c.src == U.TA_CONV3
        lda = p["a"].shape[1] + (0 if conv else c.pad)
        ldb = Q + 2 * c.pad
        self.keep = [_in(p["a"], lda), _in(p["b"], ldb)]
        a.a_dev, a.b_dev = self.keep[0].data_ptr(), self.keep[1].data_ptr()
        if c.src == U.TA_LN:
            st = torch.empty(R, 2, device="cuda")
            assert lib.uu3d_op_row_stats(_p(self.keep[0]), lda, P, R, EPS, _p(st), None) == OK
            g, b = _d(p["ln"][0]), _d(p["ln"][1])
            self.keep += [st, g, b]
            a.ln_stats_dev, a.ln_gamma_dev, a.ln_beta_dev = st.data_ptr(), g.data_ptr(), b.data_ptr()
        if c.ep == U.WEP_STORE3:
            self.outs = [_Out(P, Q // 3) for _ in range(3)]           # each segment in its own sentinel-framed buffer
            a.out_dev, a.out1_dev, a.out2_dev = [o.ptr.value for o in self.outs]
        else:
            self.outs = [_Out(P, Q, Q + c.pad)]
            a.out_dev = self.outs[0].ptr.value
        self.slab_floats = c.slab if c.slab is not None else U.FULL_SLAB
        self.slab = _slab(self.slab_floats)
        a.slab_dev, a.slab_floats = self.slab.data_ptr(), self.slab_floats
        a.a_source, a.epilogue, a.h3 = c.src, c.ep, c.h3
        a.R, a.P, a.Q, a.lda, a.ldb, a.ldo = R, P, Q, lda, ldb, Q + c.pad
        if conv:
            s, pl, Li, Lo = c.geom
            a.conv_C, a.conv_stride, a.conv_pad_left, a.conv_L_in, a.conv_L_out = P // 3, s, pl, Li, Lo
        for k, v in override.items():
            setattr(a, k, v)
        self.status = lib.uu3d_op_train_wgrad(C.byref(a), None)
        torch.cuda.synchronize()

    def result(self):
        assert bool(torch.isnan(self.slab[self.slab_floats:]).all()), "the slab was written past its capacity"
        return (np.concatenate([o.result() for o in self.outs], axis=1),)

    def untouched(self):
        for o in self.outs:
            o.untouched()
        assert bool(torch.isnan(self.slab).all()), "a refused call wrote the slab"


@pytest.mark.parametrize("name", [c.name for c in U.TN_CASES])
def test_train_wgrad(lib, monkeypatch, name):
    monkeypatch.delenv("UU3D_TNH_WGS", raising=False)
    c = U.TN_BY_NAME[name]
    p = U.tn_problem(name)
    plan = _plan_gemm_tn(c.R, c.P, c.Q, c.slab if c.slab is not None else U.FULL_SLAB, bool(c.h3))
    assert {k: plan[k] for k in c.expect} == c.expect, plan

    def run():
        r = WgradRun(lib, c)
        assert r.status == OK
        return r.result()
    got = _twice(run)[0].astype(np.float64)
    err = float(np.abs(got - p["ref"]).max())
    print(f"TRAIN-TN {name} {plan['kernel']} slices={plan['slices']} combine={plan['combine']}: max-abs {err:.3e} bound {p['bar']:.3e} (scale {np.abs(p['ref']).max():.2e})")
    assert err <= p["bar"]


WGRAD_REFUSED = [
    ("null a", dict(a_dev=None)), ("null b", dict(b_dev=None)), ("null second output", dict(out1_dev=None)), ("null stats", dict(ln_stats_dev=None)),
    ("lda not x4", dict(lda=38)), ("ldb < Q", dict(ldb=92)), ("P not x4", dict(P=30)), ("Q % 3 != 0", dict(Q=92)),
    ("EpStore3 from GELU rows", dict(a_source=U.TA_GELU)), ("conv-transpose loader", dict(a_source=U.TA_CONVT)), ("unknown epilogue", dict(epilogue=2)),
    ("slab capacity without a slab", dict(slab_dev=None)), ("R = 0", dict(R=0)),
]


@pytest.mark.parametrize("why,override", WGRAD_REFUSED, ids=[r[0] for r in WGRAD_REFUSED])
def test_train_wgrad_refusals(lib, why, override):
    r = WgradRun(lib, U.TN_BY_NAME["ln-store3-d32-R70"], **override)
    assert r.status == INVALID, why
    r.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------
# colsum3
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [85, 4000])
@pytest.mark.parametrize("seg", [32, 160])
def test_colsum3(lib, seg, R):
    Cc, ldx = 3 * seg, 3 * seg + 4
    plan = _plan_colsum(ldx, R, Cc, 0, False, int(lib.uu3d_op_scratch_floats()))
    assert plan["kernel"] == "colsum4" and (plan["slices"] > 1) == (R == 4000), plan
    rng = np.random.default_rng(seg + R)
    x = rng.normal(size=(R, Cc)).astype(np.float32)
    ref = x.astype(np.float64).sum(0)
    xd = _in(x, ldx)

    def run():
        outs, sc = [_Out(1, seg) for _ in range(3)], _Scratch(lib)
        assert lib.uu3d_op_colsum3(_p(xd), ldx, R, seg, outs[0].ptr, outs[1].ptr, outs[2].ptr, 0, sc.ptr, sc.n, None) == OK
        sc.check()
        return (np.concatenate([o.result()[0] for o in outs]),)
    _close(_twice(run)[0], ref, 2e-6)
    outs, sc = [_Out(1, seg) for _ in range(3)], _Scratch(lib, Cc - 1)
    assert lib.uu3d_op_colsum3(_p(xd), ldx, R, seg, outs[0].ptr, outs[1].ptr, outs[2].ptr, 0, sc.ptr, sc.n, None) == WORKSPACE
    assert lib.uu3d_op_colsum3(_p(xd), Cc - 4, R, seg, outs[0].ptr, outs[1].ptr, outs[2].ptr, 0, sc.ptr, sc.n, None) == INVALID
    assert lib.uu3d_op_colsum3(_p(xd), ldx, R, seg, outs[0].ptr, None, outs[2].ptr, 0, sc.ptr, sc.n, None) == INVALID
    for o in outs:
        o.untouched()
    sc.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------
# ln_bwd_ex
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gated", [False, True], ids=["nogate", "gate"])
@pytest.mark.parametrize("res", ["none", "distinct", "inplace"])
@pytest.mark.parametrize("D", [32, 384])
def test_ln_bwd_ex(lib, D, res, gated):
    from tests.test_bwd_ops_edges_gpu import _ln_problem
    M, rps, keep, ld = 85, 17, 0.9, D + 4
    assert _plan_ln_bwd(D, ld, M, int(lib.uu3d_op_scratch_floats()))["kernel"] == ("narrow<8>" if D == 32 else "wide<2>")
    x, dy, g, ref, bars = _ln_problem(M, D, False)
    rng = np.random.default_rng(D + 3)
    r32 = rng.normal(size=(M, D)).astype(np.float32)
    gate = np.array([1, 0, 1, 1, 0], np.float32)
    xd, dyd, gd, gated_d = _in(x, ld), _in(dy, ld), _d(g), _d(gate)
    want = ref["dx"] + (r32.astype(np.float64) if res != "none" else 0.0)
    want_g = want / np.float64(np.float32(keep)) * gate.astype(np.float64)[np.arange(M) // rps][:, None]

    def run():
        stats, dgb, sc = _Out(M, 2), _Out(2, D), _Scratch(lib)
        dx = _Out(M, D, ld, init=r32 if res == "inplace" else None)
        rd = _in(r32, ld) if res == "distinct" else None
        go = _Out(M, D, ld) if gated else None
        assert lib.uu3d_op_row_stats(_p(xd), ld, D, M, EPS, stats.ptr, None) == OK
        assert lib.uu3d_op_ln_bwd_ex(_p(xd), _p(dyd), stats.ptr, _p(gd), ld, D, M, dx.ptr, dx.ptr if res == "inplace" else _p(rd),
                                     _p(gated_d) if gated else None, keep, rps, go.ptr if gated else None, dgb.ptr,
                                     C.c_void_p(dgb.ptr.value + 4 * D), sc.ptr, sc.n, None) == OK
        sc.check()
        return (dx.result(), dgb.result()) + ((go.result(),) if gated else ())
    out = _twice(run)
    _close(out[0].astype(np.float64) - (r32.astype(np.float64) if res != "none" else 0.0), ref["dx"], bars["dx"])
    _close(out[1][0], ref["dg"], bars["dg"])
    _close(out[1][1], ref["db"], bars["db"])
    if gated:
        bound = (bars["dx"] * np.abs(ref["dx"]).max() + 2 * U.ULP * np.abs(want).max()) / keep        # dx's bar through the division by keep, two more roundings
        err = np.abs(out[2] - want_g).max()
        print(f"gated copy: max-abs error {err:.3e} bound {bound:.3e}")
        assert err <= bound
        dead = np.repeat(gate == 0, rps)
        assert not out[2][dead].any(), "rows of a zero gate must be exactly 0"


def test_ln_bwd_ex_refusals(lib):
    M, D = 5, 32
    xd, gd = torch.ones(M, D + 4, device="cuda"), torch.ones(D, device="cuda")
    for why, kw, want in [("gate without its output", dict(gate=True, go=False), INVALID), ("keep 0", dict(gate=True, go=True, keep=0.0), INVALID),
                          ("rps 0", dict(gate=True, go=True, rps=0), INVALID), ("ld not x4", dict(ld=D + 2), INVALID), ("null dy", dict(dy=False), INVALID),
                          ("scratch below 2 D", dict(scratch=2 * D - 1), WORKSPACE)]:
        dx, go, dgb, sc = _Out(M, D, D + 4), _Out(M, D, D + 4), _Out(2, D), _Scratch(lib, kw.get("scratch", 4096))
        r = lib.uu3d_op_ln_bwd_ex(_p(xd), _p(xd) if kw.get("dy", True) else None, _p(xd), _p(gd), kw.get("ld", D + 4), D, M, dx.ptr, None,
                                  _p(gd) if kw.get("gate") else None, kw.get("keep", 0.9), kw.get("rps", 1), go.ptr if kw.get("go") else None,
                                  dgb.ptr, C.c_void_p(dgb.ptr.value + 4 * D), sc.ptr, sc.n, None)
        assert r == want, why
        dx.untouched(); go.untouched(); dgb.untouched(); sc.untouched()


# ---------------------------------------------------------------------------------------------------------------------------------
# identity_bwd, scale_rows
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", sorted(U.GEOMS))
def test_identity_bwd(lib, g):
    """Every geometry; the step launches the kernel for stride > 1 only (stride 1 is a copy there), the kernel itself takes stride 1 as well."""
    geom = U.GEOMS[g]
    s, pl, Li, Lo = geom
    B, D = U.CONV_B, 36
    dout = np.random.default_rng(Li).normal(size=(B * Lo, D)).astype(np.float32)
    ref = U.identity_bwd_ref(dout, B, geom)
    dd = _d(dout)

    def run():
        out = _Out(B * Li, D)
        assert lib.uu3d_op_identity_bwd(_p(dd), B, Li, Lo, s, U.lo_of(geom), D, out.ptr, None) == OK
        return (out.result(),)
    got = _twice(run)[0]
    assert np.array_equal(got.view(np.int32), ref.astype(np.float32).view(np.int32)), "a gather: selected rows bit for bit, every other row +0.0"
    assert (ref == 0).all(1).sum() == B * (Li - Lo)
    out = _Out(B * Li, D)
    assert lib.uu3d_op_identity_bwd(None, B, Li, Lo, s, 0, D, out.ptr, None) == INVALID
    assert lib.uu3d_op_identity_bwd(_p(dd), B, Li, Lo, 0, 0, D, out.ptr, None) == INVALID
    out.untouched()


@pytest.mark.parametrize("form", ["gate", "mask_want0", "mask_want1", "gate_and_mask"])
def test_scale_rows(lib, form):
    rows, D, rps, keep = 85, 36, 17, 0.9
    rng = np.random.default_rng(11)
    x = rng.normal(size=(rows, D)).astype(np.float32)
    gate = np.array([0, 1, 1, 0, 1], np.float32) if "gate" in form else None
    mask = (rng.random(rows) < 0.5) if "mask" in form else None
    want = 0 if form == "mask_want0" else 1
    ref = x.astype(np.float64)
    if gate is not None:
        ref = ref / np.float64(np.float32(keep)) * gate.astype(np.float64)[np.arange(rows) // rps][:, None]
    if mask is not None:
        ref = np.where((mask == bool(want))[:, None], ref, 0.0)
    xd, gd, md = _d(x), (None if gate is None else _d(gate)), (None if mask is None else _d(mask.astype(np.uint8) * 7))

    def run():
        out = _Out(rows, D)
        assert lib.uu3d_op_scale_rows(_p(xd), rows, D, _p(gd), keep, rps, _p(md), want, out.ptr, None) == OK
        return (out.result(),)
    got = _twice(run)[0]
    _close(got, ref, 2e-6)
    zero = (ref == 0).all(1)
    assert zero.any() and not got[zero].any(), "gated-off and masked rows must be exactly 0"
    if gate is None:
        assert np.array_equal(got[~zero], x[~zero]), "a row mask copies the rows it keeps"
    out = _Out(rows, D)
    assert lib.uu3d_op_scale_rows(_p(xd), rows, D, _p(xd), 0.0, rps, None, 0, out.ptr, None) == INVALID
    assert lib.uu3d_op_scale_rows(_p(xd), rows, D, None, keep, rps, _p(xd), 2, out.ptr, None) == INVALID
    assert lib.uu3d_op_scale_rows(None, rows, D, None, keep, rps, None, 0, out.ptr, None) == INVALID
    out.untouched()
