"""The forward's kernels for a LayerNorm-fed Dense layer, each on its own through the operator ABI (include/uu3d_ops.h), against a
float64 restatement of the same expression (kl.LayerNormalization + kl.Dense / vit.MLP, vision_transformer.py:46-68,135-137,183,188):

  * gemm_h3_panel8_kernel<EP, CPW, 3> (8 waves) for every (epilogue, chunks per workgroup) pair block_head can launch, and the 4-wave
    gemm_h3_panel_kernel at every column split, its unrolled residual forms included  (uu3d_op_ln_dense_panel_ex);
  * mlp_fused_h3_kernel                                                               (uu3d_op_mlp_fused);
  * gemm_h3_wt_kernel<WtLoadF32, EP, 6>, the few-row path                             (uu3d_op_ln_dense_wt).

The operators launch through csrc/uu3d_launch.h, as the forward's Launcher does: a case here runs the instantiation the forward runs.
Inputs as in test_panel_op_gpu.py (rows with their own offset and scale, one row scaled by 1e-6, gamma 1 +- 0.1, weights drawn for
unit-scale outputs).  Every output buffer is NaN-filled and carries a guard row (a guard tile behind fragment-ordered output).

Bounds (none of them taken from what these kernels measure):
  * one LayerNorm + Dense: 2e-5 max-abs on unit-scale outputs -- test_panel_op_gpu.py's bound for this layer; planes are read as
    hi + lo / 2048; the residual forms are held to it on the sum;
  * Ln-tail fragments: 2e-5 + 2^-20.  The step: ln_split_frag_kernel (ln_split_frag_row in the epilogue) stores y through h3_split as
    hi = f16(y), lo = f16((y - hi) * 2048).  |y - hi| <= 2^(e-11) for 2^e <= |y| < 2^(e+1), so the lo plane holds a value of magnitude
    <= 2^e with an 11-bit significand: what hi + lo / 2048 cannot represent of y is <= 2^(e-11) / 2048 = 2^(e-22), = 2^-20 for |y| < 8
    (asserted) -- a lo below the smallest normal half is flushed, which loses < 2^-14 / 2048 = 2^-25;
  * fused MLP: 4e-5 = two chained layers at 2e-5 each, on sum_s mslab[s] + b2 formed in float64.
Bit identity: for a fixed (M, N, epilogue, waves) every legal column split S gives the same bits (one writer per element, its k order
does not depend on the column range) -- for the 4-wave residual epilogue that sets the unrolled CPW 12 / 6 / 4 kernels (S = 1, 2, 3)
against the runtime chunk loop (S = 4, 6, 12).  4 and 8 waves are NOT compared bitwise: the 8-wave kernel splits the contraction over
wave pairs.
gemm_h3_wt_kernel: block_head calls it only with the contraction over d_temporal (K = 384, four waves); its K = 768 form (eight waves)
is not reachable from the forward and has no case here."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

K = 384
EPS = 1e-5
TOL = 2e-5                      # test_panel_op_gpu.py: LayerNorm + Dense, unit-scale outputs
LN_STEP = 2.0 ** -20            # hi / lo representation step below 8 (module docstring)
TOL_MLP = 4e-5                  # two chained layers
QSCALE = float(np.float32(1.44269504088896341 / np.sqrt(48.0)))          # log2(e) / sqrt(d_h), the forward's attn_qscale()
EP_BIAS, EP_RELU_SPLIT, EP_SPLIT_Q, EP_RESIDUAL, EP_RESIDUAL_LN = range(5)
EP_NAME = {EP_BIAS: "Bias", EP_RELU_SPLIT: "BiasReluSplit", EP_SPLIT_Q: "BiasSplitQ", EP_RESIDUAL: "BiasResidual", EP_RESIDUAL_LN: "BiasResidualLn"}
INVALID = 1                     # UU3D_ERR_INVALID_ARGUMENT

M_PANEL = [1, 31, 33, 127, 128, 129, 1025, 1207]
M_MLP = [1, 127, 129, 1025, 1207]
M_WT = [1, 31, 32, 33, 384, 512]


@pytest.fixture(scope="module")
def lib():
    from uplift_upsample_3dhpe_amd import _capi
    assert _capi.UU3D_ERR_INVALID_ARGUMENT == INVALID
    return _capi.load_library()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                  # (a copy: the cached inputs are read-only)


def _nan(n, dtype):
    return torch.full((n,), float("nan"), dtype=dtype, device="cuda")


# ---- inputs and float64 references: made once, shared, never modified ----
@functools.lru_cache(maxsize=None)
def _rows(M):
    rng = np.random.default_rng(1000 + M)
    x = (rng.normal(size=(M, 1)) + (0.5 + np.abs(rng.normal(size=(M, 1)))) * rng.normal(size=(M, K))).astype(np.float32)
    if M > 3:
        x[3, :] *= 1e-6                                               # a row of tiny values: f16 denormal range of the split
    res = rng.normal(size=(M, K)).astype(np.float32)                  # the residual stream of the projection forms, unit scale
    for a in (x, res):
        a.setflags(write=False)
    return x, res


@functools.lru_cache(maxsize=None)
def _ln_params(which):
    rng = np.random.default_rng(7 + which)
    g = (1.0 + 0.1 * rng.normal(size=K)).astype(np.float32)
    b = (0.1 * rng.normal(size=K)).astype(np.float32)
    return g, b


@functools.lru_cache(maxsize=None)
def _dense(N):
    rng = np.random.default_rng(N * 3)
    w = (0.05 * rng.normal(size=(K, N))).astype(np.float32)           # Keras (in, out): 0.05 sqrt(384) ~ 1 at the output
    bias = (0.1 * rng.normal(size=N)).astype(np.float32)
    return w, bias


def _layer_norm(x, g, b):
    x = x.astype(np.float64)
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    return (x - mean) / np.sqrt(var + EPS) * g.astype(np.float64) + b.astype(np.float64)


@functools.lru_cache(maxsize=None)
def _ref(M, N):
    """LayerNorm(x) W + bias in float64."""
    w, bias = _dense(N)
    r = _layer_norm(_rows(M)[0], *_ln_params(1)) @ w.astype(np.float64) + bias.astype(np.float64)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def _dev_inputs(M):
    x, res = _rows(M)
    return _dev(x), _dev(_ln_params(1)[0]), _dev(_ln_params(1)[1]), _dev(_ln_params(2)[0]), _dev(_ln_params(2)[1])


_operands = {}


def _panel_operand(lib, N):
    if N not in _operands:
        w, bias = _dense(N)
        op = torch.empty(int(lib.uu3d_op_panel_operand_bytes(N)), dtype=torch.uint8, device="cuda")
        assert lib.uu3d_op_panel_pack(np.ascontiguousarray(w).ctypes.data_as(C.c_void_p), N, _p(op), None) == 0
        _operands[N] = (op, _dev(bias))
    return _operands[N]


A_TILE_BYTES = 32 * K * 2 * 2           # one 32-row panel of A fragments: two f16 planes


class PanelRun:
    """One call of uu3d_op_ln_dense_panel_ex on NaN-filled, guarded buffers."""

    def __init__(self, lib, M, N, waves, S, ep):
        self.M, self.N, self.ep = M, N, ep
        xd, g1, b1, g2, b2 = _dev_inputs(M)
        op, biasd = _panel_operand(lib, N)
        self.a_bytes = int(lib.uu3d_op_panel_a_bytes(M))
        self.scratch = _nan((self.a_bytes + A_TILE_BYTES) // 2, torch.float16)
        self.out = self.resid = self.ln_out = None
        if ep == EP_BIAS:
            self.out = _nan((M + 1) * N, torch.float32)
        elif ep in (EP_RELU_SPLIT, EP_SPLIT_Q):
            self.out = _nan((2 * M + 1) * N, torch.float16)
        else:
            self.resid = _nan((M + 1) * K, torch.float32)
            self.resid[:M * K] = _dev(_rows(M)[1]).reshape(-1)
            if ep == EP_RESIDUAL_LN:
                self.ln_out = _nan((self.a_bytes + A_TILE_BYTES) // 2, torch.float16)
        self.status = lib.uu3d_op_ln_dense_panel_ex(_p(xd), K, M, _p(g1), _p(b1), EPS, _p(op), _p(biasd), N, waves, S, ep, QSCALE, _p(self.scratch),
                                                    _p(self.out), N, _p(self.resid), _p(g2), _p(b2), _p(self.ln_out), None)
        torch.cuda.synchronize()

    def untouched(self):
        ok = bool(torch.isnan(self.scratch).all())
        if self.out is not None:
            ok = ok and bool(torch.isnan(self.out).all())
        if self.resid is not None:
            ok = ok and np.array_equal(self.resid[:self.M * K].cpu().numpy().reshape(self.M, K), _rows(self.M)[1]) and bool(torch.isnan(self.resid[self.M * K:]).all())
        if self.ln_out is not None:
            ok = ok and bool(torch.isnan(self.ln_out).all())
        return ok

    def check_guards(self):
        M, N = self.M, self.N
        assert torch.isnan(self.scratch[self.a_bytes // 2:]).all(), "the LayerNorm fragments pass uu3d_op_panel_a_bytes(M)"
        if self.ep == EP_BIAS:
            assert torch.isnan(self.out[M * N:]).all(), "rows past M were written"
        elif self.out is not None:
            assert torch.isnan(self.out[2 * M * N:]).all(), "the planes pass 2 M N halfs"
        if self.resid is not None:
            assert torch.isnan(self.resid[M * K:]).all(), "residual rows past M were written"
        if self.ln_out is not None:
            assert torch.isnan(self.ln_out[self.a_bytes // 2:]).all(), "the Ln fragments pass uu3d_op_panel_a_bytes(M)"

    def bits(self):
        """The meaningful part of every output, raw."""
        M, N = self.M, self.N
        if self.ep == EP_BIAS:
            return [self.out[:M * N].cpu().numpy().view(np.uint32)]
        if self.out is not None:
            return [self.out[:2 * M * N].cpu().numpy().view(np.uint16)]
        b = [self.resid[:M * K].cpu().numpy().view(np.uint32)]
        if self.ln_out is not None:
            b.append(self.ln_out[:self.a_bytes // 2].cpu().numpy().view(np.uint16))
        return b

    def value(self):
        """float64 [M][N] of the Dense output (planes: hi + lo / 2048; residual forms: the updated stream)."""
        M, N = self.M, self.N
        if self.ep == EP_BIAS:
            return self.out[:M * N].cpu().numpy().astype(np.float64).reshape(M, N)
        if self.out is not None:
            o = self.out[:2 * M * N].cpu().numpy().astype(np.float64).reshape(2, M, N)
            return o[0] + o[1] / 2048.0
        return self.resid[:M * K].cpu().numpy().astype(np.float64).reshape(M, K)

    def ln_value(self, lib):
        """The Ln epilogue's fragments through uu3d_op_panel_a_unpack: float64 [Mp][384] over the whole panels (rows past M: NaN expected)."""
        Mp = (self.M + 31) // 32 * 32
        frag = np.ascontiguousarray(self.ln_out[:self.a_bytes // 2].cpu().numpy())
        hi = np.empty((Mp, K), np.float32); lo = np.empty((Mp, K), np.float32)
        assert lib.uu3d_op_panel_a_unpack(frag.ctypes.data_as(C.c_void_p), Mp, hi.ctypes.data_as(C.c_void_p), lo.ctypes.data_as(C.c_void_p)) == 0
        return hi.astype(np.float64) + lo.astype(np.float64) / 2048.0


def _want(M, N, ep):
    ref = _ref(M, N)
    if ep == EP_BIAS:
        return ref
    if ep == EP_RELU_SPLIT:
        return np.maximum(ref, 0.0)
    if ep == EP_SPLIT_Q:
        w = ref.copy()
        w[:, :N // 3] *= QSCALE
        return w
    return _rows(M)[1].astype(np.float64) + ref


# the (epilogue, N, waves, S) schedules.  8 waves: block_head launches ln_qkv (N = 1152: Bias or BiasSplitQ), ln_fc1 (N = 768: BiasReluSplit) and
# proj_res (N = 384: BiasResidual, BiasResidualLn at S = 1) through gemm_panel / gemm_panel_residual, which take the 8-wave kernel whenever
# (N / 32) / S is one of 4, 6, 8, 9, 12 -- N = 1152: S = 3, 4, 6, 9 (CPW 12, 9, 6, 4); N = 768: S = 2, 3, 4, 6 (CPW 12, 8, 6, 4); N = 384: S = 1, 2, 3
# (CPW 12, 6, 4).  Bias at CPW 8 and BiasReluSplit at CPW 9 need another width than the model's layer has: N = 768 / 1152 here, so that every CPW
# is hit for those two as well (BiasSplitQ x 8 and the residual forms x 8, 9 do not exist: 36 and 12 chunks have no such divisor).
SCHEDULES = (
    [(ep, 1152, 4, S) for ep in (EP_BIAS, EP_SPLIT_Q) for S in (2, 3, 4, 6, 9, 12, 18)]
    + [(EP_RELU_SPLIT, 768, 4, S) for S in (1, 2, 3, 4, 6, 8, 12, 24)]
    + [(EP_RESIDUAL, 384, 4, S) for S in (1, 2, 3, 4, 6, 12)]            # 1, 2, 3: unrolled CPW 12 / 6 / 4; 4, 6, 12: the runtime chunk loop
    + [(ep, 1152, 8, S) for ep in (EP_BIAS, EP_SPLIT_Q) for S in (3, 4, 6, 9)]
    + [(EP_RELU_SPLIT, 768, 8, S) for S in (2, 3, 4, 6)]
    + [(EP_RESIDUAL, 384, 8, S) for S in (1, 2, 3)]
    + [(EP_RESIDUAL_LN, 384, 8, 1)]
    + [(EP_BIAS, 768, 8, 3), (EP_RELU_SPLIT, 1152, 8, 4)]
)
_first_bits = {}                # (M, N, waves, epilogue family) -> (S, bits) of the first schedule that ran


@pytest.mark.parametrize("M", M_PANEL)
@pytest.mark.parametrize("ep,N,waves,S", SCHEDULES, ids=[f"{EP_NAME[e]}-N{n}-w{w}-S{s}" for e, n, w, s in SCHEDULES])
def test_panel_schedule(lib, M, ep, N, waves, S):
    r = PanelRun(lib, M, N, waves, S, ep)
    assert r.status == 0
    r.check_guards()
    # (a) float64
    got, want = r.value(), _want(M, N, ep)
    assert np.isfinite(got).all()
    err = np.abs(got - want).max()
    print(f"panel{waves} {EP_NAME[ep]} M={M} N={N} S={S} cpw={N // 32 // S}: max-abs {err:.3e} (scale {np.abs(want).max():.2f})")
    assert err <= TOL
    if ep == EP_RESIDUAL_LN:
        y = r.ln_value(lib)
        assert np.isnan(y[M:]).all(), "fragment rows past M were written"
        want_ln = _layer_norm(want, *_ln_params(2))
        assert np.abs(want_ln).max() < 8.0                            # LN_STEP holds below 8
        err_ln = np.abs(y[:M] - want_ln).max()
        print(f"panel8 BiasResidualLn M={M}: LayerNorm-2 fragments max-abs {err_ln:.3e} (scale {np.abs(want_ln).max():.2f})")
        assert err_ln <= TOL + LN_STEP
    # (d) run to run
    bits = r.bits()
    again = PanelRun(lib, M, N, waves, S, ep).bits()
    assert all(np.array_equal(a, b) for a, b in zip(bits, again)), "two runs differ"
    # (c) every column split of one product gives the same bits (the Ln epilogue's residual stream: the plain residual epilogue's)
    key = (M, N, waves, EP_RESIDUAL if ep == EP_RESIDUAL_LN else ep)
    s0, first = _first_bits.setdefault(key, (S, bits[0]))
    assert np.array_equal(bits[0], first), f"S = {S} and S = {s0} differ"


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("N", [384, 768, 1152])
@pytest.mark.parametrize("M", M_PANEL)
def test_panel_ex_default_is_the_old_op(lib, M, N, relu):
    """uu3d_op_ln_dense_panel is uu3d_op_ln_dense_panel_ex with (4 waves, splits 0): the same bits."""
    r = PanelRun(lib, M, N, 4, 0, EP_RELU_SPLIT if relu else EP_BIAS)
    assert r.status == 0
    r.check_guards()
    xd, g1, b1, _, _ = _dev_inputs(M)
    op, biasd = _panel_operand(lib, N)
    scratch = torch.empty(r.a_bytes, dtype=torch.uint8, device="cuda")
    out = _nan((2 * M + 1) * N, torch.float16) if relu else _nan((M + 1) * N, torch.float32)
    assert lib.uu3d_op_ln_dense_panel(_p(xd), K, M, _p(g1), _p(b1), EPS, _p(op), _p(biasd), N, relu, _p(scratch), _p(out), N, None) == 0
    torch.cuda.synchronize()
    n = 2 * M * N if relu else M * N
    assert torch.isnan(out[n:]).all()
    old = out[:n].cpu().numpy().view(np.uint16 if relu else np.uint32)
    assert np.array_equal(old, r.bits()[0])
    err = np.abs(r.value() - _want(M, N, EP_RELU_SPLIT if relu else EP_BIAS)).max()
    print(f"panel4 default split M={M} N={N} relu={relu}: max-abs {err:.3e}")
    assert err <= TOL


# (e) what no kernel is instantiated for
REJECTED = [
    ("8 waves, 18 chunks per workgroup", EP_BIAS, 1152, 8, 2), ("8 waves, 2 chunks", EP_BIAS, 1152, 8, 18), ("8 waves, 1 chunk", EP_SPLIT_Q, 1152, 8, 36),
    ("8 waves, 24 chunks", EP_RELU_SPLIT, 768, 8, 1), ("8 waves, 3 chunks", EP_RELU_SPLIT, 768, 8, 8), ("8 waves, 2 chunks (residual)", EP_RESIDUAL, 384, 8, 6),
    ("8 waves, 36 chunks", EP_BIAS, 1152, 8, 1), ("8 waves, splits 0", EP_BIAS, 1152, 8, 0),
    ("S = 5 does not divide 36", EP_BIAS, 1152, 4, 5), ("S = 7 does not divide 36", EP_SPLIT_Q, 1152, 4, 7), ("S = 5 does not divide 24", EP_RELU_SPLIT, 768, 4, 5),
    ("S = 5 does not divide 12", EP_RESIDUAL, 384, 4, 5), ("S = 5 does not divide 36 (8 waves)", EP_BIAS, 1152, 8, 5), ("S = 72 > chunks", EP_BIAS, 1152, 4, 72),
    ("36 chunks > 32 per workgroup", EP_BIAS, 1152, 4, 1), ("36 chunks > 32 per workgroup (SplitQ)", EP_SPLIT_Q, 1152, 4, 1),
    ("Ln epilogue on 4 waves", EP_RESIDUAL_LN, 384, 4, 1), ("Ln epilogue with S = 2", EP_RESIDUAL_LN, 384, 8, 2), ("Ln epilogue with S = 3", EP_RESIDUAL_LN, 384, 8, 3),
    ("Ln epilogue with N = 768", EP_RESIDUAL_LN, 768, 8, 2), ("residual epilogue with N = 768", EP_RESIDUAL, 768, 4, 2),
    ("6 waves", EP_BIAS, 1152, 6, 3), ("negative splits", EP_BIAS, 1152, 4, -1), ("unknown epilogue", 5, 384, 4, 1),
]


@pytest.mark.parametrize("why,ep,N,waves,S", REJECTED, ids=[r[0] for r in REJECTED])
def test_panel_rejects(lib, why, ep, N, waves, S):
    r = PanelRun(lib, 129, N, waves, S, ep)
    assert r.status == INVALID, why
    assert r.untouched(), "a rejected call wrote something"


# ---- fused MLP ----
@functools.lru_cache(maxsize=None)
def _mlp_weights():
    rng = np.random.default_rng(77)
    w1, b1 = _dense(768)                                              # hidden pre-activations of unit scale
    w2 = (0.05 * rng.normal(size=(768, K))).astype(np.float32)        # relu(unit-scale hidden) has rms ~0.7: 0.05 sqrt(768) 0.7 ~ 1 at the output
    b2 = (0.1 * rng.normal(size=K)).astype(np.float32)
    return w1, b1, w2, b2


@functools.lru_cache(maxsize=None)
def _mlp_operand(lib):
    w1, b1, w2, _ = _mlp_weights()
    op = torch.empty(int(lib.uu3d_op_mlp_operand_bytes()), dtype=torch.uint8, device="cuda")
    assert lib.uu3d_op_mlp_pack(np.ascontiguousarray(w1).ctypes.data_as(C.c_void_p), np.ascontiguousarray(w2).ctypes.data_as(C.c_void_p), _p(op), None) == 0
    return op, _dev(b1)


@pytest.mark.parametrize("M", M_MLP)
def test_mlp_fused(lib, M):
    w1, b1, w2, b2 = _mlp_weights()
    xd, g1, be1, _, _ = _dev_inputs(M)
    op, b1d = _mlp_operand(lib)
    a_bytes = int(lib.uu3d_op_panel_a_bytes(M))

    def run():
        scratch = _nan((a_bytes + A_TILE_BYTES) // 2, torch.float16)
        mslab = _nan((3 * M + 1) * K, torch.float32)                  # [3][M][384] and a guard row
        assert lib.uu3d_op_mlp_fused(_p(xd), K, M, _p(g1), _p(be1), EPS, _p(op), _p(b1d), _p(scratch), _p(mslab), None) == 0
        torch.cuda.synchronize()
        assert torch.isnan(scratch[a_bytes // 2:]).all()
        assert torch.isnan(mslab[3 * M * K:]).all(), "rows past the third slab were written"
        return mslab[:3 * M * K].cpu().numpy()
    slabs = run()
    assert np.isfinite(slabs).all()
    got = slabs.astype(np.float64).reshape(3, M, K).sum(0) + b2.astype(np.float64)
    hidden = np.maximum(_ref(M, 768), 0.0)
    want = hidden @ w2.astype(np.float64) + b2.astype(np.float64)
    err = np.abs(got - want).max()
    print(f"mlp_fused M={M}: max-abs {err:.3e} (hidden scale {np.abs(hidden).max():.2f}, output scale {np.abs(want).max():.2f})")
    assert err <= TOL_MLP
    assert np.array_equal(slabs.view(np.uint32), run().view(np.uint32)), "two runs differ"


def test_mlp_fused_rejects(lib):
    xd, g1, be1, _, _ = _dev_inputs(129)
    op, b1d = _mlp_operand(lib)
    scratch = _nan(int(lib.uu3d_op_panel_a_bytes(129)) // 2, torch.float16)
    mslab = _nan(3 * 129 * K, torch.float32)
    for M, ldx in ((0, K), (129, K - 4), (129, K + 2)):
        assert lib.uu3d_op_mlp_fused(_p(xd), ldx, M, _p(g1), _p(be1), EPS, _p(op), _p(b1d), _p(scratch), _p(mslab), None) == INVALID
    assert lib.uu3d_op_mlp_fused(_p(xd), K, 129, _p(g1), _p(be1), EPS, None, _p(b1d), _p(scratch), _p(mslab), None) == INVALID
    torch.cuda.synchronize()
    assert torch.isnan(mslab).all() and torch.isnan(scratch).all()


# ---- few-row GEMM ----
_wt_operands = {}


def _wt_operand(lib, N):
    if N not in _wt_operands:
        w, bias = _dense(N)
        op = torch.empty(int(lib.uu3d_op_wt_operand_bytes(N, K)), dtype=torch.uint8, device="cuda")
        assert lib.uu3d_op_wt_pack(np.ascontiguousarray(w).ctypes.data_as(C.c_void_p), K, N, _p(op), None) == 0
        _wt_operands[N] = (op, _dev(bias))
    return _wt_operands[N]


def _wt_run(lib, M, N, ep):
    xd, g1, b1, _, _ = _dev_inputs(M)
    op, biasd = _wt_operand(lib, N)
    out = _nan((M + 1) * N, torch.float32) if ep == EP_BIAS else _nan((2 * M + 1) * N, torch.float16)
    st = lib.uu3d_op_ln_dense_wt(_p(xd), K, M, K, _p(g1), _p(b1), EPS, _p(op), _p(biasd), N, ep, QSCALE, _p(out), N, None)
    torch.cuda.synchronize()
    return st, out


@pytest.mark.parametrize("ep", [EP_BIAS, EP_RELU_SPLIT, EP_SPLIT_Q], ids=lambda e: EP_NAME[e])
@pytest.mark.parametrize("N", [768, 1152])
@pytest.mark.parametrize("M", M_WT)
def test_wt(lib, M, N, ep):
    st, out = _wt_run(lib, M, N, ep)
    assert st == 0
    n = M * N if ep == EP_BIAS else 2 * M * N
    assert torch.isnan(out[n:]).all(), "written past row M"
    o = out[:n].cpu().numpy()
    got = o.astype(np.float64).reshape(M, N) if ep == EP_BIAS else o.astype(np.float64).reshape(2, M, N)[0] + o.astype(np.float64).reshape(2, M, N)[1] / 2048.0
    want = _want(M, N, ep)
    assert np.isfinite(got).all()
    err = np.abs(got - want).max()
    print(f"gemm_wt {EP_NAME[ep]} M={M} N={N}: max-abs {err:.3e} (scale {np.abs(want).max():.2f})")
    assert err <= TOL
    _, out2 = _wt_run(lib, M, N, ep)
    assert np.array_equal(o.view(np.uint32 if ep == EP_BIAS else np.uint16), out2[:n].cpu().numpy().view(np.uint32 if ep == EP_BIAS else np.uint16)), "two runs differ"


WT_REJECTED = [("513 rows", 513, 768, EP_BIAS, K), ("no rows", 0, 768, EP_BIAS, K), ("N = 776 is no multiple of 32", 512, 776, EP_BIAS, K),
               ("K = 512", 512, 768, EP_RELU_SPLIT, 512), ("a residual epilogue", 512, 768, EP_RESIDUAL, K), ("SplitQ with N = 800", 512, 800, EP_SPLIT_Q, K)]


@pytest.mark.parametrize("why,M,N,ep,Kc", WT_REJECTED, ids=[r[0] for r in WT_REJECTED])
def test_wt_rejects(lib, why, M, N, ep, Kc):
    xd, g1, b1, _, _ = _dev_inputs(512)                               # (rejected before any launch: the buffers only have to exist)
    op, biasd = _wt_operand(lib, 1152)
    out = _nan(514 * 1152, torch.float32)
    st = lib.uu3d_op_ln_dense_wt(_p(xd), K, M, Kc, _p(g1), _p(b1), EPS, _p(op), _p(biasd), N, ep, QSCALE, _p(out), N, None)
    torch.cuda.synchronize()
    assert st == INVALID, why
    assert torch.isnan(out).all(), "a rejected call wrote something"
