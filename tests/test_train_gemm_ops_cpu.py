"""The references of tests/test_train_gemm_ops_gpu.py (tests/train_gemm_util.py) held to torch float64 autograd of the layers they stand for, so
that a wrong reference cannot agree with a wrong kernel by construction; and the restated launch_gemm / launch_gemm_tn plans name the expected
branch of every case of the GPU file -- the check the GPU tests assert, so a case that drifts off its branch is caught without a GPU."""
import numpy as np
import pytest
import torch

from oracle import dropout_oracle
from tests import train_gemm_util as U
from tests.bwd_plan_util import _plan_gemm_tn

F64 = torch.float64


def _same(a, b, tol=1e-12):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1e-30)


def _conv_forward(x, w, geom):
    """The literal layer: ZeroPadding1D((pad_left, pad_right)) + Conv1D(kernel 3, 'valid', stride) of x[B][L_in][C] with w[3][C][N]."""
    s, pl, Li, Lo = geom
    xp = torch.nn.functional.pad(x, (0, 0, pl, U.pad_right(geom)))
    y = torch.stack([sum(xp[:, t * s + j] @ w[j] for j in range(3)) for t in range(Lo)], 1)
    assert (xp.shape[1] - 3) // s + 1 == Lo
    return y


@pytest.mark.parametrize("g", sorted(U.GEOMS))
def test_conv_transpose_gather_is_autograd_of_the_strided_convolution(g):
    geom = U.GEOMS[g]
    s, pl, Li, Lo = geom
    B, Cc, N = U.CONV_B, 8, 12
    rng = np.random.default_rng(Li + s)
    x = torch.tensor(rng.normal(size=(B, Li, Cc)), dtype=F64, requires_grad=True)
    w = torch.tensor(rng.normal(size=(3, Cc, N)).astype(np.float32), dtype=F64, requires_grad=True)      # (float32 values: the pack's type)
    dz = rng.normal(size=(B * Lo, N))
    y = _conv_forward(x, w, geom)
    _same(y.detach().numpy().reshape(B * Lo, N), U.conv3_gather(x.detach().numpy().reshape(B * Li, Cc), B, geom) @ w.detach().numpy().reshape(3 * Cc, N))
    y.backward(torch.tensor(dz.reshape(B, Lo, N)))
    wk = w.detach().numpy().reshape(3 * Cc, N)                                               # Keras (3 C, N), as the pack sees it
    x2, w2 = x, w
    # d input = gather(dz) times the conv-transpose operand's matrix (kind 5), through the very pack formula the GPU test checks bit for bit
    dh = U.convt_gather(dz, B, geom) @ U.gemm_matrix(wk.astype(np.float32), 5, Cc)
    _same(dh, x2.grad.numpy().reshape(B * Li, Cc))
    packed = U.pack_ref(wk.astype(np.float32), 5, Cc)
    _same(U.convt_gather(dz, B, geom) @ packed[:Cc, :3 * N].T.astype(np.float64), x2.grad.numpy().reshape(B * Li, Cc))
    # d kernel = gather(x)^T dz (TnLoadConv3)
    _same(U.conv3_gather(x2.detach().numpy().reshape(B * Li, Cc), B, geom).T @ dz, w2.grad.numpy().reshape(3 * Cc, N))


@pytest.mark.parametrize("g", sorted(U.GEOMS))
def test_identity_path_reference_is_autograd_of_trim_and_maxpool(g):
    geom = U.GEOMS[g]
    s, pl, Li, Lo = geom
    B, D = U.CONV_B, 6
    rng = np.random.default_rng(Li)
    x = torch.tensor(rng.normal(size=(B, Li, D)), dtype=F64, requires_grad=True)
    lo = U.lo_of(geom)
    trimmed = x[:, lo:Li - lo] if lo else x
    y = torch.nn.functional.max_pool1d(trimmed.transpose(1, 2), 1, s).transpose(1, 2) if s > 1 else trimmed
    assert y.shape[1] >= Lo
    dout = rng.normal(size=(B * Lo, D))
    y[:, :Lo].backward(torch.tensor(dout.reshape(B, Lo, D)))
    _same(U.identity_bwd_ref(dout, B, geom), x.grad.numpy().reshape(B * Li, D))


def test_gelu_and_relu_epilogue_references_are_autograd():
    rng = np.random.default_rng(3)
    h = (1.5 * rng.normal(size=(40, 24))).astype(np.float32)
    dy = rng.normal(size=(40, 24))
    t = torch.tensor(h, dtype=F64, requires_grad=True)
    torch.nn.functional.gelu(t).backward(torch.tensor(dy))
    _same(dy * U.gelu_grad(h), t.grad.numpy(), 1e-11)                                       # EpGeluGrad
    _same(U.gelu(h), torch.nn.functional.gelu(torch.tensor(h, dtype=F64)).numpy(), 1e-12)    # ALoadGelu / TnLoadGelu
    # relu followed by inverted Dropout; the step stores H AFTER the Dropout, so H > 0 = active and kept, and the gradient is dy * scale there
    rate = 0.1
    f = dropout_oracle.drop_factor(h.shape, rate, U.SEED, 102).astype(np.float64)
    t = torch.tensor(h, dtype=F64, requires_grad=True)
    H = torch.relu(t) * torch.tensor(f)
    H.backward(torch.tensor(dy))
    scale = float(f.max())
    assert abs(scale - 1.0 / (1.0 - rate)) < 1e-6 and (f == 0).any()
    _same(np.where(H.detach().numpy() > 0, dy * scale, 0.0), t.grad.numpy())                 # EpReluMask with inner_scale


def test_residual_gate_reference_zero_pattern_is_autograds():
    """out = x + Dropout(acc + bias) / keep * gate in torch: the elements the test compares for equality (branch_zero) are exactly those
    where d out / d acc vanishes, i.e. where the gate or the Dropout mask cuts the branch."""
    c = U.NN_BY_NAME["gelu-gate-drop-K64"]
    p = U.nn_problem(c.name)
    acc = torch.tensor(p["acc"], requires_grad=True)
    f = torch.tensor(dropout_oracle.drop_factor((c.M, p["ld"]), c.opt["drop"], U.SEED, 77)[:, :c.N].astype(np.float64))
    gate = torch.tensor(p["gate"].astype(np.float64))[torch.arange(c.M) // c.opt["rps"]][:, None]
    out = torch.tensor(p["aux"].astype(np.float64)) + (acc + torch.tensor(p["bias"].astype(np.float64))) * f / float(np.float32(c.opt["keep"])) * gate
    _same(out.detach().numpy(), p["ref"])
    out.sum().backward()
    assert np.array_equal(acc.grad.numpy() == 0, p["branch_zero"])


def test_colsum3_and_gated_layernorm_backward_are_autograd():
    rng = np.random.default_rng(9)
    seg, R = 8, 30
    g = rng.normal(size=(R, 3 * seg))
    b = [torch.zeros(seg, dtype=F64, requires_grad=True) for _ in range(3)]
    (torch.tensor(g) * (torch.zeros(R, 3 * seg, dtype=F64) + torch.cat(b))).sum().backward()      # q | k | v biases broadcast over the rows
    for s in range(3):
        _same(g.sum(0)[s * seg:(s + 1) * seg], b[s].grad.numpy())
    # y = LayerNorm(x); the residual stream x also flows on: d x = res + LN-backward(dy); the gated copy = DropPath backward of d x
    M, D, rps, keep = 10, 16, 5, 0.9
    x = torch.tensor(rng.normal(size=(M, D)), dtype=F64, requires_grad=True)
    gam = torch.tensor(1 + 0.1 * rng.normal(size=D), dtype=F64)
    dy, res = rng.normal(size=(M, D)), rng.normal(size=(M, D))
    (torch.nn.functional.layer_norm(x, (D,), gam, torch.zeros(D, dtype=F64), U.EPS) * torch.tensor(dy) + x * torch.tensor(res)).sum().backward()
    from tests.test_bwd_ops_edges_gpu import _ln_formula
    f = _ln_formula(x.detach().numpy(), dy, gam.numpy(), np.float64)
    _same(f["dx"] + res, x.grad.numpy(), 1e-9)
    gate = np.array([0.0, 1.0])
    u = torch.tensor(rng.normal(size=(M, D)), dtype=F64, requires_grad=True)                    # the branch input of z = u / keep * gate (DropPath)
    z = u / keep * torch.tensor(gate)[torch.arange(M) // rps][:, None]
    z.backward(torch.tensor(f["dx"] + res))
    _same((f["dx"] + res) / keep * gate[np.arange(M) // rps][:, None], u.grad.numpy())


def test_every_gpu_case_reaches_its_branch():
    seen = set()
    for c in U.NN_CASES:
        for h3 in (False, True):
            plan = U.plan_nn(c.M, c.N, c.K, U.FULL_SLAB, h3)
            assert plan["split"] == (c.K >= 256), (c.name, plan)
            if h3:
                assert plan["deep"] == c.deep, (c.name, plan)
            seen.add((c.src, c.ep, h3, plan["deep"], plan["split"]))
        assert c.M % 64 != 0 and (c.N < 64 or c.N % 64 != 0 or c.name.endswith("wide") or "out2" in c.name), c.name
    # every (loader, epilogue) of the census at both precisions, split and unsplit
    pairs = {(U.TA_GELU, U.EP_RES_GATE), (U.TA_PLAIN, U.EP_RES_GATE), (U.TA_LN, U.EP_BIAS), (U.TA_LN, U.EP_BIAS_RELU), (U.TA_CONV3, U.EP_CONV_RES),
             (U.TA_CONVT, U.EP_RELU_MASK), (U.TA_PLAIN, U.EP_GELU_GRAD), (U.TA_PLAIN, U.EP_RELU_MASK), (U.TA_PLAIN, U.EP_ADD), (U.TA_PLAIN, U.EP_STORE)}
    for src, ep in pairs:
        for split in (False, True):
            assert (src, ep, False, None, split) in seen and (src, ep, True, True, split) in seen, (src, ep, split)
    for src, ep in ((U.TA_GELU, U.EP_RES_GATE), (U.TA_CONVT, U.EP_RELU_MASK), (U.TA_LN, U.EP_BIAS)):
        assert (src, ep, True, False, True) in seen, "one non-DEEP f16x3 case per loader"
    kernels = set()
    for c in U.TN_CASES:
        plan = _plan_gemm_tn(c.R, c.P, c.Q, c.slab if c.slab is not None else U.FULL_SLAB, bool(c.h3))
        assert {k: plan[k] for k in c.expect} == c.expect, (c.name, plan)
        kernels.add((c.src, c.ep, plan["kernel"], plan["combine"]))
    for want in [(U.TA_LN, U.WEP_STORE3, "tn_f32", None), (U.TA_LN, U.WEP_STORE3, "tn_f32", "reduce"), (U.TA_LN, U.WEP_STORE3, "tn_h3", None),
                 (U.TA_LN, U.WEP_STORE3, "tn_h3", "reduce"), (U.TA_LN, U.WEP_STORE, "tn_h3", "reduce"), (U.TA_GELU, U.WEP_STORE, "tn_f32", "reduce16"),
                 (U.TA_GELU, U.WEP_STORE, "tn_f32", "reduce"), (U.TA_CONV3, U.WEP_STORE, "tn_f32", None), (U.TA_CONV3, U.WEP_STORE, "tn_h3", None),
                 (U.TA_CONV3, U.WEP_STORE, "tn_h3", "reduce")]:
        assert want in kernels, want
    d160 = U.TN_BY_NAME["ln-store3-d160-R600"]
    assert d160.Q // 3 % 128 != 0 and d160.P % 128 != 0                                      # a segment boundary inside a 128-wide tile


def test_every_problem_builds_with_the_factor_its_options_state():
    """nn_problem asserts the largest multiplying factor of each epilogue from the case's options (scale, keep, Dropout rate, max gelu');
    nn_bound asserts every allowance <= 1e-4."""
    for c in U.NN_CASES:
        p = U.nn_problem(c.name)
        for prec in (U.PREC_F32, U.PREC_H3):
            assert 0.0 < U.nn_bound(c, p, prec) <= 1e-4
        if c.opt.get("scale", 1.0) != 1.0:
            assert abs(p["factor"] - 1.0 / 0.9) < 1e-6


def test_pack_formula_and_operand_dims():
    w = np.arange(51 * 40, dtype=np.float32).reshape(51, 40)
    assert U.pack_ref(w, 1).shape == (128, 64) and U.pack_ref(w, 4).shape == (64, 64)
    assert U.pack_ref(w, 1)[7, 5] == w[5, 7] and U.pack_ref(w, 4)[5, 7] == w[5, 7]
    w5 = np.arange(72 * 40, dtype=np.float32).reshape(72, 40)
    p5 = U.pack_ref(w5, 5, 24)
    assert p5.shape == (128, 128) and p5[3, 2 * 40 + 9] == w5[2 * 24 + 3, 9]
    _same(U.gemm_matrix(w5, 5, 24), p5[:24, :120].T.astype(np.float64))
