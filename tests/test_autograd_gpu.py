"""Autograd through the HIP backward pass (the role of tf.GradientTape, train.py:477-498): model(..., training=True) under grad mode
records a tape (uu3d_train_forward_tape) and loss.backward() runs the library's backward pass from the output gradients
(uu3d_train_backward_tape).  Checked against float64 autograd through the oracle, against the built-in training step, and for the
parameter's life cycle (optimizer steps, version checks, the non-finite word)."""
import ctypes as C

import numpy as np
import pytest

import uplift_upsample_3dhpe_amd as pkg
from tests import util

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

_MASKS = [(0, 0), (1, 0), (2, 0)]


def _setup(cfgname, B, seed, variant=None, weights_seed=None):
    cfg = util.load_config(cfgname)
    cfg.BATCH_SIZE = 4
    if variant is None:
        cfg.DROP_PATH_RATE = [0.0, 0.0, 0.0]
    elif variant == "droppath":
        cfg.DROP_PATH_RATE = [0.1, 0.1, 0.4]
    elif variant == "dropout":
        cfg.DROP_PATH_RATE = [0.0, 0.0, 0.0]
        cfg.DROP_RATE, cfg.ATTENTION_DROP_RATE = 0.1, 0.15
    elif variant == "tokenmask":
        cfg.DROP_PATH_RATE = [0.0, 0.0, 0.0]
        cfg.TOKEN_MASK_RATE = 0.3
    arch = pkg.arch_from_config(cfg)
    w = pkg.init_weights(arch, seed=seed if weights_seed is None else weights_seed, perturb=0.1)
    model = pkg.build_uplift_upsample_transformer(cfg, weights=w)
    x, _ = util.synthetic_batch(cfg, B, seed=seed)
    ms = cfg.MASK_STRIDE if isinstance(cfg.MASK_STRIDE, list) else [cfg.MASK_STRIDE]
    m = np.stack([util.eval_stride_mask(arch.num_frames, cfg.SEQUENCE_STRIDE, ms[_MASKS[b % len(_MASKS)][0]], 0) for b in range(B)])
    xm = (x * m[:, :, None, None].astype(np.float32)).astype(np.float32)
    gt = np.random.default_rng(seed + 50).normal(0, 0.3, size=(B, arch.num_frames, arch.num_keypoints, 3)).astype(np.float32)
    return cfg, arch, w, model, x, xm, m, gt


def _draws(tr, arch, B):
    """The draws the next training-mode call takes from the trainer's generator (the generator is left where it was)."""
    st = tr._rng.get_state()
    u = torch.rand(tr.drop_path_size(B), generator=tr._rng, device="cuda", dtype=torch.float32)
    tm = torch.rand((B, arch.num_frames), generator=tr._rng, device="cuda", dtype=torch.float32) if arch.token_mask_rate > 0 else None
    seed = 0
    if arch.drop_rate > 0 or arch.attention_drop_rate > 0:
        seed = int(torch.randint(0, 2 ** 62, (1,), generator=tr._rng, device="cuda", dtype=torch.int64).item())
    tr._rng.set_state(st)
    return u, tm, seed


def _split(model, flat):
    out, o = {}, 0
    flat = flat.detach().cpu().numpy() if torch.is_tensor(flat) else flat
    for name, shape in model._spec:
        n = int(np.prod(shape))
        out[name] = flat[o:o + n].reshape(shape)
        o += n
    return out


def _worst(got, ref):
    """The error measure of test_train_step_gpu.py::test_gradients_match_autograd: max |d| per tensor / max(|ref|, 1e-4 global max)."""
    gmax = max(np.abs(v).max() for v in ref.values())
    worst = ("", 0.0)
    for name in ref:
        scale = max(np.abs(ref[name]).max(), 1e-4 * gmax)
        if name.endswith("/attn/wk/bias") and np.abs(ref[name]).max() < 1e-12 * gmax:      # structurally zero (softmax shift invariance)
            scale = max(scale, np.abs(ref[name.replace("/bias", "/kernel")]).max())
        err = float(np.abs(got[name] - ref[name]).max() / scale)
        if err > worst[1]:
            worst = (name, err)
    return worst


def _mpjpe_cotangents(model, full, central, gt, cfg):
    """What uu3d_mpjpe_loss returns as d loss / d predictions (the cotangents the built-in step starts its backward pass from)."""
    lib = model._lib
    B, N, J = full.shape[0], full.shape[1], full.shape[2]
    gF, gC = torch.empty_like(full), torch.empty_like(central)
    loss = torch.empty(3, dtype=torch.float32, device="cuda")
    scratch = torch.empty(4096, dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())         # noqa: E731
    st = lib.uu3d_mpjpe_loss(p(full.detach()), p(central.detach()), p(gt), B, N, J, int(cfg.ROOT_KEYTPOINT), float(cfg.LOSS_WEIGHT_CENTER),
                             float(cfg.LOSS_WEIGHT_SEQUENCE), int(cfg.BATCH_SIZE), p(loss), p(gF), p(gC), p(scratch),
                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0
    return gF, gC


@pytest.mark.parametrize("cfgname,variant", [("h36m_81", None), ("h36m_351", None), ("h36m_81", "droppath"), ("h36m_351", "droppath"),
                                             ("h36m_81", "dropout"), ("h36m_351", "tokenmask")])
def test_vjp_matches_float64_autograd(cfgname, variant):
    """d <(gF, gC), (full, central)> / d params and / d x for seeded random cotangents at 1e-2 and 1e-7 against float64 autograd
    through the oracle with the same draws.  1e-7 only resolves in the f16x3 gradient GEMMs because the cotangent pass scales them
    on the device.  Rows of masked frames of d x are exactly 0."""
    from oracle import uplift_oracle as O
    from uplift_upsample_3dhpe_amd.trainer import Trainer
    B = 3
    cfg, arch, w, model, x, xm, m, gt = _setup(cfgname, B, seed=7, variant=variant)
    tr = Trainer(model, cfg, seed=3)
    model.requires_grad_()
    u, tm, seed = _draws(tr, arch, B)
    xt = torch.from_numpy(xm).cuda().requires_grad_()
    full, central = model([xt, torch.from_numpy(m).cuda()], training=True)
    assert full.grad_fn is not None and central.grad_fn is not None
    p, = model.parameters()
    assert p is tr.params and p.grad is tr.grads

    dp = None
    if variant == "droppath":
        un = u.cpu().numpy()
        ns, nt = arch.spatial_depth * 2 * B * arch.num_frames, arch.temporal_depth * 2 * B
        dp = dict(rates=tuple(cfg.DROP_PATH_RATE), u_spatial=un[:ns].reshape(arch.spatial_depth, 2, B * arch.num_frames),
                  u_temporal=un[ns:ns + nt].reshape(arch.temporal_depth, 2, B), u_strided=un[ns + nt:].reshape(len(arch.strides), 2, B))
    tmc = dict(rate=0.3, u=tm.cpu().numpy()) if tm is not None else None
    doc = dict(rate=0.1, attn_rate=0.15, seed=seed) if variant == "dropout" else None
    pw = {k: torch.tensor(np.asarray(v), dtype=torch.float64, requires_grad=True) for k, v in w.items()}
    x64 = torch.tensor(xm, dtype=torch.float64, requires_grad=True)
    f64, c64, _ = O.forward_torch(util.hp_from_arch(arch), pw, x64, m, torch.float64, dp, tmc, None, doc)
    rows = m.any(axis=1)
    assert rows.all()
    assert np.abs(full.detach().cpu().numpy() - f64.detach().numpy()).max() <= util.TOL_MAX_ABS
    names = list(pw)
    rng = np.random.default_rng(23)
    for k, scale in enumerate((1e-2, 1e-7)):
        gF = (rng.normal(size=full.shape) * scale).astype(np.float32)
        gC = (rng.normal(size=central.shape) * scale).astype(np.float32)
        ref = torch.autograd.grad((f64, c64), [pw[n] for n in names] + [x64], (torch.from_numpy(gF).double(), torch.from_numpy(gC).double()),
                                  retain_graph=True, allow_unused=True)
        gref = {n: (g.numpy() if g is not None else np.zeros(w[n].shape)) for n, g in zip(names, ref[:-1])}
        gx_ref = ref[-1].numpy()
        gp, gx = torch.autograd.grad((full, central), (p, xt), (torch.from_numpy(gF).cuda(), torch.from_numpy(gC).cuda()), retain_graph=k == 0)
        worst = _worst(_split(model, gp), gref)
        print(f"{cfgname} {variant} cotangent scale {scale:g}: worst weight-gradient error {worst[1]:.2e} at {worst[0]}")
        assert worst[1] <= 1e-4, (scale, worst)
        gx = gx.cpu().numpy()
        assert np.abs(gx - gx_ref).max() <= 1e-4 * np.abs(gx_ref).max(), (scale, np.abs(gx - gx_ref).max(), np.abs(gx_ref).max())
        dead = m == 0
        assert dead.any() and not gx[dead].any()                       # masked frames: exactly 0
        assert np.abs(gx[~dead]).max() > 0


def test_tape_backward_is_bitwise_the_builtin_step_in_f32(monkeypatch):
    """UU3D_TRAIN_F32=1: a tape backward seeded with uu3d_mpjpe_loss's cotangents gives the gradients of Trainer.forward_backward
    bit for bit, and zero_grad + backward + apply_gradients leaves the weights of train_step bit for bit."""
    from uplift_upsample_3dhpe_amd.trainer import Trainer
    monkeypatch.setenv("UU3D_TRAIN_F32", "1")
    B = 4
    cfg, arch, w, model_a, x, xm, m, gt = _setup("h36m_81", B, seed=5, variant="droppath")
    model_b = pkg.build_uplift_upsample_transformer(cfg, weights=w)
    tr_a, tr_b = Trainer(model_a, cfg, seed=9), Trainer(model_b, cfg, seed=9)
    mt, gtt = torch.from_numpy(m).cuda(), torch.from_numpy(gt).cuda()
    u = torch.rand(tr_a.drop_path_size(B), generator=tr_a._rng, device="cuda", dtype=torch.float32)
    _, fa, ca = tr_a.forward_backward(torch.from_numpy(x).cuda(), gtt, mt, drop_path_uniform=u)
    model_b.requires_grad_()
    tr_b.zero_grad()
    fb, cb = model_b([torch.from_numpy(xm).cuda(), mt], training=True)      # draws u from tr_b's generator: the same u
    assert torch.equal(fa, fb.detach()) and torch.equal(ca, cb.detach())
    gF, gC = _mpjpe_cotangents(model_b, fb, cb, gtt, cfg)
    torch.autograd.backward((fb, cb), (gF, gC))
    assert tr_b.params.grad is tr_b.grads
    assert torch.equal(tr_a.grads, tr_b.grads)
    tr_a.apply_gradients()
    tr_b.apply_gradients()
    assert torch.equal(tr_a.params, tr_b.params)


def test_torch_mpjpe_loss_matches_builtin_step():
    """Default f16x3: the reference's MPJPE loss written in torch, loss.backward(), against Trainer.forward_backward on the same draws."""
    from uplift_upsample_3dhpe_amd.trainer import Trainer
    B = 4
    cfg, arch, w, model_a, x, xm, m, gt = _setup("h36m_351", B, seed=6, variant="droppath")
    cfg.BATCH_SIZE = 512                                    # the production normaliser: d loss / d joint ~ 1e-6
    model_b = pkg.build_uplift_upsample_transformer(cfg, weights=w)
    tr_a, tr_b = Trainer(model_a, cfg, seed=4), Trainer(model_b, cfg, seed=4)
    mt, gtt = torch.from_numpy(m).cuda(), torch.from_numpy(gt).cuda()
    u = torch.rand(tr_a.drop_path_size(B), generator=tr_a._rng, device="cuda", dtype=torch.float32)
    loss_a, _, _ = tr_a.forward_backward(torch.from_numpy(x).cuda(), gtt, mt, drop_path_uniform=u)
    model_b.requires_grad_()
    tr_b.zero_grad()
    full, central = model_b([torch.from_numpy(xm).cuda(), mt], training=True)
    g = gtt - gtt[:, :, cfg.ROOT_KEYTPOINT:cfg.ROOT_KEYTPOINT + 1]
    N, J = full.shape[1], full.shape[2]
    cen = torch.linalg.norm(g[:, N // 2] - central, dim=-1).sum() / (cfg.BATCH_SIZE * J)
    seq = torch.linalg.norm(g - full, dim=-1).sum() / (cfg.BATCH_SIZE * N * J)
    loss = cfg.LOSS_WEIGHT_CENTER * cen + cfg.LOSS_WEIGHT_SEQUENCE * seq
    loss.backward()
    assert float(loss.detach()) == pytest.approx(float(loss_a[0]), rel=1e-5)
    worst = _worst(_split(model_b, tr_b.grads), _split(model_a, tr_a.grads))
    print(f"torch MPJPE vs built-in step: worst {worst[1]:.2e} at {worst[0]}")
    assert worst[1] <= 1e-4, worst


def test_gradients_accumulate():
    """Two backward calls through one graph double .grad; one loss over two forwards (x and its flip) equals two separate backward calls."""
    B = 3
    cfg, arch, w, model, x, xm, m, gt = _setup("h36m_81", B, seed=8)
    model.requires_grad_()
    p, = model.parameters()
    assert isinstance(p, torch.nn.Parameter) and p.requires_grad
    mt = torch.from_numpy(m).cuda()
    xa = torch.from_numpy(xm).cuda()
    xb = xa.clone(); xb[..., 0] = -xb[..., 0]
    f, c = model([xa, mt], training=True)
    loss = (f ** 2).sum() * 1e-3 + c.abs().sum() * 1e-2
    loss.backward(retain_graph=True)
    g1 = p.grad.clone()
    loss.backward()
    assert torch.allclose(p.grad, 2 * g1, rtol=1e-6, atol=0)
    p.grad = None
    fa, ca = model([xa, mt], training=True)
    fb, cb = model([xb, mt], training=True)
    (((fa - fb) ** 2).sum() * 1e-3 + (ca * cb).sum() * 1e-2).backward()
    joint = p.grad.clone()
    p.grad = None
    fa, ca = model([xa, mt], training=True)
    fb, cb = model([xb, mt], training=True)
    fa_d, ca_d, fb_d, cb_d = fa.detach(), ca.detach(), fb.detach(), cb.detach()
    (((fa - fb_d) ** 2).sum() * 1e-3 + (ca * cb_d).sum() * 1e-2).backward()
    (((fa_d - fb) ** 2).sum() * 1e-3 + (ca_d * cb).sum() * 1e-2).backward()
    assert (p.grad - joint).abs().max() <= 1e-5 * joint.abs().max()


def test_sgd_step_reaches_the_inference_call():
    """torch.optim.SGD on model.parameters(): the next training=False call equals a fresh model loaded with the updated weights."""
    B = 3
    cfg, arch, w, model, x, xm, m, gt = _setup("h36m_81", B, seed=9)
    inputs = [torch.from_numpy(xm).cuda(), torch.from_numpy(m).cuda()]
    f0, _ = model(inputs, training=False)
    model.requires_grad_()
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    f, c = model(inputs, training=True)
    ((f ** 2).mean() + (c ** 2).mean()).backward()
    opt.step()
    f1, c1 = model(inputs, training=False)
    assert (f1 - f0).abs().max() > 1e-3
    fresh = pkg.build_uplift_upsample_transformer(cfg, weights=w)
    fresh.set_weights([v.cpu().numpy() for _, v in model.named_parameters()])
    f2, c2 = fresh(inputs, training=False)
    assert (f1 - f2).abs().max() <= util.TOL_MAX_ABS and (c1 - c2).abs().max() <= util.TOL_MAX_ABS
    # writes through p.data bypass the version counter: parameters_changed() declares them
    p, = model.parameters()
    p.data.mul_(0.5)
    model.parameters_changed()
    f3, _ = model(inputs, training=False)
    fresh.set_weights([v.cpu().numpy() for _, v in model.named_parameters()])
    f4, _ = fresh(inputs, training=False)
    assert (f3 - f4).abs().max() <= util.TOL_MAX_ABS


def test_safety():
    """In-place change between forward and backward: torch's version check.  A NaN cotangent raises the non-finite word and
    apply_gradients leaves the weights alone.  requires_grad off: no graph.  create_graph=True is refused."""
    from uplift_upsample_3dhpe_amd.trainer import Trainer
    B = 3
    cfg, arch, w, model, x, xm, m, gt = _setup("h36m_81", B, seed=10)
    inputs = [torch.from_numpy(xm).cuda(), torch.from_numpy(m).cuda()]
    tr = Trainer(model, cfg)
    f, c = model(inputs, training=True)
    assert f.grad_fn is None and c.grad_fn is None and not f.requires_grad
    model.requires_grad_()
    p, = model.parameters()
    f, c = model(inputs, training=True)
    with torch.no_grad():
        p[0] += 1.0
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        c.sum().backward()
    f, c = model(inputs, training=True)
    with pytest.raises(RuntimeError, match="higher-order"):
        torch.autograd.grad(c.sum(), p, create_graph=True)
    tr.zero_grad()
    assert not tr.nonfinite()
    f, c = model(inputs, training=True)
    gC = torch.zeros_like(c); gC[0, 0, 0] = float("nan")
    torch.autograd.backward((c,), (gC,))
    assert tr.nonfinite()
    before = tr.params.detach().clone()
    tr.apply_gradients()
    assert torch.equal(tr.params, before)
    tr.zero_grad()
    assert not tr.nonfinite()
