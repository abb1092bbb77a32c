"""GPU: training of the structures the forward already runs (tests/test_parity_gpu.py::test_structural_variants_match_oracle) but no
shipped config has -- TEMPORAL_TRANSFORMER_BLOCKS = 0 (no full-sequence head; the first strided block takes the key mask), STRIDES = []
(the central token x[:, N // 2] feeds strided_temporal_fc) and both -- through every training entry: the built-in step, autograd and
two ranks.  Without temporal blocks the reference's loss is (LOSS_WEIGHT_CENTER + LOSS_WEIGHT_SEQUENCE) * central (train.py:484-494);
oracle.train_oracle.train_step_grads assumes a full head, so the float64 reference loss is written out here."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import uplift_upsample_3dhpe_amd as pkg
from tests import util

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

VARIANTS = ["no_temporal_blocks", "no_strided_blocks", "neither", "no_temporal_blocks_no_mask"]


def _variant_cfg(variant, base="h36m_81"):
    """The config of a structural variant, built as test_structural_variants_match_oracle builds it."""
    cfg = util.load_config(base)
    if variant.startswith("no_temporal_blocks") or variant == "neither":
        cfg.TEMPORAL_TRANSFORMER_BLOCKS = 0
    if variant.startswith("no_strided_blocks") or variant == "neither":
        cfg.STRIDES, cfg.PADDINGS = [], []
    if variant == "no_temporal_blocks_no_mask":
        cfg.MASK_STRIDE = None
    return cfg


def _inputs(cfg, arch, B, seed):
    """Keypoints, ground truth and a stride mask (None without strided input) with the central frame real and no all-masked row."""
    rng = np.random.default_rng(seed)
    n = arch.num_frames
    x = rng.uniform(-1, 1, size=(B, n, 17, 2)).astype(np.float32)
    gt = rng.normal(0, 0.3, size=(B, n, 17, 3)).astype(np.float32)
    m = None
    if arch.has_strided_input:
        ms = cfg.MASK_STRIDE if isinstance(cfg.MASK_STRIDE, list) else [cfg.MASK_STRIDE]
        m = np.stack([util.eval_stride_mask(n, cfg.SEQUENCE_STRIDE, ms[b % len(ms)], b % 3) for b in range(B)])
        m[:, n // 2] = True
        assert not m.all()
    return x, gt, m


def _reference(cfg, arch, w, x, m, gt, dp=None, bn_train=None):
    """Loss and d loss / d weights by float64 autograd through oracle.uplift_oracle.forward_torch, with the reference's loss
    including its fallback without a full-sequence output.  Returns (loss, grads, full or None, central)."""
    from oracle import uplift_oracle as O
    f64 = torch.float64
    p = {k: torch.tensor(np.asarray(v), dtype=f64, requires_grad=True) for k, v in w.items()}
    xt = torch.tensor(x, dtype=f64)
    if arch.has_strided_input:
        xt = xt * torch.tensor(m.astype(np.float64))[:, :, None, None]              # train.py:474
    full, central, _ = O.forward_torch(util.hp_from_arch(arch), p, xt, m if arch.has_strided_input else None, f64, dp, None, bn_train, None)
    r = cfg.ROOT_KEYTPOINT
    g = torch.tensor(gt, dtype=f64)
    g = g - g[:, :, r:r + 1, :]
    N, J = g.shape[1], g.shape[2]
    cen = torch.linalg.norm(g[:, N // 2] - central, dim=-1).sum() / (cfg.BATCH_SIZE * J)
    if full is not None:
        seq = torch.linalg.norm(g - full, dim=-1).sum() / (cfg.BATCH_SIZE * N * J)
        loss = cfg.LOSS_WEIGHT_CENTER * cen + cfg.LOSS_WEIGHT_SEQUENCE * seq
    else:
        loss = (cfg.LOSS_WEIGHT_CENTER + cfg.LOSS_WEIGHT_SEQUENCE) * cen           # train.py:491-494
    loss.backward()
    grads = {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in p.items()}
    return float(loss.detach()), grads, None if full is None else full.detach().numpy(), central.detach().numpy()


# the error measure and the flipped-hidden-unit recogniser are shared with tests/test_train_step_rows_gpu.py (tests/util.py)
_bad_tensors, _is_flip = util.bad_tensors, util.is_flip


def _check_against_oracle(cfg, B, seed, droppath=False):
    """Trainer.forward_backward against float64 autograd: loss rel 2e-5, outputs, every gradient tensor <= 1e-4 of its scale; at most
    one flipped hidden unit per weight draw is tolerated (and reported) -- then another weight draw, three at most."""
    from uplift_upsample_3dhpe_amd.trainer import Trainer
    arch = pkg.arch_from_config(cfg)
    x, gt, m = _inputs(cfg, arch, B, seed)
    for attempt in range(3):
        w = pkg.init_weights(arch, seed=seed + 1000 * attempt, perturb=0.1)
        model = pkg.build_uplift_upsample_transformer(cfg, weights=w)
        tr = Trainer(model, cfg)
        u, dp = None, None
        if droppath:
            u = np.random.default_rng(seed + 1).random(tr.drop_path_size(B)).astype(np.float32)
            ns_, nt_ = arch.spatial_depth * 2 * B * arch.num_frames, arch.temporal_depth * 2 * B
            assert u.size == ns_ + nt_ + len(arch.strides) * 2 * B              # stacks that do not exist take no draws
            dp = dict(rates=tuple(cfg.DROP_PATH_RATE), u_spatial=u[:ns_].reshape(arch.spatial_depth, 2, B * arch.num_frames),
                      u_temporal=u[ns_:ns_ + nt_].reshape(arch.temporal_depth, 2, B), u_strided=u[ns_ + nt_:].reshape(len(arch.strides), 2, B))
        loss, full, central = tr.forward_backward(torch.from_numpy(x).cuda(), torch.from_numpy(gt).cuda(),
                                                  None if m is None else torch.from_numpy(m).cuda(),
                                                  drop_path_uniform=None if u is None else torch.from_numpy(u).cuda())
        torch.cuda.synchronize()
        ref_loss, gref, fref, cref = _reference(cfg, arch, w, x, m, gt, dp)
        lv = loss.cpu().numpy()
        assert (full is None) == (fref is None) == (arch.temporal_depth == 0)
        if full is None:
            assert lv[2] == 0.0
        else:
            assert np.abs(full.cpu().numpy() - fref).max() <= util.TOL_MAX_ABS
        assert np.abs(central.cpu().numpy() - cref).max() <= util.TOL_MAX_ABS
        assert float(lv[0]) == pytest.approx(ref_loss, rel=2e-5)
        bad = _bad_tensors(tr.grads_dict(), gref)
        print(f"attempt {attempt}: loss {float(lv[0]):.6f} (float64 {ref_loss:.6f}); tensors over 1e-4: {[(k, '%.1e' % e) for k, e, _ in bad][:6]}")
        if not bad:
            return
        assert _is_flip(bad), [(k, e) for k, e, _ in bad[:8]]
        k0 = bad[0][0] if bad[0][0].endswith("/mlp/fc1/bias") else bad[1][0]
        print(f"      a hidden unit of {k0.rsplit('/', 3)[0]} flips against float64: another weight draw")
    pytest.fail("three weight draws in a row with a flipped hidden unit")


@pytest.mark.parametrize("variant", VARIANTS + ["no_temporal_blocks_droppath", "no_strided_blocks_droppath"])
def test_variant_gradients_match_float64_autograd(variant):
    """Each variant on h36m_81, batch 3, BATCH_SIZE 4, DropPath off (the *_droppath cases: DropPath in every existing stack with explicit
    uniforms, whose layout skips the missing stack)."""
    cfg = _variant_cfg(variant.replace("_droppath", ""))
    cfg.BATCH_SIZE = 4
    droppath = variant.endswith("_droppath")
    cfg.DROP_PATH_RATE = [0.1, 0.1, 0.3] if droppath else [0.0, 0.0, 0.0]
    _check_against_oracle(cfg, B=3, seed=31 + VARIANTS.index(variant.replace("_droppath", "")), droppath=droppath)


def test_output_bn_without_strided_blocks():
    """OUTPUT_BN in training mode without strided blocks: strided_temporal_norm normalises the central tokens (read in place, rows N d_t
    apart) with their batch statistics; the moving statistics after one call match the oracle's, and so do loss and gradients."""
    from uplift_upsample_3dhpe_amd.trainer import Trainer
    cfg = _variant_cfg("no_strided_blocks")
    cfg.BATCH_SIZE, cfg.OUTPUT_BN, cfg.DROP_PATH_RATE = 12, True, [0.0, 0.0, 0.0]
    arch = pkg.arch_from_config(cfg)
    B = 12                                        # (BatchNorm over a few samples multiplies every f32 rounding: see test_train_step_gpu.py)
    x, gt, m = _inputs(cfg, arch, B, seed=41)
    w = pkg.init_weights(arch, seed=41, perturb=0.1)
    model = pkg.build_uplift_upsample_transformer(cfg, weights=w)
    tr = Trainer(model, cfg)
    loss, full, central = tr.forward_backward(torch.from_numpy(x).cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(m).cuda(),
                                              drop_path_uniform=None)
    torch.cuda.synchronize()
    ref_loss, gref, fref, cref = _reference(cfg, arch, w, x, m, gt, bn_train=(moving := {}))
    assert set(moving) == {"temporal_norm/moving_mean", "temporal_norm/moving_variance", "strided_temporal_norm/moving_mean",
                           "strided_temporal_norm/moving_variance"}
    live = tr.params_dict()
    for name, want in moving.items():
        want = want.numpy()
        assert np.abs(live[name] - want).max() <= 2e-5 * max(1.0, np.abs(want).max()), name
        assert np.abs(live[name] - w[name]).max() > 1e-3, name                  # ... and they did move
        assert not tr.grads_dict()[name].any(), name
    assert np.abs(full.cpu().numpy() - fref).max() <= util.TOL_MAX_ABS
    assert np.abs(central.cpu().numpy() - cref).max() <= util.TOL_MAX_ABS
    assert float(loss.cpu()[0]) == pytest.approx(ref_loss, rel=2e-5)
    gref = {k: v for k, v in gref.items() if "/moving_" not in k}
    bad = _bad_tensors(tr.grads_dict(), gref, floor=1e-3)         # (the floor of test_train_step_gpu.py's OUTPUT_BN case)
    assert not bad, [(k, e) for k, e, _ in bad[:8]]


def test_masked_first_strided_block_on_the_long_pair():
    """No temporal blocks at 176 tokens (dense_351 with SEQUENCE_LENGTH 176, STRIDES [4, 11, 4]: 176 -> 44 -> 4 -> 1): strided block 1
    attends over 176 tokens with the stride mask on its keys, on the tiled exact-f32 pair, in both passes."""
    cfg = util.load_config("dense_351")
    cfg.SEQUENCE_LENGTH, cfg.STRIDES, cfg.TEMPORAL_TRANSFORMER_BLOCKS = 176, [4, 11, 4], 0
    cfg.BATCH_SIZE, cfg.DROP_PATH_RATE = 4, [0.0, 0.0, 0.0]
    arch = pkg.arch_from_config(cfg)
    assert arch.num_frames == 176 and arch.has_strided_input and arch.first_strided_token_attention_layer >= 1
    L = [arch.num_frames]
    for s, (pl, pr) in zip(arch.strides, arch.paddings):
        L.append((L[-1] + pl + pr - 3) // s + 1)
    assert L == [176, 44, 4, 1]
    _check_against_oracle(cfg, B=2, seed=51)


def _batch(cfg, arch, B, seed):
    x, gt, m = _inputs(cfg, arch, B, seed)
    if m is not None:
        x = x * m[:, :, None, None].astype(np.float32)
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    return T(x), T(gt), T(m)


@pytest.mark.parametrize("variant", VARIANTS)
def test_adamw_steps_lower_the_loss_and_repeat(variant):
    """Five Trainer.train_step calls (AdamW, DropPath draws from the trainer's generator) on a fixed batch: the loss stays finite and the
    DropPath-free loss of the batch falls; two fresh runs from the same start are bitwise equal."""
    from uplift_upsample_3dhpe_amd.trainer import Trainer
    cfg = _variant_cfg(variant)
    cfg.BATCH_SIZE = 8
    cfg.SCHEDULE_PARAMS = dict(cfg.SCHEDULE_PARAMS, initial_learning_rate=1e-4)
    arch = pkg.arch_from_config(cfg)
    w = pkg.init_weights(arch, seed=61, perturb=0.1)
    x, gt, m = _batch(cfg, arch, 8, seed=61)
    runs = []
    for _ in range(2):
        model = pkg.build_uplift_upsample_transformer(cfg, weights=w)
        tr = Trainer(model, cfg, seed=3)
        l0 = float(tr.forward_backward(x, gt, m, drop_path_uniform=None)[0][0].cpu())
        losses = []
        for _ in range(5):
            losses.append(tr.train_step(x, gt, m).clone())
        l5 = float(tr.forward_backward(x, gt, m, drop_path_uniform=None)[0][0].cpu())
        torch.cuda.synchronize()
        losses = torch.stack(losses).cpu().numpy()
        print(f"{variant}: DropPath-free loss {l0:.6f} -> {l5:.6f}; step losses {losses[:, 0]}")
        assert np.isfinite(losses).all() and not tr.nonfinite()
        if arch.temporal_depth == 0:
            assert (losses[:, 2] == 0).all()
        assert l5 < l0
        runs.append((losses, tr.params.detach().clone(), tr.grads.clone()))
    assert np.array_equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])


@pytest.mark.parametrize("variant", VARIANTS)
def test_custom_loss_restating_the_builtin_step(variant, monkeypatch):
    """UU3D_TRAIN_F32=1: loss.backward() through model(..., training=True) of a torch loss that restates the built-in one (its fallback
    without a full-sequence output included) gives trainer.grads of forward_backward to 1e-6 of each tensor's scale (1e-5 for the q / k
    kernels and biases); without temporal blocks the training call returns full = None.  d x flows as well."""
    from uplift_upsample_3dhpe_amd.trainer import Trainer
    monkeypatch.setenv("UU3D_TRAIN_F32", "1")
    cfg = _variant_cfg(variant)
    cfg.BATCH_SIZE = 4
    arch = pkg.arch_from_config(cfg)
    w = pkg.init_weights(arch, seed=71, perturb=0.1)
    B = 4
    x, gt, m = _batch(cfg, arch, B, seed=71)
    model_a, model_b = pkg.build_uplift_upsample_transformer(cfg, weights=w), pkg.build_uplift_upsample_transformer(cfg, weights=w)
    tr_a, tr_b = Trainer(model_a, cfg, seed=9), Trainer(model_b, cfg, seed=9)
    u = torch.rand(tr_a.drop_path_size(B), generator=tr_a._rng, device="cuda", dtype=torch.float32)
    loss_a, fa, ca = tr_a.forward_backward(x, gt, m, drop_path_uniform=u)
    model_b.requires_grad_()
    tr_b.zero_grad()
    xb = x.clone().requires_grad_()
    fb, cb = model_b([xb, m] if m is not None else xb, training=True)       # draws u from tr_b's generator: the same u
    assert (fa is None) == (fb is None) == (arch.temporal_depth == 0)
    assert torch.equal(ca, cb.detach()) and (fa is None or torch.equal(fa, fb.detach()))
    r = cfg.ROOT_KEYTPOINT
    g = gt - gt[:, :, r:r + 1]
    N, J = g.shape[1], g.shape[2]
    cen = torch.linalg.norm(g[:, N // 2] - cb, dim=-1).sum() / (cfg.BATCH_SIZE * J)
    if fb is None:
        loss = (cfg.LOSS_WEIGHT_CENTER + cfg.LOSS_WEIGHT_SEQUENCE) * cen
    else:
        loss = cfg.LOSS_WEIGHT_CENTER * cen + cfg.LOSS_WEIGHT_SEQUENCE * torch.linalg.norm(g - fb, dim=-1).sum() / (cfg.BATCH_SIZE * N * J)
    loss.backward()
    torch.cuda.synchronize()
    assert float(loss.detach()) == pytest.approx(float(loss_a[0]), rel=1e-6)
    assert tr_b.params.grad is tr_b.grads
    assert xb.grad is not None and torch.isfinite(xb.grad).all() and xb.grad.abs().max() > 0
    if m is not None:
        assert not xb.grad[~m.bool()].any()                   # frames the stride mask discards
    ga, gb = tr_a.grads_dict(), tr_b.grads_dict()
    gmax = max(np.abs(v).max() for v in ga.values())
    errs = []
    for k in ga:
        scale = max(np.abs(ga[k]).max(), 1e-4 * gmax)
        if k.endswith("/attn/wk/bias"):          # zero up to rounding (softmax shift invariance): its natural scale is the key kernel's gradient
            scale = max(scale, np.abs(ga[k.replace("/bias", "/kernel")]).max())
        errs.append((float(np.abs(gb[k] - ga[k]).max() / scale), k))
    errs.sort(reverse=True)
    print(f"{variant}: custom loss vs built-in step, worst {[(k, '%.1e' % e) for e, k in errs[:5]]}")
    # torch's norm backward and the loss kernel round the cotangents differently in the last bit; the softmax backward amplifies that in
    # the q / k gradients to a few 1e-6 (measured <= 2.7e-6), every other tensor stays below 1e-6
    assert errs[0][0] <= 1e-5, errs[:5]
    assert max(e for e, k in errs if "/attn/wq/" not in k and "/attn/wk/" not in k) <= 1e-6, errs[:5]


def test_no_temporal_blocks_on_two_ranks(tmp_path):
    """Variant (a) on two ranks sharing cuda:0 over gloo (tests/structural_dist2_worker.py; the time limits of
    tests/test_autograd_dist2_gpu.py): the reporting backward pass plus the step equals one flat all-reduce plus the step, bit for bit."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, PYTHONPATH=util.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(util.ROOT, "tests", "structural_dist2_worker.py"), str(r), "2", str(port),
                               str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=900)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o)
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-3000:] for l in logs)
    res = [json.load(open(os.path.join(tmp_path, f"rank{r}.json"))) for r in range(2)]
    for r in res:
        assert r["full_is_none"] and r["buckets"] >= 2 and r["ranges_tile_the_buffer"], r
        assert r["grads_equal_flat"] and r["params_equal_reference"], r
        assert r["params_moved"] and r["not_skipped"] and r["replicas_identical"], r
    assert res[0]["crc"] == res[1]["crc"]
