"""GPU: ForwardPipeline(exact_f32=True) and eval.predict_windows(exact_f32=True) -- every forward of a pipeline on the exact-f32 kernels
(UU3D_SCHEDULE_EXACT_F32 OR-ed into the slot's schedule), the way out after the Uu3dRangeError a pipeline's check_range() raises for weights
whose activations leave the f16 range.  At 41 tokens (h36m_81: the register-resident exact-f32 attention) and at 130 (the tiled one)."""
import warnings

import numpy as np
import pytest

import uplift_upsample_3dhpe_amd as pkg
from uplift_upsample_3dhpe_amd import _capi
from uplift_upsample_3dhpe_amd import data as D
from tests import util

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
BATCH = 6
CASES = ["h36m_81", "dense_130"]


def _config(name):
    if name == "dense_130":
        cfg = util.load_config("dense_351")
        cfg.SEQUENCE_LENGTH, cfg.STRIDES = 130, [2, 5, 13]
        return cfg
    return util.load_config(name)


def _overflowing_weights(arch, scale=3.0e4, block="temporal_block_2"):
    """tests/test_range_guard_gpu.py's: hidden activations of one block `scale` times larger, the same function in exact arithmetic."""
    w = dict(pkg.init_weights(arch, seed=2, perturb=0.1))
    w[block + "/mlp/fc1/kernel"] = w[block + "/mlp/fc1/kernel"] * np.float32(scale)
    w[block + "/mlp/fc1/bias"] = w[block + "/mlp/fc1/bias"] * np.float32(scale)
    w[block + "/mlp/fc2/kernel"] = w[block + "/mlp/fc2/kernel"] / np.float32(scale)
    return w


@pytest.fixture(scope="module", params=CASES)
def case(request):
    """Config, overflowing weights, one batch, the float32 oracle's answer and the model -- computed once per config."""
    from oracle import uplift_oracle as O
    cfg = _config(request.param)
    arch = pkg.arch_from_config(cfg)
    w = _overflowing_weights(arch)
    x, m = util.synthetic_batch(cfg, batch=BATCH, seed=3)
    xm = x * m[:, :, None, None].astype(np.float32)
    f32, c32 = O.forward(util.hp_from_arch(arch), w, xm, m, torch.float32)
    model = pkg.build_uplift_upsample_transformer(cfg, weights=w)
    return dict(name=request.param, cfg=cfg, arch=arch, w=w, xt=torch.from_numpy(xm).cuda(), mt=torch.from_numpy(m).cuda(), f32=f32, c32=c32, model=model)


def _oracle_error(case, full, cen):
    scale = max(np.abs(case["f32"]).max(), np.abs(case["c32"]).max())
    err = max(np.abs(full.cpu().numpy() - case["f32"]).max(), np.abs(cen.cpu().numpy() - case["c32"]).max())
    return err, 1e-4 * max(1.0, scale)                         # tests/test_range_guard_gpu.py's measure of the fallback


def test_one_slot_returns_the_bits_of_the_direct_exact_f32_call(case):
    model, xt, mt = case["model"], case["xt"], case["mt"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        full, cen = model([xt, mt], training=False)            # overflows, repeated on the exact-f32 kernels
        torch.cuda.synchronize()
    assert model._range_warned and bool(torch.isfinite(full).all()) and bool(torch.isfinite(cen).all())
    for graph in (True, False):
        pipe = model.pipeline(BATCH, depth=1, graph=graph, exact_f32=True)
        f1, c1 = pipe.result(pipe.submit(xt, mt))
        torch.cuda.synchronize()
        assert torch.equal(f1, full) and torch.equal(c1, cen)
        assert pipe.check_range() is False                     # nothing to find: no f16x3 forward ran
        pipe.close()


@pytest.mark.parametrize("graph", [True, False])
def test_two_slots_match_the_oracle(case, graph):
    model, xt, mt = case["model"], case["xt"], case["mt"]
    pipe = model.pipeline(BATCH, depth=2, graph=graph, exact_f32=True)
    outs = []
    for full, cen in pipe.run([(xt, mt)] * 3):
        torch.cuda.synchronize()
        outs.append((full.clone(), cen.clone()))
    assert pipe.check_range() is False
    pipe.close()
    for full, cen in outs:
        err, bar = _oracle_error(case, full, cen)
        print(f"{case['name']} depth 2 graph {graph}: exact-f32 pipeline vs oracle {err:.3e} (bar {bar:.1e})")
        assert bool(torch.isfinite(full).all()) and err <= bar
        assert torch.equal(full, outs[0][0]) and torch.equal(cen, outs[0][1])


def test_the_default_pipeline_still_raises(case):
    model, xt, mt = case["model"], case["xt"], case["mt"]
    pipe = model.pipeline(BATCH, depth=2)
    assert pipe.exact_f32 is False
    for _ in range(2):
        pipe.result(pipe.submit(xt, mt))
    with pytest.raises(_capi.Uu3dRangeError):
        pipe.check_range()
    pipe.close()
    assert model.check_range(raise_error=False) is False


def _tracks(cfg, seed):
    rng = np.random.default_rng(seed)
    lens = (300, 290)
    p2 = [rng.uniform(-1, 1, size=(n, 17, 2)).astype(np.float32) for n in lens]
    table = D.PoseTable(p2)
    ms = cfg.MASK_STRIDE[0] if isinstance(cfg.MASK_STRIDE, list) else cfg.MASK_STRIDE
    gen = D.SequenceGenerator(table, seq_len=cfg.SEQUENCE_LENGTH, stride=cfg.SEQUENCE_STRIDE, padding_type=cfg.PADDING_TYPE, flip_augment=False,
                              flip_lr_indices=cfg.AUGM_FLIP_KEYPOINT_ORDER, mask_stride=ms, stride_mask_align_global=True, shuffle=False)
    return gen, gen.descriptors()[::6]                         # ~100 windows of both tracks, padded ones at the ends included


@pytest.mark.parametrize("reuse", [False, True])
def test_predict_windows_exact_f32_where_the_default_raises(case, reuse):
    from uplift_upsample_3dhpe_amd import eval as ev
    cfg, model = case["cfg"], case["model"]
    gen, desc = _tracks(cfg, 7)
    with pytest.raises(_capi.Uu3dRangeError, match="exact_f32=True"):
        ev.predict_windows(model, gen, desc, cfg, 16, flip=True, depth=2, reuse_frames=reuse)
    assert model.check_range(raise_error=False) is False
    pred = ev.predict_windows(model, gen, desc, cfg, 16, flip=True, depth=2, reuse_frames=reuse, exact_f32=True)
    torch.cuda.synchronize()
    assert pred.shape == (len(desc), 17, 3) and bool(torch.isfinite(pred).all())
    again = ev.predict_windows(model, gen, desc, cfg, 16, flip=True, depth=2, reuse_frames=reuse, exact_f32=True)
    assert torch.equal(pred, again)
    eager = ev.predict_windows(model, gen, desc, cfg, 16, flip=True, depth=1, graph=False, reuse_frames=reuse, exact_f32=True)
    assert bool(torch.isfinite(eager).all())                   # (depth 1 without a graph: still through a pipeline, with the bit set)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("reuse", [False, True])
def test_predict_windows_exact_f32_agrees_with_the_default_on_ordinary_weights(name, reuse):
    from uplift_upsample_3dhpe_amd import eval as ev
    cfg = _config(name)
    arch = pkg.arch_from_config(cfg)
    model = pkg.build_uplift_upsample_transformer(cfg, weights=pkg.init_weights(arch, seed=3, perturb=0.1))
    gen, desc = _tracks(cfg, 8)
    a = ev.predict_windows(model, gen, desc, cfg, 16, flip=True, depth=2, reuse_frames=reuse)
    b = ev.predict_windows(model, gen, desc, cfg, 16, flip=True, depth=2, reuse_frames=reuse, exact_f32=True)
    torch.cuda.synchronize()
    err = (a - b).abs().max().item()
    print(f"{name} reuse {reuse}: exact-f32 evaluation vs the default {err:.2e} over {len(desc)} windows")
    assert 0.0 < err <= util.TOL_MAX_ABS
