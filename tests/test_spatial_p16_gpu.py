"""GPU tests of spatial_stack_p16_kernel (csrc/uu3d_spatial_p16.h), the inference spatial stack on 16-token panels:
against the 32-token-tile kernel it replaced (UU3D_SPATIAL=h3tiles) and the oracle, slot independence of a frame inside
a workgroup, and weights re-committed."""
import numpy as np
import pytest

import uplift_upsample_3dhpe_amd as pkg
from tests import util

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _call(model, x, m):
    full, cen = model([torch.as_tensor(x).cuda(), torch.as_tensor(m).cuda()], training=False)
    torch.cuda.synchronize()
    return full.cpu().numpy(), cen.cpu().numpy()


def _batch(cfg, batch, seed, mask_stride=None):
    specs = None if mask_stride is None else [(mask_stride, 0), (mask_stride, cfg.SEQUENCE_STRIDE)]
    x, m = util.synthetic_batch(cfg, batch, seed=seed, mask_specs=specs)
    return x * m[:, :, None, None], m


@pytest.mark.parametrize("cfgname,batch,mask_stride", [("h36m_351", 128, None), ("h36m_81", 256, None),
                                                       ("h36m_351", 32, 10), ("h36m_351", 32, 20)])
def test_panels_match_tiles_and_oracle(cfgname, batch, mask_stride, monkeypatch):
    from oracle import uplift_oracle as O
    cfg = util.load_config(cfgname)
    arch = pkg.arch_from_config(cfg)
    w = pkg.init_weights(arch, seed=7, perturb=0.1)
    x, m = _batch(cfg, batch, 7, mask_stride)
    f, c = _call(pkg.build_uplift_upsample_transformer(cfg, weights=w), x, m)
    monkeypatch.setenv("UU3D_SPATIAL", "h3tiles")
    ft, ct = _call(pkg.build_uplift_upsample_transformer(cfg, weights=w), x, m)
    monkeypatch.delenv("UU3D_SPATIAL")
    assert np.isfinite(f).all() and np.isfinite(c).all()
    d = max(np.abs(f - ft).max(), np.abs(c - ct).max())
    print(f"{cfgname} x {batch} (s_in {mask_stride}): panels vs tiles {d:.3e}")
    assert 0.0 < d <= 3e-5, d
    idx = np.array([0, 1, batch // 2, batch - 1])
    fo, co = O.forward(util.hp_from_arch(arch), w, x[idx], m[idx], torch.float32)
    assert np.abs(f[idx] - fo).max() <= util.TOL_MAX_ABS and np.abs(c[idx] - co).max() <= util.TOL_MAX_ABS


def test_frame_result_does_not_depend_on_its_slot():
    """h36m_81: 81 = 4 (mod 7), so sequence r of a batch starts at slot 4 r (mod 7) of a 7-frame workgroup; batches of 1 .. 7
    that end in the same sequence put each of its frames at every slot, the batch of one in a partial last workgroup."""
    cfg = util.load_config("h36m_81")
    arch = pkg.arch_from_config(cfg)
    model = pkg.build_uplift_upsample_transformer(cfg, weights=pkg.init_weights(arch, seed=8, perturb=0.1))
    x, m = _batch(cfg, 7, 8)
    m[:] = True                                             # dense: no compaction, the slot arithmetic above holds
    f1, c1 = _call(model, x[6:7], m[6:7])
    for b in range(2, 8):
        f, c = _call(model, x[7 - b:], m[7 - b:])
        assert np.array_equal(f[-1], f1[0]) and np.array_equal(c[-1], c1[0]), b


def test_recommitted_weights_reach_the_panels():
    from oracle import uplift_oracle as O
    cfg = util.load_config("h36m_81")
    arch = pkg.arch_from_config(cfg)
    w1, w2 = (pkg.init_weights(arch, seed=s, perturb=0.1) for s in (9, 10))
    model = pkg.build_uplift_upsample_transformer(cfg, weights=w1)
    x, m = _batch(cfg, 3, 9)
    for w in (w1, w2, w1):
        model.set_weights_dict(w)
        f, c = _call(model, x, m)
        fo, co = O.forward(util.hp_from_arch(arch), w, x, m, torch.float32)
        assert max(np.abs(f - fo).max(), np.abs(c - co).max()) <= util.TOL_MAX_ABS
