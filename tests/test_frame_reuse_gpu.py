"""GPU: the frames form of the forward (include/uu3d.h, FRAMES FORM) and eval.predict_windows(reuse_frames=True).

The spatial stack and spatial_to_temporal_fc of a frame do not depend on the window the frame sits in, so evaluation can compute them once
per frame (uu3d_frame_features) and forward the windows from a feature table (uu3d_gather_window_frames + uu3d_forward_frames_ex).  Checked
here: the table rows name exactly the frames uu3d_gather_windows copies, the frames form agrees with uu3d_forward_ex on the same windows
(~3e-5: the s2t GEMM sums in another split-K order) and with the oracle, evaluation with reuse agrees with the default, the range guard
holds, and new weights are picked up."""
import ctypes as C
import warnings

import numpy as np
import pytest

import uplift_upsample_3dhpe_amd as pkg
from uplift_upsample_3dhpe_amd import _capi
from uplift_upsample_3dhpe_amd import data as D
from tests import util

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
FLIP = [5, 4, 3, 2, 1, 0, 6, 7, 8, 9, 10, 16, 15, 14, 13, 12, 11]


def _videos(seed, lens, J=17):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1, 1, size=(n, J, 2)).astype(np.float32) for n in lens], \
           [rng.normal(0, 0.4, size=(n, J, 3)).astype(np.float32) for n in lens]


def _rows(table, desc, N, pad_edge, frame_base, zero_row, video_start=None, zero_masked=1):
    lib = _capi.load_library()
    B = len(desc)
    d = torch.from_numpy(np.ascontiguousarray(desc, np.int32)).cuda()
    vs = table.d_starts if video_start is None else torch.from_numpy(np.asarray(video_start, np.int64)).cuda()
    rows = torch.empty((B, N), dtype=torch.int32, device="cuda")
    sm = torch.empty((B, N), dtype=torch.uint8, device="cuda")
    pm = torch.empty((B, N), dtype=torch.uint8, device="cuda")
    st = lib.uu3d_gather_window_frames(C.c_void_p(vs.data_ptr()), C.c_void_p(table.d_lens.data_ptr()), C.c_void_p(d.data_ptr()), B, N,
                                       int(pad_edge), int(zero_masked), int(frame_base), int(zero_row), C.c_void_p(rows.data_ptr()),
                                       C.c_void_p(sm.data_ptr()), C.c_void_p(pm.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _capi.check(lib, st, None)
    torch.cuda.synchronize()
    return rows.cpu().numpy(), sm.cpu().numpy(), pm.cpu().numpy()


@pytest.mark.parametrize("mode", [
    dict(seq_len=71, stride=5, padding_type="copy", mask_stride=10, stride_mask_align_global=True, flip_augment=True),
    dict(seq_len=41, stride=2, padding_type="zeros", mask_stride=[4, 8], rand_shift_stride_mask=True, flip_augment=True, in_batch_augment=True),
    dict(seq_len=27, stride=3, padding_type="zeros", mask_stride=9, stride_mask_align_global=True, flip_augment=False),
    dict(seq_len=9, stride=1, padding_type="copy", mask_stride=None, flip_augment=True),
])
def test_frame_rows_name_the_frames_gather_windows_copies(mode):
    """Poses whose x coordinate is (global frame id + 1): the frame uu3d_gather_windows copies into a token can be read off its output."""
    lens = (3, 40, 97, 260, 7)                                  # windows longer than their video included
    J = 17
    poses = []
    off = 0
    for n in lens:
        p = np.zeros((n, J, 2), np.float32)
        p[:, :, 0] = (off + np.arange(n) + 1)[:, None]
        p[:, :, 1] = np.arange(J)[None, :]
        poses.append(p); off += n
    table = D.PoseTable(poses, frame_rates=[50, 100, 50, 50, 100])
    gen = D.SequenceGenerator(table, flip_lr_indices=FLIP, shuffle=True, seed=2, **mode)
    desc = gen.descriptors()
    N = mode["seq_len"]
    F = int(table.lens.sum())
    for shift in (0, 37):                                       # video starts shifted (the table holds frames at an offset)
        vs, base, zrow = table.starts + shift, F + shift, 2 * (F + shift)
        rows, sm, pm = _rows(table, desc, N, gen.pad_edge, frame_base=base, zero_row=zrow, video_start=vs)
        for zm in (1, 0):
            out = gen.gather(desc, zero_masked=bool(zm), with_3d=False)
            k = out["kp2d"].cpu().numpy()
            assert np.array_equal(sm, out["stride_mask"].cpu().numpy()) and np.array_equal(pm, out["mask"].cpu().numpy())
            if zm == 0:
                rows0, _, _ = _rows(table, desc, N, gen.pad_edge, frame_base=base, zero_row=zrow, video_start=vs, zero_masked=0)
                assert (rows0 >= 0).all()
                r = rows0
            else:
                r = rows
                assert np.array_equal(r < 0, sm == 0)           # -1 exactly where the mask drops the token
            x = k[..., 0, 0]                                    # (+-(id + 1)) or 0
            flip = desc[:, 5:6].astype(bool) & np.ones_like(r, bool)
            real = r >= 0
            zero = r == zrow
            assert np.array_equal(x[zero], np.zeros(zero.sum(), np.float32))
            assert np.array_equal(pm[zero], np.zeros(zero.sum(), np.uint8))
            got = r - np.where(flip, base, 0) - shift           # the global frame id the row names
            want = np.abs(x) - 1
            sel = real & ~zero
            assert np.array_equal(got[sel], want[sel].astype(np.int64))
            assert np.array_equal(np.sign(x[sel]) < 0, flip[sel])


def _feature_table(model, table, flip_order):
    """Every frame of the pose table: rows [0, F) plain, [F, 2F) flipped, 2F the all-zero frame."""
    kp = table.kp2d
    order = torch.as_tensor(np.asarray(flip_order), dtype=torch.long, device=kp.device)
    fl = kp.index_select(1, order).clone()
    fl[..., 0] = -fl[..., 0]
    frames = torch.cat([kp, fl, torch.zeros_like(kp[:1])], 0)
    return model.frame_features(frames)


def _direct_frames(model, feats, rows, m, schedule, attn=None):
    a = model.arch
    B = rows.shape[0]
    full = torch.empty((B, a.num_frames, a.num_keypoints, 3), dtype=torch.float32, device="cuda") if model._returns_full else None
    cen = torch.empty((B, a.num_keypoints, 3), dtype=torch.float32, device="cuda")
    model._forward_frames(feats, rows, m, full, cen, 0, torch.cuda.current_stream(), schedule=schedule, attn=attn)
    torch.cuda.synchronize()
    return full, cen


@pytest.mark.parametrize("cfgname,msv,batch", [("h36m_351", 5, 8), ("h36m_351", 10, 32), ("h36m_351", 20, 16), ("h36m_81", 4, 40),
                                               ("h36m_81", 10, 6), ("dense_351", 20, 4), ("dense_351", 5, 2)])
def test_forward_frames_matches_the_window_forward(cfgname, msv, batch):
    from oracle import uplift_oracle as O
    cfg = util.load_config(cfgname)
    arch = pkg.arch_from_config(cfg)
    w = pkg.init_weights(arch, seed=4, perturb=0.1)
    model = pkg.build_uplift_upsample_transformer(cfg, weights=w)
    N = cfg.SEQUENCE_LENGTH
    p2, _ = _videos(1, (N // 3, 2 * N, 5 * N))
    table = D.PoseTable(p2)
    gen = D.SequenceGenerator(table, seq_len=N, stride=cfg.SEQUENCE_STRIDE, padding_type=cfg.PADDING_TYPE, flip_augment=True,
                              flip_lr_indices=cfg.AUGM_FLIP_KEYPOINT_ORDER, mask_stride=msv, stride_mask_align_global=True, shuffle=True, seed=5)
    desc = gen.descriptors()[:batch]
    F = int(table.lens.sum())
    feats = _feature_table(model, table, cfg.AUGM_FLIP_KEYPOINT_ORDER)
    b = gen.gather(desc, zero_masked=True, with_3d=False)
    xt, mt = b["kp2d"], b["stride_mask"]
    rows, sm, _ = _rows(table, desc, N, gen.pad_edge, F, 2 * F)
    assert np.array_equal(sm, mt.cpu().numpy())
    rt = torch.from_numpy(rows).cuda()
    for schedule in (0, 1):
        f0, c0 = util.direct_forward(model, xt, mt, schedule)
        f1, c1 = _direct_frames(model, feats, rt, mt, schedule)
        f2, c2 = _direct_frames(model, feats, rt, mt, schedule)
        assert torch.equal(c1, c2) and (f1 is None or torch.equal(f1, f2))                     # bitwise run to run
        err = (c1 - c0).abs().max().item()
        if f1 is not None:
            err = max(err, (f1 - f0).abs().max().item())
        print(f"{cfgname} mask stride {msv} batch {batch} ({batch * N} rows) schedule {schedule}: frames vs windows {err:.2e}")
        assert err <= 3e-5
    assert model.check_range(raise_error=False) is False
    n = min(batch, 2 if cfgname == "dense_351" else 4)
    xm = xt[:n].cpu().numpy()
    f32, c32 = O.forward(util.hp_from_arch(arch), w, xm, mt[:n].cpu().numpy().astype(bool), torch.float32)
    err = np.abs(c1[:n].cpu().numpy() - c32).max()
    if f1 is not None:
        err = max(err, np.abs(f1[:n].cpu().numpy() - f32).max())
    assert err <= util.TOL_MAX_ABS, err


def test_forward_frames_attention_maps():
    cfg = util.load_config("h36m_351")
    arch = pkg.arch_from_config(cfg)
    model = pkg.build_uplift_upsample_transformer(cfg, weights=pkg.init_weights(arch, seed=7, perturb=0.1), return_attention=True)
    N = cfg.SEQUENCE_LENGTH
    p2, _ = _videos(2, (N, 3 * N))
    table = D.PoseTable(p2)
    gen = D.SequenceGenerator(table, seq_len=N, stride=cfg.SEQUENCE_STRIDE, padding_type="copy", flip_augment=True,
                              flip_lr_indices=cfg.AUGM_FLIP_KEYPOINT_ORDER, mask_stride=10, stride_mask_align_global=True, shuffle=True, seed=1)
    desc = gen.descriptors()[:6]
    F = int(table.lens.sum())
    feats = _feature_table(model, table, cfg.AUGM_FLIP_KEYPOINT_ORDER)
    b = gen.gather(desc, zero_masked=True, with_3d=False)
    rows, _, _ = _rows(table, desc, N, True, F, 2 * F)
    f0, c0, a0 = model([b["kp2d"], b["stride_mask"]], training=False)
    f1, c1, a1 = model.forward_frames(feats, torch.from_numpy(rows).cuda(), b["stride_mask"])
    torch.cuda.synchronize()
    assert len(a0) == len(a1) == arch.temporal_depth
    assert max((x - y).abs().max().item() for x, y in zip(a0, a1)) <= 3e-5
    assert (c0 - c1).abs().max().item() <= 3e-5


def _report(cfg, table, desc, pred):
    from uplift_upsample_3dhpe_amd import evaluation
    mid = desc[:, 1].astype(np.int64) + table.starts[desc[:, 0]]
    gt = table.kp3d[torch.as_tensor(mid, device=table.device)].cpu().numpy().astype(np.float64)
    gt = gt - gt[:, cfg.ROOT_KEYTPOINT:cfg.ROOT_KEYTPOINT + 1, :]
    return evaluation.evaluate_predictions(pred.cpu().numpy().astype(np.float64), gt, table.actions[desc[:, 0]], desc[:, 1].copy(), cfg,
                                           action_wise=False)


@pytest.mark.parametrize("cfgname,msv,flip,depth,graph,table_bytes", [
    ("h36m_351", 5, True, None, True, None), ("h36m_351", 10, False, 1, False, None), ("h36m_351", 20, True, 1, False, 600_000),
    ("h36m_81", 4, True, None, True, 400_000), ("h36m_81", 20, False, None, True, None)])
def test_predict_windows_with_reuse_matches_the_default(cfgname, msv, flip, depth, graph, table_bytes):
    from uplift_upsample_3dhpe_amd import eval as ev
    cfg = util.load_config(cfgname)
    cfg.MASK_STRIDE = msv
    arch = pkg.arch_from_config(cfg)
    model = pkg.build_uplift_upsample_transformer(cfg, weights=pkg.init_weights(arch, seed=3, perturb=0.1))
    N = cfg.SEQUENCE_LENGTH
    p2, p3 = _videos(3, (N // 4, 40, 3 * N, 7 * N, 2 * N + 3))          # some videos shorter than a window
    table = D.PoseTable(p2, p3, actions=[0, 3, 3, 14, 2])
    gen = D.SequenceGenerator(table, seq_len=N, stride=cfg.SEQUENCE_STRIDE, padding_type=cfg.PADDING_TYPE, flip_augment=False,
                              flip_lr_indices=cfg.AUGM_FLIP_KEYPOINT_ORDER, mask_stride=msv, stride_mask_align_global=True, shuffle=False)
    desc = gen.descriptors()
    run = desc[ev.needed_windows(desc[:, 1], cfg)]
    kw = {} if table_bytes is None else dict(frame_table_bytes=table_bytes)     # (small tables: several chunks)
    a = ev.predict_windows(model, gen, run, cfg, 48, flip=flip, depth=depth, graph=graph)
    b = ev.predict_windows(model, gen, run, cfg, 48, flip=flip, depth=depth, graph=graph, reuse_frames=True, **kw)
    b2 = ev.predict_windows(model, gen, run, cfg, 48, flip=flip, depth=depth, graph=graph, reuse_frames=True, **kw)
    torch.cuda.synchronize()
    assert torch.equal(b, b2)
    err = (a - b).abs().max().item()
    print(f"{cfgname} mask stride {msv} flip {flip} depth {depth}: reuse vs default {err:.2e} over {len(run)} windows")
    assert err <= 3e-5
    ra, rb = _report(cfg, table, run, a), _report(cfg, table, run, b)
    for k in ra["all_frames"]:
        assert rb["all_frames"][k] == pytest.approx(ra["all_frames"][k], rel=1e-5)


def _overflowing_weights(arch, scale=3.0e4, block="temporal_block_2"):
    w = dict(pkg.init_weights(arch, seed=2, perturb=0.1))
    w[block + "/mlp/fc1/kernel"] = w[block + "/mlp/fc1/kernel"] * np.float32(scale)
    w[block + "/mlp/fc1/bias"] = w[block + "/mlp/fc1/bias"] * np.float32(scale)
    w[block + "/mlp/fc2/kernel"] = w[block + "/mlp/fc2/kernel"] / np.float32(scale)
    return w


def test_range_guard_in_the_frames_form():
    from oracle import uplift_oracle as O
    from uplift_upsample_3dhpe_amd import eval as ev
    cfg = util.load_config("h36m_351")
    cfg.MASK_STRIDE = 10
    arch = pkg.arch_from_config(cfg)
    w = _overflowing_weights(arch)
    model = pkg.build_uplift_upsample_transformer(cfg, weights=w)
    N = cfg.SEQUENCE_LENGTH
    p2, _ = _videos(4, (2 * N, 3 * N))
    table = D.PoseTable(p2)
    gen = D.SequenceGenerator(table, seq_len=N, stride=cfg.SEQUENCE_STRIDE, padding_type="copy", flip_augment=False,
                              flip_lr_indices=cfg.AUGM_FLIP_KEYPOINT_ORDER, mask_stride=10, stride_mask_align_global=True, shuffle=False)
    desc = gen.descriptors()
    with pytest.raises(_capi.Uu3dRangeError):
        ev.predict_windows(model, gen, desc[::5], cfg, 16, flip=True, depth=2, reuse_frames=True)
    assert model.check_range(raise_error=False) is False
    # a direct forward_frames repeats the overflowed batch in exact f32
    F = int(table.lens.sum())
    feats = _feature_table(model, table, cfg.AUGM_FLIP_KEYPOINT_ORDER)
    d = desc[::37][:5]
    b = gen.gather(d, zero_masked=True, with_3d=False)
    rows, _, _ = _rows(table, d, N, True, F, 2 * F)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        full, cen = model.forward_frames(feats, torch.from_numpy(rows).cuda(), b["stride_mask"])
        torch.cuda.synchronize()
    assert any("f16 range" in str(r.message) for r in rec) or model._range_warned
    xm, m = b["kp2d"].cpu().numpy(), b["stride_mask"].cpu().numpy().astype(bool)
    f32, c32 = O.forward(util.hp_from_arch(arch), w, xm, m, torch.float32)
    full, cen = full.cpu().numpy(), cen.cpu().numpy()
    assert np.isfinite(full).all() and np.isfinite(cen).all()
    scale = max(np.abs(f32).max(), np.abs(c32).max())
    assert max(np.abs(full - f32).max(), np.abs(cen - c32).max()) <= 1e-4 * max(1.0, scale)
    assert model.check_range(raise_error=False) is False


def test_new_weights_are_picked_up():
    from uplift_upsample_3dhpe_amd import eval as ev
    cfg = util.load_config("h36m_81")
    cfg.MASK_STRIDE = 4
    arch = pkg.arch_from_config(cfg)
    N = cfg.SEQUENCE_LENGTH
    p2, _ = _videos(5, (3 * N, 40))
    table = D.PoseTable(p2)
    gen = D.SequenceGenerator(table, seq_len=N, stride=cfg.SEQUENCE_STRIDE, padding_type="copy", flip_augment=False,
                              flip_lr_indices=cfg.AUGM_FLIP_KEYPOINT_ORDER, mask_stride=4, stride_mask_align_global=True, shuffle=False)
    desc = gen.descriptors()[::2]
    w1, w2 = pkg.init_weights(arch, seed=1, perturb=0.1), pkg.init_weights(arch, seed=9, perturb=0.1)
    model = pkg.build_uplift_upsample_transformer(cfg, weights=w1)
    a = ev.predict_windows(model, gen, desc, cfg, 32, flip=True, reuse_frames=True)
    model.set_weights_dict(w2)
    b = ev.predict_windows(model, gen, desc, cfg, 32, flip=True, reuse_frames=True)
    fresh = pkg.build_uplift_upsample_transformer(cfg, weights=w2)
    c = ev.predict_windows(fresh, gen, desc, cfg, 32, flip=True, reuse_frames=True)
    torch.cuda.synchronize()
    assert not torch.equal(a, b)
    assert torch.equal(b, c)
