"""GPU: predict.predict_tracks -- 3D poses for the caller's own 2D keypoint tracks -- and its two kernels (csrc/uu3d_tracks.h).

Both kernels reproduce the host's dtypes and operation order (numpy's float32 / float64 mix of ``h36m.normalize_screen_coordinates``; the two
float64 products and one sum of ``evaluation.interpolate_between_keyframes``, rounded to float32 on store), so every comparison against those
host functions below asserts BITWISE equality, on interpolated frames too, instead of an ulp bound."""
import os

import numpy as np
import pytest

import uplift_upsample_3dhpe_amd as pkg
from tests import util
from tests.tracks_util import RES, _bits, _host_normalised, _model, _oracle_tracks, _pixel_tracks, _same_bits  # noqa: F401 (test_track_fps_gpu reads them here)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
G = os.path.join(util.ROOT, "tests", "golden")
MASK_STRIDE = {"h36m_351": 5, "h36m_81": 4}


def test_normalize_tracks_equals_the_host_rule_bitwise():
    from uplift_upsample_3dhpe_amd import predict
    lens = [13, 40, 1]                                                # 54 rows x 17 joints: an even number of pairs; [13, 40]: an odd one (8-byte tail)
    for ls in (lens, lens[:2]):
        tracks = _pixel_tracks(ls, seed=1)
        want = np.concatenate(_host_normalised(tracks), 0)
        res = [RES[i % len(RES)] for i in range(len(ls))]
        table, got_lens = predict.pose_table(tracks, "cuda", resolutions=res)
        assert list(got_lens) == ls and _same_bits(table.kp2d, want)
        dev_tracks = [torch.from_numpy(t).cuda() for t in tracks]        # device input: the caller's tensors are not written
        table2, _ = predict.pose_table(dev_tracks, "cuda", resolutions=res)
        assert _same_bits(table2.kp2d, want) and all(_same_bits(d, t) for d, t in zip(dev_tracks, tracks))
        # keyframes only: the same launch scatters them into the dense table and writes zeros elsewhere
        for s in (4, 5):
            keys = [t[::s] for t in tracks]
            table3, l3 = predict.pose_table(keys, "cuda", resolutions=res, key_stride=s, lengths=ls)
            dense = np.concatenate([np.where((np.arange(len(w_)) % s == 0)[:, None, None], w_, 0.0).astype(np.float32)
                                    for w_ in _host_normalised(tracks)], 0)
            assert list(l3) == ls and _same_bits(table3.kp2d, dense)
    # one (w, h) for all tracks, and no resolution at all (already normalised: the table is the input)
    tracks = _pixel_tracks([9, 9], seed=2)
    from uplift_upsample_3dhpe_amd import h36m
    table, _ = predict.pose_table(tracks, "cuda", resolutions=(1920, 1080))
    assert _same_bits(table.kp2d, np.concatenate([h36m.normalize_screen_coordinates(t, w=1920, h=1080).astype(np.float32) for t in tracks], 0))
    table, _ = predict.pose_table(tracks, "cuda")
    assert _same_bits(table.kp2d, np.concatenate(tracks, 0))


@pytest.mark.parametrize("stride,flip", [(5, True), (2, True), (5, False)])
def test_assemble_tracks_alone(stride, flip):
    """Random central predictions for tracks of 1, 37 and 1200 frames against un-flip + average in numpy float32 followed by
    evaluation.interpolate_between_keyframes on the same arrays: bitwise on predicted AND interpolated frames (the kernel computes the
    host's float64 expression and rounds once, as numpy does when it stores into the float32 array)."""
    from uplift_upsample_3dhpe_amd import evaluation, predict
    cfg = util.load_config("h36m_351")
    order, root, J = np.asarray(cfg.AUGM_FLIP_KEYPOINT_ORDER), cfg.ROOT_KEYTPOINT, 17
    lens = [1, 37, 1200]
    idx = np.concatenate([np.arange(n) for n in lens])
    run = np.flatnonzero(idx % stride == 0)
    W, P = len(run), len(idx)
    rng = np.random.default_rng(3)
    plain = rng.normal(size=(W, J, 3)).astype(np.float32)
    flipped = rng.normal(size=(W, J, 3)).astype(np.float32)
    avg = plain
    if flip:
        f = np.concatenate([flipped[..., :1] * np.float32(-1.0), flipped[..., 1:]], axis=-1)[:, order]
        avg = (plain + f) / np.float32(2.0)
        assert avg.dtype == np.float32
    pred = np.zeros((P, J, 3), np.float32)
    pred[run] = avg
    want, key = evaluation.interpolate_between_keyframes(pred, idx, stride)
    assert want.dtype == np.float32
    rows = np.full(P, -1, np.int64); rows[run] = np.arange(W)
    left, right, weight, _ = evaluation.keyframe_plan(idx, stride, rows=rows)
    dp, df = torch.from_numpy(plain).cuda(), (torch.from_numpy(flipped).cuda() if flip else None)
    got = predict.assemble_tracks(dp, df, left, right, weight, flip_order=order).cpu().numpy()
    assert _same_bits(got[key], avg)                                  # a predicted frame is the averaged prediction
    n_interp = int(((left != right)).sum())
    assert n_interp > 500 and _same_bits(got, want)                   # interpolated frames and the tails behind the last keyframe too
    # root_relative: the root joint is exactly 0, the rest is the float32 difference
    rel = predict.assemble_tracks(dp, df, left, right, weight, flip_order=order, root=root).cpu().numpy()
    assert not rel[:, root].any()
    assert _same_bits(rel, want - want[:, root:root + 1])
    again = predict.assemble_tracks(dp, df, left, right, weight, flip_order=order, root=root).cpu().numpy()
    assert _same_bits(again, rel)
    # a plan row outside the predictions gives NaN instead of a read out of bounds
    bad = left.copy(); bad[5] = W
    out = predict.assemble_tracks(dp, df, bad, right, weight, flip_order=order).cpu().numpy()
    assert np.isnan(out[5]).all() and _same_bits(np.delete(out, 5, 0), np.delete(want, 5, 0))


@pytest.mark.parametrize("cfgname", ["h36m_351", "h36m_81"])
def test_predict_tracks_against_the_oracle(cfgname):
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model(cfgname)
    ms = MASK_STRIDE[cfgname]
    lens = [203, 418, 600]
    tracks = _pixel_tracks(lens, seed=4)
    res = [RES[i % len(RES)] for i in range(len(lens))]
    want = _oracle_tracks(cfg, arch, w, _host_normalised(tracks), ms)
    got = predict.predict_tracks(model, cfg, tracks, resolutions=res, mask_stride=ms, flip=True)
    assert [tuple(g.shape) for g in got] == [(n, 17, 3) for n in lens] and all(g.is_cuda and g.dtype == torch.float32 for g in got)
    a = torch.cat(got, 0).cpu().numpy()
    err = float(np.abs(a - want).max())
    print(f"{cfgname}: predict_tracks vs oracle pipeline max-abs {err:.3e} (bar {util.TOL_MAX_ABS})")
    assert err <= util.TOL_MAX_ABS
    assert not a[:, cfg.ROOT_KEYTPOINT].any()
    # the window forward instead of the frames form
    b = torch.cat(predict.predict_tracks(model, cfg, tracks, resolutions=res, mask_stride=ms, flip=True, reuse_frames=False), 0).cpu().numpy()
    d = float(np.abs(a - b).max())
    print(f"{cfgname}: reuse_frames True vs False max-abs {d:.3e} (bar 3e-5)")
    assert d <= 3e-5
    assert float(np.abs(b - want).max()) <= util.TOL_MAX_ABS
    # two calls: the same bits; the package-level export is the same function
    again = torch.cat(pkg.predict_tracks(model, cfg, tracks, resolutions=res, mask_stride=ms, flip=True), 0)
    assert _same_bits(again, a)


@pytest.mark.parametrize("cfgname", ["h36m_351", "h36m_81"])
def test_keyframes_only_equals_the_full_track_bitwise(cfgname):
    """Tracks whose copy-padding source frame (the last multiple of SEQUENCE_STRIDE) is one of the given keyframes -- for h36m_351 (mask
    stride == sequence stride) every length, for h36m_81 at mask stride 4 the lengths 4k + 1 and 4k + 2 (predict.padding_source_is_keyframe)."""
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model(cfgname, seed=5)
    ms = MASK_STRIDE[cfgname]
    lens = [201, 418, 597, 1]
    assert all(predict.padding_source_is_keyframe(n, cfg, ms) for n in lens)
    tracks = _pixel_tracks(lens, seed=6)
    res = [RES[i % len(RES)] for i in range(len(lens))]
    for reuse in (True, False):
        full = predict.predict_tracks(model, cfg, tracks, resolutions=res, mask_stride=ms, reuse_frames=reuse)
        keys = predict.predict_tracks(model, cfg, [t[::ms] for t in tracks], resolutions=res, mask_stride=ms, keyframes_only=True, lengths=lens,
                                      reuse_frames=reuse)
        for f, k in zip(full, keys):
            assert _same_bits(f, k), reuse
    with pytest.raises(ValueError):
        predict.predict_tracks(model, cfg, [t[::ms] for t in tracks], mask_stride=ms, keyframes_only=True)       # no lengths


def test_keyframes_only_where_copy_padding_repeats_a_frame_that_was_not_given():
    """h36m_81, mask stride 4 > sequence stride 2, lengths 4k + 3 and 4k: behind the end of the track the reference's copy padding repeats
    the last even frame, which is no multiple of 4 -- a full track has it, keyframe input cannot.  Every frame up to the last predicted one
    whose window ends inside the track is still bit-identical; the frames behind stay finite."""
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model("h36m_81", seed=5)
    ms, s, half = 4, cfg.SEQUENCE_STRIDE, cfg.SEQUENCE_LENGTH // 2
    lens = [203, 600]
    assert not any(predict.padding_source_is_keyframe(n, cfg, ms) for n in lens)
    tracks = _pixel_tracks(lens, seed=7)
    res = [RES[i % len(RES)] for i in range(len(lens))]
    full = predict.predict_tracks(model, cfg, tracks, resolutions=res, mask_stride=ms)
    keys = predict.predict_tracks(model, cfg, [t[::ms] for t in tracks], resolutions=res, mask_stride=ms, keyframes_only=True, lengths=lens)
    for n, f, k in zip(lens, full, keys):
        inside = [c for c in range(0, n, s) if c + half * s < n]      # predicted frames whose window reads nothing behind the end
        safe = inside[-1] + 1
        assert safe > n // 2 and _same_bits(f[:safe], k[:safe])
        assert bool(torch.isfinite(k).all())


@pytest.mark.parametrize("cfgname", ["h36m_351", "h36m_81"])
def test_consistent_with_run_eval(cfgname, monkeypatch):
    """The 2D data of the tiny Human3.6M fixture through predict_tracks against the predictions run_eval hands to its report, interpolated by
    the host: the same windows, batches and launches, and the assemble kernel in the host's operation order -- the same bits."""
    from uplift_upsample_3dhpe_amd import eval as ev
    from uplift_upsample_3dhpe_amd import evaluation, h36m, predict
    cfg, arch, w, model = _model(cfgname)
    cfg.BATCH_SIZE = 16
    cfg.MASK_STRIDE = cfg.MASK_STRIDE[0]
    seen = {}
    real = evaluation.evaluate_predictions

    def spy(pred3d, gt3d, actions, frame_indices, config, action_wise=True):
        seen["pred"], seen["idx"] = np.array(pred3d), np.array(frame_indices)
        return real(pred3d, gt3d, actions, frame_indices, config, action_wise=action_wise)
    monkeypatch.setattr(evaluation, "evaluate_predictions", spy)
    ev.run_eval(cfg, "h36m", os.path.join(G, "h36m_tiny_3d.npz"), os.path.join(G, "h36m_tiny_2d.npz"), "S9", model=model, action_wise=False,
                log=lambda *a: None)
    want, _ = evaluation.interpolate_between_keyframes(seen["pred"], seen["idx"], cfg.SEQUENCE_STRIDE)
    ds, p2 = h36m.load_dataset_and_2d_poses(os.path.join(G, "h36m_tiny_3d.npz"), os.path.join(G, "h36m_tiny_2d.npz"), verbose=False)
    _, _, p2d, _, _, _, _ = h36m.filter_and_subsample_dataset(ds, p2, ["S9"], "*", verbose=False)
    got = predict.predict_tracks(model, cfg, p2d, reuse_frames=False, root_relative=False)
    assert [len(g) for g in got] == [len(v) for v in p2d]
    got = torch.cat(got, 0).cpu().numpy()
    assert got.shape == want.shape and (np.diff(seen["idx"]) != 1).sum() == len(p2d) - 1       # run_eval's positions are the dense frames of the videos
    assert _same_bits(got, want.astype(np.float32))


def test_front_and_back_never_wait_for_the_device():
    """Everything predict_tracks adds around eval.predict_windows -- device tracks -> pose table (uu3d_normalize_tracks), plan upload and
    uu3d_assemble_tracks -- runs under torch's sync debug mode "error": no host synchronisation, no copy to the host.  (predict_windows
    itself synchronises once after its last forward and reads the range flag; with reuse_frames one frame count per table chunk.)"""
    from uplift_upsample_3dhpe_amd import evaluation, predict
    cfg = util.load_config("h36m_351")
    lens = [50, 64]
    tracks = [torch.from_numpy(t).cuda() for t in _pixel_tracks(lens, seed=8)]
    idx = np.concatenate([np.arange(n) for n in lens])
    run = np.flatnonzero(idx % 5 == 0)
    rows = np.full(len(idx), -1, np.int64); rows[run] = np.arange(len(run))
    left, right, weight, _ = evaluation.keyframe_plan(idx, 5, rows=rows)
    plain = torch.randn((len(run), 17, 3), device="cuda")
    flipped = torch.randn((len(run), 17, 3), device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        table, _ = predict.pose_table(tracks, "cuda", resolutions=RES[:2])
        keyt, _ = predict.pose_table([t[::5] for t in tracks], "cuda", resolutions=RES[:2], key_stride=5, lengths=lens)
        out = predict.assemble_tracks(plain, flipped, left, right, weight, flip_order=cfg.AUGM_FLIP_KEYPOINT_ORDER, root=cfg.ROOT_KEYTPOINT)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert tuple(table.kp2d.shape) == (114, 17, 2) and tuple(keyt.kp2d.shape) == (114, 17, 2) and tuple(out.shape) == (114, 17, 3)
    assert bool(torch.isfinite(out).all())
