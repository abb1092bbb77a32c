"""Shared helpers of the GPU tests of the track and live paths (test_predict_tracks_gpu, test_missed_detections_gpu, test_stream_gpu,
test_stream_fps_gpu, test_stream_out_fps_gpu): seeded models, pixel tracks at three resolutions, bit comparison, the push loop of a
session, the CPU oracle as the model.  A plain module: nothing here is collected."""
import numpy as np
import pytest

import uplift_upsample_3dhpe_amd as pkg
from tests import util

torch = pytest.importorskip("torch")
RES = [(1000, 1002), (1920, 1080), (640, 480)]                        # Human3.6M's near-square camera, two non-square ones
_MODELS = {}


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else b
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _pixel_tracks(lens, seed, J=17):
    rng = np.random.default_rng(seed)
    return [(rng.uniform(0.0, 1.0, size=(n, J, 2)) * np.array(RES[i % len(RES)], np.float64)).astype(np.float32) for i, n in enumerate(lens)]


def _host_normalised(tracks):
    from uplift_upsample_3dhpe_amd import h36m
    return [h36m.normalize_screen_coordinates(t, w=RES[i % len(RES)][0], h=RES[i % len(RES)][1]).astype(np.float32) for i, t in enumerate(tracks)]


def _model(cfgname, seed=2):
    """(config, arch, weights, model) with seeded weights, BATCH_SIZE 64; one model per (config, seed) for the whole run.  The config is
    the caller's own copy."""
    if (cfgname, seed) not in _MODELS:
        cfg = util.load_config(cfgname)
        cfg.BATCH_SIZE = 64
        arch = pkg.arch_from_config(cfg)
        w = pkg.init_weights(arch, seed=seed, perturb=0.1)
        _MODELS[cfgname, seed] = (cfg, arch, w, pkg.build_uplift_upsample_transformer(cfg, weights=w))
    cfg, arch, w, model = _MODELS[cfgname, seed]
    return cfg.copy(), arch, w, model


def _run(session, tracks, ticks, active=None, before_tick=None, valid=None, device_active=False):
    """Push ``tracks[i][k]`` into slot i at push k; a slot's frame is the next one of ITS track.  ``active(k)`` -> (T,) bools or None;
    ``valid[i]``: per-frame flags of track i.  One copy to the host at the end.  A session without ``out_fps`` -> (poses (ticks, T, J, 3),
    fresh (ticks, T)); with it -> (poses (ticks, T, R, J, 3), count (ticks, T), out_frames after the push (ticks, T)); ``check_range()`` is
    False and ``captures`` is 1 throughout (0 for a session without a graph)."""
    T, J = session.slots, session.model.arch.num_keypoints
    multi = session.max_out is not None
    poses = torch.zeros((ticks, T) + ((session.max_out,) if multi else ()) + (J, 3), dtype=torch.float32, device="cuda")
    flags = torch.zeros((ticks, T), dtype=torch.int32 if multi else torch.bool, device="cuda")
    total = torch.zeros((ticks, T), dtype=torch.int32, device="cuda")
    used = [0] * T
    for k in range(ticks):
        if before_tick is not None:
            before_tick(k, used)
        act = None if active is None else np.asarray(active(k), bool)
        kp = np.zeros((T, J, 2), np.float32)
        ok = np.ones(T, bool)
        for i in range(T):
            if act is None or act[i]:
                kp[i] = tracks[i][used[i]]
                if valid is not None:
                    ok[i] = bool(valid[i][used[i]])
                used[i] += 1
        a = act if act is None or not device_active else torch.from_numpy(act).cuda()
        p, f = session.push(kp, a, **({} if valid is None else {"valid": ok}))
        assert tuple(p.shape) == tuple(poses.shape[1:]) and p.is_cuda and f.is_cuda and session.captures == int(session.graph)
        poses[k].copy_(p)
        flags[k].copy_(f)
        if multi:
            total[k].copy_(session.out_frames)
        if k % 64 == 63:
            assert session.check_range() is False
    assert session.check_range() is False and session.captures == int(session.graph)
    return (poses.cpu().numpy(), flags.cpu().numpy()) + ((total.cpu().numpy(),) if multi else ())


def _model_rate_frames(tracks, fps, n_model, valid=None):
    """The first ``n_model`` model-rate frames of every track (uu3d_resample_tracks), normalised -> list of (n_model, J, 2) host arrays
    (and, with ``valid``, their flags)."""
    from uplift_upsample_3dhpe_amd import predict
    table, model_lens, _ = predict.resampled_pose_table(tracks, torch.device("cuda", 0), fps, resolutions=RES[:len(tracks)], valid=valid)
    assert (model_lens >= n_model).all()
    kp = torch.split(table.kp2d, [int(n) for n in model_lens], 0)
    frames = [t[:n_model].cpu().numpy() for t in kp]
    if valid is None:
        return frames
    return frames, [v[:n_model].cpu().numpy() != 0 for v in torch.split(table.valid, [int(n) for n in model_lens], 0)]


def _plain_keyframes(model, cfg, ms, a_m, frames, valid=None, with_capacity=False):
    """The model-rate frames through a plain session at lookahead a_m -> {centre: (T, J, 3) pose} (``with_capacity``: and the session's
    ring capacity)."""
    from uplift_upsample_3dhpe_amd import stream
    s = stream.StreamSession(model, cfg, slots=len(frames), resolutions=None, mask_stride=ms, flip=True, lookahead=a_m,
                             **({} if valid is None else {"missed_detections": True}))
    n = len(frames[0])
    poses, fresh = _run(s, frames, n, valid=valid)
    cap = s.ring_capacity
    s.close()
    keys = {}
    for t in range(n):
        if fresh[t].all():
            keys[t - a_m] = poses[t]
        else:
            assert not fresh[t].any()
    return (keys, cap) if with_capacity else keys


def _oracle_windows(cfg, norm_tracks, ms):
    """The sequence generator of the tracks as the evaluation sets it up (stride masks aligned globally, the config's padding) ->
    (config with MASK_STRIDE = ms, table, generator, descriptors)."""
    from uplift_upsample_3dhpe_amd.data import PoseTable, SequenceGenerator
    c = cfg.copy(); c.MASK_STRIDE = ms
    table = PoseTable(norm_tracks)
    gen = SequenceGenerator(table, seq_len=c.SEQUENCE_LENGTH, subsample=1, stride=c.SEQUENCE_STRIDE, padding_type=c.PADDING_TYPE,
                            flip_augment=False, mask_stride=ms, stride_mask_align_global=True, shuffle=False)
    return c, table, gen, gen.descriptors()


def _oracle_central(c, arch, w, gen, desc, window_valid=None):
    """The CPU oracle as the model on the windows ``desc``: flip as a second call, averaged -> (len(desc), J, 3) float64.
    ``window_valid`` (len(desc), N) bools: ANDed into the stride mask (it may only clear bits)."""
    from oracle import uplift_oracle as O
    b = gen.gather(desc, zero_masked=False, with_3d=False)
    x, m = b["kp2d"].cpu().numpy(), b["stride_mask"].cpu().numpy().astype(bool)
    if window_valid is not None:
        assert not (window_valid & ~m).any()
        m = m & window_valid
    _, cen = O.eval_step_with_flip(util.hp_from_arch(arch), w, x, m, c.AUGM_FLIP_KEYPOINT_ORDER)
    return np.asarray(cen, np.float64)


def _oracle_poses(cfg, arch, w, norm_tracks, centres, ms):
    """The CPU oracle as the model, in the manner of the predict_tracks test: the window of frame ``centres[k]`` of track k by the sequence
    generator (stride masks aligned globally, the config's padding), flip as a second call, averaged; root-relative."""
    c, table, gen, desc = _oracle_windows(cfg, norm_tracks, ms)
    starts = np.concatenate([[0], np.cumsum([len(t) for t in norm_tracks])[:-1]])
    run = starts + np.asarray(centres)
    assert np.array_equal(desc[run, 0], np.arange(len(norm_tracks))) and np.array_equal(desc[run, 1], centres)
    cen = _oracle_central(c, arch, w, gen, desc[run])
    return cen - cen[:, c.ROOT_KEYTPOINT:c.ROOT_KEYTPOINT + 1]


def _oracle_tracks(cfg, arch, w, norm_tracks, ms, window_valid=None):
    """The same pipeline with the CPU oracle as the model: windows of the needed frames, flip as a second call, host interpolation.
    ``window_valid(desc, config, table)`` -> (len(desc), N) bools for ``_oracle_central`` (missed detections)."""
    from uplift_upsample_3dhpe_amd import eval as ev
    from uplift_upsample_3dhpe_amd import evaluation
    c, table, gen, desc = _oracle_windows(cfg, norm_tracks, ms)
    run = np.flatnonzero(ev.needed_windows(desc[:, 1], c))
    pred = np.zeros((len(desc), 17, 3), np.float64)
    pred[run] = _oracle_central(c, arch, w, gen, desc[run], None if window_valid is None else window_valid(desc[run], c, table))
    pred, _ = evaluation.interpolate_between_keyframes(pred, desc[:, 1], c.SEQUENCE_STRIDE)
    return pred - pred[:, c.ROOT_KEYTPOINT:c.ROOT_KEYTPOINT + 1]
