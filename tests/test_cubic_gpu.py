"""GPU: C1 motion between keyframes -- uu3d_assemble_tracks_cubic and ``predict_tracks(interpolation="cubic")``.  The reference is
evaluation.interpolate_cubic_host, the rule in numpy, on the raw window predictions; the kernel computes its float64 expression in its
order and rounds once, so every comparison is on the float32 bits.
  1. the launch alone on the track table of tests/cubic_util: flip on and off, root joints, the scalar tail, NaN rows
  2. predict_tracks(interpolation="cubic"): plain, keyframes_only, fps, fps + out_fps, valid="finite"
  3. camera= with out_fps: the roots are solved against the cubic poses
  4. predict_detections(interpolation="cubic") equals predict_tracks on the tracks of the association
  5. interpolation="linear" is the call without the keyword"""
import numpy as np
import pytest

from tests import cubic_util as cu
from tests.tracks_util import RES, _model, _pixel_tracks, _same_bits

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
CAMS = [(1145.0, 1143.8, 512.5, 515.5), (1400.0, 1390.0, 960.0, 540.0), (600.0, 610.0, 320.0, 240.0)]


def _mean_with_unflipped(plain, flipped, order):
    """eval.py:163-166 in numpy float32: x negated, joints permuted, (a + b) / 2."""
    if flipped is None:
        return plain
    f = np.concatenate([flipped[..., :1] * np.float32(-1.0), flipped[..., 1:]], axis=-1)[:, order]
    avg = (plain + f) / np.float32(2.0)
    assert avg.dtype == np.float32
    return avg


def _shift(poses, root):
    return poses if root < 0 else poses - poses[:, root:root + 1]


# ---- 1. the launch alone -------------------------------------------------------------------------------------------------------------
_PLANS = {}


def _plan(name):
    """The cubic plan of the track table through ``rows`` (only keyframes are predictions), computed once -> (plan, W)."""
    from uplift_upsample_3dhpe_amd import evaluation
    if name not in _PLANS:
        rows, W = cu.key_rows()
        f = cu.frame_indices()
        if name == "frames":
            plan = evaluation.keyframe_plan_cubic(f, cu.STRIDE, rows=rows)
        else:
            plan = evaluation.keyframe_plan_cubic_at(f, cu.STRIDE, cu.positions_at(cu.STEPS[name]), rows=rows)
        _PLANS[name] = (plan, W)
    return _PLANS[name]


@pytest.mark.parametrize("J,flip,root,name,frames,tail", [
    (17, True, 0, "frames", None, 0),                                 # 92 frames x 51 floats = 4692: five blocks, a multiple of 4, no tail
    (17, True, 5, "frames", 91, 1),                                   # 91 x 51 = 4641 floats: a tail of one float
    (13, False, -1, "frames", 91, 1),
    (13, True, 5, "fps30", None, None),                               # weights in thirds of a frame
    (17, False, 5, "out_fps100", None, None),
    (17, True, 0, "frames", 1, 3),                                    # one frame, 51 floats: 12 stores of 16 bytes and a tail of three floats
])
def test_assemble_tracks_cubic_alone_equals_the_rule_bitwise(J, flip, root, name, frames, tail):
    from uplift_upsample_3dhpe_amd import evaluation, predict
    plan, W = _plan(name)
    if frames is not None:
        plan = tuple(a[:frames] for a in plan)
    F = len(plan[1])
    rng = np.random.default_rng(J + 100 * flip + root)
    plain = rng.normal(size=(W, J, 3)).astype(np.float32)
    flipped = rng.normal(size=(W, J, 3)).astype(np.float32) if flip else None
    order = rng.permutation(J)
    want = _shift(evaluation.interpolate_cubic_host(_mean_with_unflipped(plain, flipped, order), plan), root)
    dp, df = torch.from_numpy(plain).cuda(), (torch.from_numpy(flipped).cuda() if flip else None)
    got = predict.assemble_tracks_cubic(dp, df, *plan, flip_order=order if flip else None, root=root)
    assert got.dtype == torch.float32 and tuple(got.shape) == (F, J, 3) and (tail is None or F * J * 3 % 4 == tail)
    assert _same_bits(got, want)
    if root >= 0:
        assert not got[:, root].any()                                 # exactly 0, on interpolated frames too
    if F == 1:
        return
    assert (plan[1] != plan[2]).sum() >= 20 and (plan[0] >= 0).any() and (plan[3] >= 0).any()
    # keyframes and frames behind the last one: the linear launch's bits
    own = np.flatnonzero(plan[1] == plan[2])
    linear = predict.assemble_tracks(dp, df, plan[1], plan[2], plan[4], flip_order=order if flip else None, root=root)
    assert _same_bits(got[own], linear[own]) and not _same_bits(got, linear)
    # rows outside the predictions give NaN frames and nothing else changes
    bad = [a.copy() for a in plan]
    mixed = np.flatnonzero((plan[0] >= 0) & (plan[3] >= 0))
    bad[1][2], bad[1][own[-1]], bad[0][mixed[0]], bad[3][mixed[-1]] = W, -1, W, -2
    rows = [2, int(own[-1]), int(mixed[0]), int(mixed[-1])]
    out = predict.assemble_tracks_cubic(dp, df, *bad, flip_order=order if flip else None, root=root).cpu().numpy()
    assert np.isnan(out[rows]).all() and _same_bits(np.delete(out, rows, 0), np.delete(want, rows, 0))


# ---- 2. predict_tracks ---------------------------------------------------------------------------------------------------------------
def _expected(model, cfg, tracks, res, ms, flip, keyframes_only=False, lengths=None, valid=None, fps=None, out_fps=None):
    """The front of predict_tracks up to the raw window predictions (``predict._predicted_windows``), then the rule in numpy:
    -> (poses (R, J, 3) float32 root-relative, returned frames per track, the plan)."""
    from uplift_upsample_3dhpe_amd import eval as ev
    from uplift_upsample_3dhpe_amd import evaluation, predict
    c = cfg.copy()
    c.MASK_STRIDE = ms
    given = [len(t) for t in tracks]
    if fps is None:
        table, lens = predict.pose_table(tracks, model.device, res, ms if keyframes_only else 0, lengths, valid=valid, model=model)
    else:
        rates = predict.frame_rates(fps, len(tracks))
        table, _, _ = predict.resampled_pose_table(tracks, model.device, rates, res, valid=valid, model=model)
        lens, positions = predict.output_positions(given, rates, rates if out_fps is None else out_fps)
    raw, frame_idx, rows = predict._predicted_windows(model, c, table, ms, flip, None, None, True, True)
    order = np.asarray(c.AUGM_FLIP_KEYPOINT_ORDER)
    avg = _mean_with_unflipped(raw[0].cpu().numpy(), raw[1].cpu().numpy() if flip else None, order)
    stride = ev.prediction_stride(c)
    assert stride == c.SEQUENCE_STRIDE > 1
    if fps is None:
        plan = evaluation.keyframe_plan_cubic(frame_idx, stride, rows=rows)
    else:
        plan = evaluation.keyframe_plan_cubic_at(frame_idx, stride, positions, rows=rows)
    return _shift(evaluation.interpolate_cubic_host(avg, plan), int(c.ROOT_KEYTPOINT)), [int(n) for n in lens], plan


def _case(name):
    """-> (track lengths, keywords).  h36m_351 predicts every 5th model frame; the lengths give 1, 3 and 6 predicted frames per track on the
    model's grid (fps=30: 1, 13 and 28 model frames; fps=10: 1, 11 and 26)."""
    if name == "fps30":
        return [1, 8, 17], dict(fps=30)
    if name == "fps10_out50":
        return [1, 3, 6], dict(fps=10, out_fps=50)
    return [1, 13, 26], {}


@pytest.mark.parametrize("name", ["plain", "keyframes_only", "fps30", "fps10_out50", "finite"])
def test_predict_tracks_cubic_equals_the_rule_on_the_raw_predictions(name):
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model("h36m_351")
    ms = 5
    lens, kw = _case(name)
    tracks = _pixel_tracks(lens, seed=61)
    res = [RES[i % len(RES)] for i in range(len(lens))]
    if name == "keyframes_only":
        tracks, kw = [t[::ms] for t in tracks], dict(keyframes_only=True, lengths=lens)
    elif name == "finite":
        tracks[1][5], tracks[2][11, 3, 0] = np.nan, np.nan            # a predicted frame of track 1, one coordinate of a frame of track 2
        kw = dict(valid="finite")
    for flip in (True, False):
        want, returned, plan = _expected(model, cfg, tracks, res, ms, flip, **kw)
        got = predict.predict_tracks(model, cfg, tracks, resolutions=res, mask_stride=ms, flip=flip, interpolation="cubic", **kw)
        assert [int(g.shape[0]) for g in got] == returned and all(g.is_cuda and g.dtype == torch.float32 for g in got)
        got = torch.cat(got, 0)
        assert bool(torch.isfinite(got).all()) and _same_bits(got, want)
        assert not got[:, cfg.ROOT_KEYTPOINT].any()
        # 3 predicted frames: every segment has a neighbour on one side only; 6: the inner segments have both
        mixed = plan[1] != plan[2]
        assert ((plan[0] >= 0) & (plan[3] >= 0)).any() and ((plan[0] >= 0) & (plan[3] < 0)).any() and ((plan[0] < 0) & (plan[3] >= 0)).any()
        # a predicted frame and a frame behind the last one keep the linear call's bits; the frames between move
        linear = torch.cat(predict.predict_tracks(model, cfg, tracks, resolutions=res, mask_stride=ms, flip=flip, **kw), 0)
        own = torch.from_numpy(~mixed).cuda()
        assert linear.shape == got.shape and _same_bits(got[own], linear[own]) and not _same_bits(got[~own], linear[~own])


# ---- 3. camera= with out_fps -----------------------------------------------------------------------------------------------------------
def test_camera_with_out_fps_solves_the_roots_against_the_cubic_poses():
    """fps=25, out_fps=50: every second returned frame is a given frame, and only every fifth of those is a predicted one -- the poses
    the roots are solved against are read from the cubic at the given frames' times, the same motion that is returned."""
    from fractions import Fraction
    from uplift_upsample_3dhpe_amd import predict, rates
    cfg, arch, w, model = _model("h36m_351")
    lens = [1, 9, 16]
    rng = np.random.default_rng(62)
    tracks = []
    for i, n in enumerate(lens):                                      # people far from the camera: solved and unsolved frames mix
        centre = rng.uniform(0.3, 0.7, size=2) * RES[i] + np.arange(n)[:, None] * np.array([1.5, 0.5])
        tracks.append((centre[:, None, :] + rng.uniform(-4.0, 4.0, size=(n, 17, 2))).astype(np.float32))
    kw = dict(resolutions=RES, mask_stride=5, fps=25, out_fps=50)
    cubic = predict.predict_tracks(model, cfg, tracks, interpolation="cubic", **kw)
    poses, roots, state = predict.predict_tracks(model, cfg, tracks, interpolation="cubic", camera=CAMS, **kw)
    want, returned, plan = _expected(model, cfg, tracks, RES, 5, bool(cfg.EVAL_FLIP), fps=25, out_fps=50)
    assert returned == [2 * n - 1 for n in lens]
    assert _same_bits(torch.cat(poses, 0), want) and all(_same_bits(p, q) for p, q in zip(poses, cubic))
    at_given = np.concatenate([p.cpu().numpy()[::2] for p in poses])
    assert len(at_given) == sum(lens)
    want_roots, want_solved = predict.solve_roots_host(at_given, np.concatenate(tracks), CAMS, lens=lens)
    want_traj, want_state = predict.root_trajectory_host(want_roots, want_solved, lens, rates.given_positions(returned, [Fraction(1, 2)] * 3))
    assert np.array_equal(torch.cat(state, 0).cpu().numpy(), want_state) and _same_bits(torch.cat(roots, 0), want_traj)
    assert want_solved.any()
    # the given frames between two predicted ones are where the linear call's poses, and so its roots, differ
    lin_poses, lin_roots, _ = predict.predict_tracks(model, cfg, tracks, camera=CAMS, **kw)
    assert not _same_bits(torch.cat(lin_poses, 0), want) and not _same_bits(torch.cat(lin_roots, 0), want_traj)


# ---- 4. predict_detections ---------------------------------------------------------------------------------------------------------------
def test_predict_detections_cubic_equals_predict_tracks_on_the_associations_tracks():
    """One video, two people 600 px apart who walk slowly, listed in changing order."""
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model("h36m_81")
    T, K = 21, 17
    rng = np.random.default_rng(63)
    body = rng.uniform(-1.0, 1.0, size=(K, 2)) * [50.0, 100.0]
    people = [np.array([500.0 + 600.0 * p, 500.0]) + np.arange(T)[:, None, None] * np.array([2.0, 0.5]) + body + rng.uniform(-2, 2, size=(T, K, 2))
              for p in range(2)]
    dets = np.stack(people, 1).astype(np.float32)
    swap = rng.uniform(size=T) < 0.5
    dets[swap] = dets[swap][:, ::-1]
    rule = dict(max_age=2, max_dist=0.5, min_common=3)
    kw = dict(resolutions=(1920, 1080), mask_stride=4)
    got = predict.predict_detections(model, cfg, [dets], slots=2, interpolation="cubic", **rule, **kw)
    tracks = predict.association_tracks_host(dets, None, predict.associate_host(dets, None, slots=2, **rule))
    assert len(got) == 1 and len(got[0]) == len(tracks) == 2 and [len(t[2]) for t in tracks] == [T, T]
    ref = predict.predict_tracks(model, cfg, [t[2] for t in tracks], valid=[t[3] for t in tracks], interpolation="cubic", **kw)
    linear = predict.predict_detections(model, cfg, [dets], slots=2, **rule, **kw)
    for person, (tid, first, _, _), p, q in zip(got[0], tracks, ref, linear[0]):
        assert person[:2] == (tid, first) and _same_bits(person[2], p) and not _same_bits(person[2], q[2])


# ---- 5. linear is unchanged ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, {"fps": 30}], ids=["plain", "fps30"])
def test_interpolation_linear_is_the_call_without_the_keyword(kw):
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model("h36m_351")
    tracks = _pixel_tracks([1, 13, 26], seed=64)
    a = predict.predict_tracks(model, cfg, tracks, resolutions=RES, mask_stride=5, **kw)
    b = predict.predict_tracks(model, cfg, tracks, resolutions=RES, mask_stride=5, interpolation="linear", **kw)
    assert len(a) == len(b) == 3 and all(_same_bits(p, q) for p, q in zip(a, b))
