"""GPU: stream.StreamSession(fps=F, interpolation="cubic") -- the poses of a session with a frame rate read from the C1 cubic through its
keyframes -- against what it is defined to be: evaluation.interpolate_cubic_host on the keyframes of a plain session at the cubic plan's
model lookahead a_m fed the model-rate frames, with the rows of rates.push_plan_cubic / out_push_plan_cubic, BIT FOR BIT (hermite_mix runs
with contraction off, as the offline cubic does).  Three slots, flip on, pixel tracks at three resolutions, seeded weights."""
import math

import numpy as np
import pytest

from tests import util
from tests.tracks_util import RES, _bits, _model, _model_rate_frames, _pixel_tracks, _plain_keyframes, _run

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
T, J = 3, 17


def _cubic_plan(cfg, fps, ms, extra, out_fps=None):
    from uplift_upsample_3dhpe_amd import stream
    lo = stream.rate_plan(cfg, fps, None, ms, out_fps=out_fps, interpolation="cubic").min_lookahead
    return stream.rate_plan(cfg, fps, lo + extra, ms, out_fps=out_fps, interpolation="cubic")


def _pushes(plan, least=60):
    """Source frames so that the key ring wraps twice, n_model >= 2 D P + a_m + 12, and at least ``least`` -> (n_src, n_model)."""
    n_src = max(least, -(-(2 * plan.D * plan.pred_stride + plan.a_m + 11) * plan.B // plan.A) + 1)
    n_model = (n_src - 1) * plan.A // plan.B + 1
    assert n_model >= 2 * plan.D * plan.pred_stride + plan.a_m + 12
    return n_src, n_model


def _rule(keys, P, rows):
    """interpolate_cubic_host on the plain session's keyframes.  ``keys``: {centre: (T, J, 3)}; ``rows``: (before, k0, k1, after, weight)
    per pose as MODEL frames, None where there is none -> (len(rows), T, J, 3) float32."""
    from uplift_upsample_3dhpe_amd import evaluation
    table = np.stack([keys[c] for c in range(0, max(keys) + 1, P)])
    place = lambda k: -1 if k is None else k // P
    plan = tuple(np.array([place(r[i]) for r in rows], np.int64) for i in range(4)) + (np.array([r[4] for r in rows], np.float64),)
    assert plan[3].max() < len(table)                                    # every keyframe the rule reads was emitted by the plain session
    return evaluation.interpolate_cubic_host(table, plan)


def _session(model, cfg, ms, plan, fps, out_fps=None, **kw):
    from uplift_upsample_3dhpe_amd import stream
    s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=ms, flip=True, lookahead=plan.lookahead, fps=fps, out_fps=out_fps,
                             interpolation="cubic", **kw)
    assert s.interpolation == "cubic" and s.rate == plan and s.model_lookahead == plan.a_m
    emit = "uu3d_stream_timed_emit_cubic" if out_fps is None else "uu3d_stream_timed_emit_multi_cubic"
    assert s._push_after[0][0].__name__ == emit and [fn.__name__ for fn, a in s._tick_steps if a is not None][-1] == "uu3d_stream_file_keyframe"
    return s


@pytest.mark.parametrize("cfgname,ms,fps", [("h36m_81", 4, 24), ("h36m_81", 4, 30), ("h36m_351", 5, 30)])
def test_bits_against_the_numpy_rule(cfgname, ms, fps):
    """Every returned pose with j >= lookahead equals the rule on bits.  A slot's first segment (no keyframe in front: the one-sided
    tangent) is read iff a source frame lies strictly inside (0, P): at 30 fps in both configs; at 24 fps on P = 2 frame 1 already sits
    at 25/12 > 2, so that case has none -- the assertion says which."""
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model = _model(cfgname)
    plan = _cubic_plan(cfg, fps, ms, 2)
    P, L = plan.pred_stride, plan.lookahead
    n_src, n_model = _pushes(plan)
    tracks = _pixel_tracks([n_src] * T, seed=311)
    keys = _plain_keyframes(model, cfg, ms, plan.a_m, _model_rate_frames(tracks, fps, n_model))
    s = _session(model, cfg, ms, plan, fps)
    poses, fresh = _run(s, tracks, n_src)                                 # (asserts captures == 1 and check_range() is False throughout)
    assert s.check_range() is False and s.captures == 1
    assert s.source_frames.cpu().tolist() == [n_src] * T and s.frames.cpu().tolist() == [n_model] * T
    s.close()
    assert np.array_equal(fresh, np.repeat((np.arange(n_src) >= L)[:, None], T, 1)) and not poses[:L].any()
    assert np.isfinite(poses).all() and not poses[:, :, cfg.ROOT_KEYTPOINT].any()
    pps = [stream.push_plan_cubic(j, plan) for j in range(L, n_src)]
    want = _rule(keys, P, [(pp["before"], pp["k0"], pp["k1"], pp["after"], pp["weight"]) for pp in pps])
    exact = sum(pp["k0"] == pp["k1"] for pp in pps)
    mixed = len(pps) - exact
    first = sum(pp["k0"] != pp["k1"] and pp["before"] is None for pp in pps)
    wrong = np.flatnonzero((_bits(poses[L:]) != _bits(want)).any(axis=(1, 2, 3)))
    print(f"{cfgname} s_in {ms} at {fps} fps cubic, lookahead {L} (a_m {plan.a_m}, D {plan.D}): {n_src} pushes, {n_model} model frames, "
          f"{exact} keyframe outputs, {mixed} mixed ({first} in the first segment), {len(wrong)} pushes differ from the rule")
    assert len(wrong) == 0, (wrong[:5] + L, float(np.abs(poses[L:] - want).max()))
    assert exact >= 2 and mixed > 0 and (first > 0) == (plan.A < P * plan.B)
    assert first > 0 or (cfgname, fps) == ("h36m_81", 24)
    assert float(np.abs(want).max()) > 1e-3                              # (poses, not zeros)


@pytest.mark.parametrize("cfgname,ms,fps,out_fps", [("h36m_351", 5, 10, 50), ("h36m_81", 4, 30, 24)])
def test_bits_against_the_numpy_rule_with_an_output_rate(cfgname, ms, fps, out_fps):
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model = _model(cfgname)
    plan = _cubic_plan(cfg, fps, ms, 2, out_fps)
    P, L, R = plan.pred_stride, plan.lookahead, plan.max_out
    n_src, n_model = _pushes(plan, least=48)
    tracks = _pixel_tracks([n_src] * T, seed=321)
    keys = _plain_keyframes(model, cfg, ms, plan.a_m, _model_rate_frames(tracks, fps, n_model))
    s = _session(model, cfg, ms, plan, fps, out_fps)
    poses, count, total = _run(s, tracks, n_src)
    assert s.check_range() is False and s.captures == 1
    s.close()
    linear = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=ms, flip=True, lookahead=L, fps=fps, out_fps=out_fps)
    assert linear.interpolation == "linear" and linear._push_after[0][0].__name__ == "uu3d_stream_timed_emit_multi"
    lp, lc, lt = _run(linear, tracks, n_src)
    linear.close()
    assert np.array_equal(count, lc) and np.array_equal(total, lt) and total[-1].tolist() == [(n_src - 1 - L) * out_fps // fps + 1] * T
    frames = [stream.out_push_plan_cubic(j, plan) for j in range(n_src)]
    assert np.array_equal(count, np.repeat(np.array([len(f) for f in frames])[:, None], T, 1)) and count.max() == R
    rows = [f[1:] for fs in frames for f in fs]
    want = _rule(keys, P, rows)
    got = np.concatenate([poses[j, :, :len(fs)].transpose(1, 0, 2, 3) for j, fs in enumerate(frames)])      # (poses, T, J, 3), in order
    exact = sum(r[1] == r[2] for r in rows)
    first = sum(r[1] != r[2] and r[0] is None for r in rows)
    wrong = np.flatnonzero((_bits(got) != _bits(want)).any(axis=(1, 2, 3)))
    print(f"{cfgname} s_in {ms}, {fps} -> {out_fps} fps cubic, lookahead {L} (a_m {plan.a_m}, D {plan.D}, R {R}): {n_src} pushes, {len(rows)} poses, "
          f"{exact} on keyframes, {first} in the first segment, {len(wrong)} differ from the rule")
    assert len(wrong) == 0, (wrong[:5], float(np.abs(got - want).max()))
    # (the first segment is read iff an output frame lies strictly inside (0, P): at 50 fps out on P = 5, not at 24 fps out on P = 2)
    assert exact >= 2 and len(rows) - exact > 0 and (first > 0) == (plan.pos_num < P * plan.pos_den)
    assert first > 0 or (cfgname, out_fps) == ("h36m_81", 24)
    for j, fs in enumerate(frames):                                      # rows behind count are zeros
        assert not poses[j, :, len(fs):].any(), j
    assert not np.array_equal(_bits(lp), _bits(poses))                   # (and the cubic is not the line)


def test_against_predict_tracks_cubic():
    """replay_tracks(interpolation="cubic") against predict_tracks(fps=30, out_fps=60, interpolation="cubic") on the whole track, at the
    smallest lookahead for which the cubic plan's a_m = (SEQUENCE_LENGTH // 2) * SEQUENCE_STRIDE: every window of the session is complete,
    and every keyframe a returned pose reads -- k1 + P included -- is one whose offline window ends inside the track."""
    from uplift_upsample_3dhpe_amd import predict, stream
    cfgname, ms, fps, out_fps = "h36m_81", 4, 30, 60
    cfg, arch, w, model = _model(cfgname)
    cubic = lambda la: stream.rate_plan(cfg, fps, la, ms, out_fps=out_fps, interpolation="cubic")
    lo = cubic(None).min_lookahead
    L = next(la for la in range(lo, lo + 400) if cubic(la).a_m == stream.max_lookahead(cfg))
    plan = cubic(L)
    lens = [L + 45, L + 38, L + 30]
    tracks = _pixel_tracks(lens, seed=331)
    got, counts = stream.replay_tracks(model, cfg, tracks, resolutions=RES, mask_stride=ms, flip=True, lookahead=L, fps=fps, out_fps=out_fps,
                                       interpolation="cubic")
    want = predict.predict_tracks(model, cfg, tracks, resolutions=RES, mask_stride=ms, flip=True, fps=fps, out_fps=out_fps, interpolation="cubic")
    line = predict.predict_tracks(model, cfg, tracks, resolutions=RES, mask_stride=ms, flip=True, fps=fps, out_fps=out_fps)
    worst = apart = 0.0
    for i, n in enumerate(lens):
        n_out = (n - 1 - L) * out_fps // fps + 1
        assert got[i].shape == (n_out, J, 3) and counts[i].shape == (n,) and counts[i].sum() == n_out and n_out >= 50
        assert counts[i].tolist() == [len(stream.out_push_plan_cubic(j, plan)) for j in range(n)]
        worst = max(worst, float(np.abs(got[i] - want[i][:n_out].cpu().numpy()).max()))
        apart = max(apart, float(np.abs(got[i] - line[i][:n_out].cpu().numpy()).max()))
        assert float(np.abs(got[i]).max()) > 1e-3 and got[i].any(axis=(1, 2)).all()      # (poses, not zeros)
    print(f"{cfgname} {fps} -> {out_fps} fps cubic, lookahead {L} (a_m {plan.a_m}): max-abs to predict_tracks(interpolation='cubic') {worst:.3e} "
          f"(bar {util.TOL_MAX_ABS}); to the linear call {apart:.3e}")
    assert worst <= util.TOL_MAX_ABS


def test_reset_leaks_no_stale_keyframe():
    """h36m_81 at 30 fps: slot 0 is reset at push 50, long after its ring has wrapped, and pushed a new track.  Its poses equal, bit for
    bit, those of a session that never saw the first track -- the one-sided first segment does not read the ring place in front of
    keyframe 0, which still holds a pose of the old track -- and slots 1 and 2 equal the same session's, undisturbed."""
    cfgname, ms, fps = "h36m_81", 4, 30
    cfg, arch, w, model = _model(cfgname)
    plan = _cubic_plan(cfg, fps, ms, 2)
    ticks, at = 100, 50
    assert (at - 1) * plan.A // plan.B > 2 * plan.D * plan.pred_stride + plan.a_m and plan.A < plan.pred_stride * plan.B
    tracks = _pixel_tracks([ticks] * T, seed=341)
    s = _session(model, cfg, ms, plan, fps)

    def before(k, used):
        if k == at:
            s.reset([0])
    poses, fresh = _run(s, tracks, ticks, before_tick=before)
    assert s.source_frames.cpu().tolist() == [ticks - at, ticks, ticks]
    s.close()
    alone = _session(model, cfg, ms, plan, fps)
    p, f = _run(alone, [np.concatenate([tracks[0][at:], tracks[0][:at]]), tracks[1], tracks[2]], ticks)
    alone.close()
    n = ticks - at
    assert np.array_equal(f[:n, 0], fresh[at:, 0]) and f[:n, 0].sum() == n - plan.lookahead
    assert np.array_equal(_bits(p[:n, 0]), _bits(poses[at:, 0]))
    assert np.array_equal(f[:, 1:], fresh[:, 1:]) and np.array_equal(_bits(p[:, 1:]), _bits(poses[:, 1:]))
    assert not np.array_equal(_bits(poses[:n, 0]), _bits(poses[at:, 0]))      # (the new track is another track)
    # between the reset and the new track's first pose the slot holds zeros
    assert not fresh[at:at + plan.lookahead, 0].any() and not poses[at:at + plan.lookahead, 0].any()


def test_stages_behind_the_emit_read_the_cubic_poses():
    """fps=30, interpolation="cubic", rotations=True, bones="track": the raw poses are the cubic session's own, the returned poses are
    LiveBonesHost fed them, the quaternions joint_rotations_host of the returned poses -- all on bits."""
    from uplift_upsample_3dhpe_amd import stream
    cfgname, ms, fps = "h36m_81", 4, 30
    cfg, arch, w, model = _model(cfgname)
    plan = _cubic_plan(cfg, fps, ms, 2)
    ticks = 60
    tracks = _pixel_tracks([ticks] * T, seed=351)
    s = _session(model, cfg, ms, plan, fps)
    plain, plain_fresh = _run(s, tracks, ticks)
    s.close()
    s = _session(model, cfg, ms, plan, fps, rotations=True, bones="track")
    assert [fn.__name__ for fn, a in s._push_after] == ["uu3d_stream_timed_emit_cubic", "uu3d_stream_bones", "uu3d_joint_rotations"]
    dev = model.device
    grab = {k: torch.zeros((ticks, T) + shape, dtype=dt, device=dev) for k, shape, dt in (
        ("out", (J, 3), torch.float32), ("raw", (J, 3), torch.float32), ("fresh", (), torch.bool), ("quat", (J, 4), torch.float32))}
    for k in range(ticks):
        out = s.push(np.stack([t[k] for t in tracks]))
        assert len(out) == 3 and s.captures == 1 and out[0] is s.fixed_poses
        for key, t in (("out", out[0]), ("raw", s.raw_poses), ("fresh", out[1]), ("quat", out[2])):
            grab[key][k].copy_(t)
    assert s.check_range() is False and s.captures == 1
    s.close()
    g = {k: v.cpu().numpy() for k, v in grab.items()}
    assert np.array_equal(g["fresh"], plain_fresh) and np.array_equal(_bits(g["raw"]), _bits(plain)) and g["fresh"].sum() == T * (ticks - plan.lookahead)
    host = stream.LiveBonesHost(T)
    for k in range(ticks):
        fixed = host.step(g["raw"][k], g["fresh"][k], None)
        assert np.array_equal(_bits(g["out"][k]), _bits(fixed)), k
        assert np.array_equal(_bits(g["quat"][k]), _bits(stream.joint_rotations_host(g["out"][k])[0])), k
    assert not np.array_equal(_bits(g["out"]), _bits(g["raw"]))


@pytest.mark.parametrize("rates", [{}, {"fps": 30}, {"fps": 10, "out_fps": 50}])
def test_linear_is_the_session_without_the_keyword(rates):
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model = _model("h36m_81")
    ticks = 60
    tracks = _pixel_tracks([ticks] * T, seed=361)
    runs, tables = [], []
    for kw in ({}, {"interpolation": "linear"}):
        s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=4, flip=True, lookahead=4, **rates, **kw)
        assert s.interpolation == "linear"
        tables.append([[fn.__name__ for fn, a in steps if a is not None] for steps in (s._push_before, s._tick_steps, s._push_after)])
        runs.append(_run(s, tracks, ticks))
        assert s.captures == 1
        s.close()
    assert tables[0] == tables[1] and not any("cubic" in name for steps in tables[0] for name in steps)
    for a, b in zip(*runs):
        assert np.array_equal(a, b) if a.dtype != np.float32 else np.array_equal(_bits(a), _bits(b))
    assert float(np.abs(runs[0][0]).max()) > 1e-3
