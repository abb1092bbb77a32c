"""GPU: the end of a live track -- StreamSession.finish and the ``drain`` keywords (include/uu3d.h, LIVE TRACKS: END OF A TRACK).  The one
rule, extended: row k - 1 of ``finish`` is the pose predict_tracks gives for frame len - 1 - lookahead + k of the WHOLE track, and the pose a
session of lookahead a - k returns at its last push.  Three slots, flip on, pixel tracks at three resolutions, seeded weights.
  1. whole-track identity: replay_tracks(drain=True) against predict_tracks and the oracle pipeline
  2. bit identity: finish() row k - 1 against the last push of a session with lookahead a - k
  3. staggered ends: finish([i]) while the other slots go on
  4. graph and state: captures, graph=False, finish never waits
  5. options: missed detections, repair_joints, keypoints
  6. camera and smooth against the numpy mirrors' drain steps
  7. replay_detections(drain=True)"""
import numpy as np
import pytest

from tests import util
from tests.tracks_util import RES, _bits, _model, _oracle_poses, _pixel_tracks

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
T, J = 3, 17
CAMERAS = [(8.0 * w, 8.0 * w, 0.5 * w, 0.5 * h) for w, h in RES]      # a long lens: solved and held roots mix (tests/test_stream_root_gpu.py)


def _push_all(s, tracks, first=0, last=None, valid=None, active=None, keep=False):
    """Push frames first .. last - 1 of every track (slot i: tracks[i]) -> what the last push returned, as host arrays; ``keep``: what
    every push returned, stacked (one copy to the host)."""
    last = len(tracks[0]) if last is None else last
    kept = []
    out = None
    for k in range(first, last):
        kw = {} if valid is None else {"valid": np.stack([np.asarray(valid[i][k]) for i in range(len(tracks))])}
        out = s.push(np.stack([t[k] for t in tracks]), active, **kw)
        if keep:
            kept.append([o.clone() for o in out])
    if keep:
        return [torch.stack(c).cpu().numpy() for c in zip(*kept)]
    return [o.cpu().numpy() for o in out]


def _host(out):
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("cfgname,ms,L,a", [("h36m_81", 4, 60, 7), ("h36m_81", 4, 60, 40), ("h36m_81", 4, 5, 7), ("h36m_351", 5, 120, 13)])
def test_whole_track_identity(cfgname, ms, L, a):
    from uplift_upsample_3dhpe_amd import h36m, predict, stream
    cfg, arch, w, model = _model(cfgname)
    S, s_in, pred = stream.session_strides(cfg, ms)
    tracks = _pixel_tracks([L] * T, seed=61)
    poses, fresh = stream.replay_tracks(model, cfg, tracks, resolutions=RES, mask_stride=ms, flip=True, lookahead=a, drain=True)
    plain = stream.replay_tracks(model, cfg, tracks, resolutions=RES, mask_stride=ms, flip=True, lookahead=a)
    rule = np.array([t - a >= 0 and (t - a) % pred == 0 for t in range(L + a)])
    assert rule[a:].sum() == len(range(0, L, pred)) and rule[L:].any()
    whole = predict.predict_tracks(model, cfg, tracks, resolutions=RES, mask_stride=ms, flip=True)
    # Which rows the whole track decides.  A PUSHED row t < L - 1 is the pose of the track cut at t (the session's one rule, tests/test_stream_gpu.py):
    # with lookahead < (SEQUENCE_LENGTH // 2) * SEQUENCE_STRIDE its window hangs over the cut and is padded there, so it is the whole
    # track's pose only where nothing is cut -- the last push, every drained row, and every row when the lookahead is at its maximum.
    # The other pushed rows are held to the bits of the session without a drain, below.
    first_whole = 0 if a == stream.max_lookahead(cfg) else L - 1 - a
    centres = np.array([c for c in range(0, L, pred) if c >= first_whole])
    assert (centres >= L - a).sum() >= 1
    worst = 0.0
    for i in range(T):
        assert poses[i].shape == (L + a, J, 3) and fresh[i].shape == (L + a,) and poses[i].dtype == np.float32
        assert np.array_equal(fresh[i], rule)
        assert np.array_equal(_bits(poses[i][:L]), _bits(plain[0][i])) and np.array_equal(fresh[i][:L], plain[1][i])      # the pushes are today's
        prev = np.concatenate([np.zeros_like(poses[i][:1]), poses[i][:-1]], 0)
        assert np.array_equal(_bits(poses[i][~rule]), _bits(prev[~rule]))                                                   # not fresh: the held pose
        assert np.isfinite(poses[i]).all() and not poses[i][:, cfg.ROOT_KEYTPOINT].any()
        want = whole[i].cpu().numpy()
        d = np.abs(poses[i][a + centres] - want[centres]).reshape(len(centres), -1).max(1)
        worst = max(worst, float(d.max()))
        assert float(np.abs(want[centres]).max()) > 1e-3
    # the oracle pipeline at about ten picked (slot, centre) pairs, the last `a` frames among them
    every = [(i, int(c)) for c in centres for i in range(T)]
    pairs = every if len(every) <= 10 else [every[k] for k in sorted(set(np.linspace(0, len(every) - 1, 10).astype(int).tolist()))]
    assert any(c >= L - a for _, c in pairs)
    norm = [h36m.normalize_screen_coordinates(tracks[i], w=RES[i][0], h=RES[i][1]).astype(np.float32) for i, _ in pairs]
    orc = _oracle_poses(cfg, arch, w, norm, np.array([c for _, c in pairs]), ms)
    d_orc = max(float(np.abs(poses[i][a + c] - orc[k]).max()) for k, (i, c) in enumerate(pairs))
    print(f"{cfgname} s_in {ms} L {L} lookahead {a}: max-abs to predict_tracks on the whole track {worst:.3e}, to the oracle pipeline at "
          f"{pairs} {d_orc:.3e} (bar {util.TOL_MAX_ABS})")
    assert worst <= util.TOL_MAX_ABS and d_orc <= util.TOL_MAX_ABS


def test_bit_identity_with_shorter_lookaheads():
    """Row k - 1 of finish() after L pushes has the bits of the last push of a session with lookahead a - k: the same window, the same
    batch shape, the same features -- only the ring places differ."""
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model = _model("h36m_81")
    L, a, ms = 60, 7, 4
    pred = stream.session_strides(cfg, ms)[2]
    tracks = _pixel_tracks([L] * T, seed=62)
    common = dict(slots=T, resolutions=RES, mask_stride=ms, flip=True)
    s = stream.StreamSession(model, cfg, lookahead=a, **common)
    _push_all(s, tracks)
    rows, fresh = _host(s.finish())
    assert s.check_range() is False and s.frames.cpu().tolist() == [0] * T
    s.close()
    assert rows.shape == (T, a, J, 3) and fresh.shape == (T, a)
    compared = 0
    for k in range(1, a + 1):
        short = stream.StreamSession(model, cfg, lookahead=a - k, **common)
        p, f = _push_all(short, tracks)
        short.close()
        want_fresh = (L - 1 - a + k) % pred == 0
        assert f.tolist() == [want_fresh] * T and fresh[:, k - 1].tolist() == [want_fresh] * T
        if want_fresh:
            same = np.array_equal(_bits(rows[:, k - 1]), _bits(p))
            print(f"k {k}: max-abs {float(np.abs(rows[:, k - 1] - p).max()):.3e}, same bits: {same}")
            assert same, k
            compared += 1
    assert compared >= 1


def test_staggered_ends():
    """Tracks of 30, 45 and 60 frames; finish([i]) when track i ends.  The other slots return, at every later tick, the bits of a session in
    which nothing was finished; the finished slot is at zero frames and takes a new track whose poses equal that track running alone."""
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model = _model("h36m_81")
    lens, a, ms = [30, 45, 60], 7, 4
    ticks = max(lens)
    tracks = _pixel_tracks([ticks] * T, seed=63)                        # (slot i's first track: its first lens[i] frames)
    again = _pixel_tracks([ticks] * T, seed=64)                         # the track a finished slot takes next
    new = lambda: stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=ms, flip=True, lookahead=a)
    s, ref = new(), new()
    got, want, tails = [], [], {}
    for k in range(ticks):
        kp = np.stack([tracks[i][k] if k < lens[i] else again[i][k - lens[i]] for i in range(T)])
        got.append([o.clone() for o in s.push(kp)])
        want.append([o.clone() for o in ref.push(np.stack([t[k] for t in tracks]))])
        for i in range(T):
            if k + 1 == lens[i] and k + 1 < ticks:
                before = s.frames.cpu().tolist()
                tails[i] = [o.clone() for o in s.finish([i])]
                after = s.frames.cpu().tolist()
                assert after[i] == 0 and [after[j] for j in range(T) if j != i] == [before[j] for j in range(T) if j != i]
    assert s.check_range() is False and s.captures == 2 and ref.captures == 1
    s.close()
    ref.close()
    got, want = [torch.stack(c).cpu().numpy() for c in zip(*got)], [torch.stack(c).cpu().numpy() for c in zip(*want)]
    for i in range(T):                                                # untouched by the finishes of the others: the reference's bits
        n = lens[i]
        assert np.array_equal(_bits(got[0][:n, i]), _bits(want[0][:n, i])) and np.array_equal(got[1][:n, i], want[1][:n, i])
    assert got[1][lens[0]:, 2].any() and got[1][lens[1]:, 2].any()
    for i in (0, 1):
        rows, fresh = [o.cpu().numpy() for o in tails[i]]
        others = [j for j in range(T) if j != i]
        assert not rows[others].any() and not fresh[others].any() and fresh[i].any()       # rows of slots that were not chosen: zeros
        # the tail is the one of the track alone; the new track in the slot equals itself running alone in a fresh session
        alone = new()
        solo = [t[:lens[i]] if j == i else np.zeros((lens[i], J, 2), np.float32) for j, t in enumerate(tracks)]
        act = np.array([j == i for j in range(T)])
        _push_all(alone, solo, active=act)
        r, f = _host(alone.finish([i]))
        assert np.array_equal(f[i], fresh[i]) and float(np.abs(r[i] - rows[i]).max()) <= util.TOL_MAX_ABS
        n = ticks - lens[i]
        solo = [again[j][:n] if j == i else np.zeros((n, J, 2), np.float32) for j in range(T)]
        p, f = _push_all(alone, solo, active=act, keep=True)
        alone.close()
        assert np.array_equal(f[:, i], got[1][lens[i]:, i]) and f[:, i].sum() >= 1
        d = float(np.abs(p[:, i] - got[0][lens[i]:, i]).max())
        print(f"slot {i}: the new track against itself alone, max-abs {d:.3e} (bar {util.TOL_MAX_ABS})")
        assert d <= util.TOL_MAX_ABS


def test_graph_and_state():
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model = _model("h36m_81")
    L, a, ms = 33, 7, 4
    tracks = _pixel_tracks([L] * T, seed=65)
    runs = []
    for graph in (True, False):
        s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=ms, flip=True, lookahead=a, graph=graph)
        assert s.captures == int(graph) and s._drain_steps == []
        _push_all(s, tracks)
        assert s.captures == int(graph)
        first = _host(s.finish())
        assert s.captures == 2 * int(graph)
        names = [fn.__name__ for fn, args in s._drain_steps if args is not None]
        assert names == ["uu3d_stream_drain_commit", "uu3d_stream_emit", "uu3d_stream_drain_file"] and len(s._drain_steps) == 4
        _push_all(s, tracks)                                          # a second track in every slot, a second finish: no new capture
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")                       # ... and no host synchronisation, no copy to the host
        try:
            second = s.finish()
            s.push(np.stack([t[0] for t in tracks]))
            third = s.finish([0, 2])
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert s.captures == 2 * int(graph)
        third = _host(third)
        assert s.check_range() is False and s.frames.cpu().tolist() == [0, 1, 0]
        assert not third[1][1].any() and not third[0][1].any()
        runs.append(first)
        s.close()
    assert np.array_equal(runs[0][1], runs[1][1]) and runs[0][1].any() and np.array_equal(_bits(runs[0][0]), _bits(runs[1][0]))
    # lookahead 0: empty second dimensions, only the reset
    s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=ms, flip=True, lookahead=0)
    _push_all(s, tracks, last=3)
    p, f = s.finish()
    assert tuple(p.shape) == (T, 0, J, 3) and tuple(f.shape) == (T, 0) and s.captures == 1 and s.frames.cpu().tolist() == [0] * T
    s.close()


@pytest.mark.parametrize("kind", ["missed", "repair", "coco17"])
def test_options(kind):
    from uplift_upsample_3dhpe_amd import predict, stream
    cfg, arch, w, model = _model("h36m_81")
    L, a, ms = 60, 7, 4
    pred = stream.session_strides(cfg, ms)[2]
    rng = np.random.default_rng(66)
    kw, valid = {}, None
    tracks = _pixel_tracks([L] * T, seed=66)
    if kind == "missed":                                              # missing frames inside the last `a` frames (and before them)
        valid = [np.ones(L, bool) for _ in range(T)]
        for i, gone in enumerate(([L - 3, L - 2], [L - 1, 20], [L - 6, L - 5, L - 4, 8])):
            valid[i][gone] = False
    elif kind == "repair":                                            # a trailing gap of one joint, shorter than G; a closed gap earlier
        kw = {"repair_joints": 5}
        valid = [np.ones((L, J), bool) for _ in range(T)]
        valid[0][L - 3:, 4] = False
        valid[1][L - 4:, 9] = False
        valid[1][30:33, 2] = False
        valid[2][L - 2:, [3, 11]] = False
    else:
        kw = {"keypoints": "coco17"}
        tracks = _pixel_tracks([L] * T, seed=66, J=predict.KEYPOINT_PRESETS["coco17"].inputs)
    s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=ms, flip=True, lookahead=a, missed_detections=kind == "missed", **kw)
    _push_all(s, tracks, valid=valid)
    joint_state = s.joint_state.clone() if kind == "repair" else None
    rows, fresh = _host(s.finish())
    if kind == "repair":
        assert torch.equal(joint_state, s.joint_state) and (joint_state == 2).any()
    assert s.check_range() is False
    s.close()
    whole = predict.predict_tracks(model, cfg, tracks, resolutions=RES, mask_stride=ms, flip=True, **({} if valid is None else {"valid": valid}), **kw)
    plain = predict.predict_tracks(model, cfg, tracks, resolutions=RES, mask_stride=ms, flip=True, **({"keypoints": "coco17"} if kind == "coco17" else {}))
    worst, moved = 0.0, 0.0
    for k in range(1, a + 1):
        c = L - 1 - a + k
        assert fresh[:, k - 1].tolist() == [c % pred == 0] * T
        if c % pred == 0:
            want = np.stack([whole[i][c].cpu().numpy() for i in range(T)])
            worst = max(worst, float(np.abs(rows[:, k - 1] - want).max()))
            moved = max(moved, float(np.abs(want - np.stack([plain[i][c].cpu().numpy() for i in range(T)])).max()))
    print(f"{kind}: drained rows against predict_tracks with the same option, max-abs {worst:.3e} (bar {util.TOL_MAX_ABS}); the option moves "
          f"those poses by {moved:.3e}")
    assert worst <= util.TOL_MAX_ABS
    assert kind == "coco17" or moved > util.TOL_MAX_ABS                  # (the option shows in the drained frames)


@pytest.mark.parametrize("smooth", [None, True])
def test_camera_and_smooth_equal_the_mirrors(smooth):
    from uplift_upsample_3dhpe_amd import predict, stream
    cfg, arch, w, model = _model("h36m_81")
    L, a, ms, m = 40, 7, 4, 6
    pred = stream.session_strides(cfg, ms)[2]
    tracks = _pixel_tracks([L] * T, seed=67)
    s = stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=ms, flip=True, lookahead=a, camera=CAMERAS, min_root_joints=m,
                             **({} if smooth is None else {"smooth": smooth}))
    raw = []
    for k in range(L):
        out = s.push(np.stack([t[k] for t in tracks]))
        raw.append([o.clone() for o in (s.raw_poses, out[1], s.raw_roots, out[3], out[0], out[2])])
    out = _host(s.finish())
    raw_rows, raw_roots = s.drain_raw_poses.cpu().numpy(), s.drain_raw_roots.cpu().numpy()
    names = [fn.__name__ for fn, args in s._drain_steps if args is not None]
    assert names == ["uu3d_stream_drain_commit", "uu3d_stream_emit", "uu3d_stream_root_drain"] + ["uu3d_stream_one_euro"] * (2 if smooth else 0) + ["uu3d_stream_drain_file"]
    assert s.check_range() is False and s.captures == 2
    s.close()
    poses, fresh, roots, states, f_poses, f_roots = [torch.stack(c).cpu().numpy() for c in zip(*raw)]
    assert out[0].shape == (T, a, J, 3) and out[2].shape == (T, a, 3) and out[3].shape == (T, a) and out[3].dtype == np.uint8
    if smooth is None:
        assert np.array_equal(_bits(out[0]), _bits(raw_rows)) and np.array_equal(_bits(out[2]), _bits(raw_roots))
    seen = set()
    for i in range(T):
        host = stream.LiveRootHost(J, a, CAMERAS[i], m)
        for k in range(L):
            r, st = host.step(tracks[i][k], None, poses[k, i] if fresh[k, i] else None)
            assert st == states[k, i] and np.array_equal(_bits(r), _bits(roots[k, i]))
        for k in range(1, a + 1):
            r, st = host.drain(raw_rows[i, k - 1] if out[1][i, k - 1] else None)
            assert out[1][i, k - 1] == ((L - 1 - a + k) % pred == 0)
            assert st == out[3][i, k - 1] and np.array_equal(_bits(r), _bits(raw_roots[i, k - 1])), (i, k)
            seen.add(int(st))
    assert 1 in seen
    if smooth is not None:
        filt = predict.OneEuro()
        for values, rows, got_push, got_rows, state_of in ((poses.reshape(L, T, -1), raw_rows.reshape(T, a, -1), f_poses.reshape(L, T, -1),
                                                            out[0].reshape(T, a, -1), None),
                                                           (roots, raw_roots, f_roots, out[2], (states, out[3]))):
            host = stream.LiveOneEuroHost(T, values.shape[-1], 50, filt, a)
            for k in range(L):
                want = host.step(values[k], [k + 1] * T, fresh[k], None, None if state_of is None else state_of[0][k])
                assert np.array_equal(_bits(want), _bits(got_push[k])), k
            for k in range(1, a + 1):
                want = host.drain(rows[:, k - 1], [L] * T, [k] * T, out[1][:, k - 1], None, None if state_of is None else state_of[1][:, k - 1])
                assert np.array_equal(_bits(want), _bits(got_rows[:, k - 1])), k
        assert not np.array_equal(_bits(out[0]), _bits(raw_rows))


def test_replay_detections_drain():
    """20 frames, 2 people, lookahead 7: every track alive at the end gains 7 rows, the bits of finish() on a missed_detections session
    driven by associate_host."""
    from uplift_upsample_3dhpe_amd import predict, stream
    cfg, arch, w, model = _model("h36m_81")
    frames, D, a = 20, 2, 7
    rng = np.random.default_rng(68)
    body = rng.uniform(-1.0, 1.0, size=(J, 2)) * [50.0, 100.0]
    dets = np.zeros((frames, D, J, 2), np.float32)
    for t in range(frames):
        people = [body + [300.0 + 5.0 * t, 400.0] + rng.uniform(-2, 2, size=(J, 2)), body + [1200.0 - 5.0 * t, 600.0] + rng.uniform(-2, 2, size=(J, 2))]
        for d, p in zip(rng.permutation(D), people):
            dets[t, d] = p
    counts = np.full(frames, D, np.int32)
    rule = dict(max_age=2, max_dist=0.5, min_common=3)
    common = dict(resolutions=(1920, 1080), mask_stride=4, flip=True, lookahead=a)
    plain = stream.replay_detections(model, cfg, dets, counts, slots=D, **rule, **common)
    live = stream.replay_detections(model, cfg, dets, counts, slots=D, drain=True, **rule, **common)
    want = predict.associate_host(dets, counts, slots=D, **rule)
    assert want.num_tracks == 2 and (want.track_ids[-1] >= 0).all()
    ref = stream.StreamSession(model, cfg, slots=D, missed_detections=True, **common)
    for t in range(frames):
        kp = np.zeros((D, J, 2), np.float32)
        for sl in range(D):
            if want.slot_det[t, sl] >= 0:
                kp[sl] = dets[t, want.slot_det[t, sl]]
        if want.born[t].any():
            ref.reset(slots=np.flatnonzero(want.born[t]))
        ref.push(kp, active=want.alive[t] != 0, valid=want.slot_full[t])
    rows, fresh = _host(ref.finish())
    ref.close()
    assert len(live) == len(plain) == 2 and fresh.any()
    for (tid, first, p, f), (tid0, first0, p0, f0) in zip(live, plain):
        slot = int(np.flatnonzero(want.track_ids[-1] == tid)[0])
        assert (tid, first) == (tid0, first0) and len(p) == len(p0) + a and len(f) == len(f0) + a
        assert np.array_equal(_bits(p[:-a]), _bits(p0)) and np.array_equal(f[:-a], f0)
        assert np.array_equal(_bits(p[-a:]), _bits(rows[slot])) and np.array_equal(f[-a:], fresh[slot])
