"""GPU: world space on the device (include/uu3d.h, WORLD SPACE; camera.py), with h36m_81 at mask stride 4 and seeded weights.  The reference
is predict.camera_to_world_host, the rule in numpy (tests/test_world_cpu.py pins it to h36m.camera_to_world); every comparison is on the
bits, NaN positions compared separately.
  1. predict.camera_to_world equals the mirror: (rows, J) = (1, 1), (19, 17) -- 342 points, a partial second block --, (11, 25), three
     tracks of 5 / 1 / 13 rows with three cameras; NaN poses, root states 0, 1 and 2; poses only, roots only, in place
  2. predict_tracks(camera=Camera with distortion and extrinsics) equals joint_rotations_host(one_euro_host(camera_to_world_host(the call
     with the Camera minus extrinsics and smooth=None, rotations=None))) in every form of the call, bare and with bones / smooth /
     rotations; predict_detections likewise per track
  3. StreamSession: every push and every finish() row of a session with extrinsics is camera_to_world_host of the session without, beside
     it on the same frames; smooth and rotations read the world buffers; captures stays 1
  4. a Camera without extrinsics launches nothing new, offline and live"""
import numpy as np
import pytest

from tests.test_distortion_cpu import SETS
from tests.test_distortion_gpu import _all_same, _host, _lens_tracks, _same, _two_people
from tests.tracks_util import RES, _model

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
MS, S, J17 = 4, 3, 17
LENS = [23, 40, 61]
POSES = [((0.81, -0.53, 0.2, 0.15), (1.8, 4.9, 1.6)), ((-0.14, 0.15, 0.76, -0.62), (-4.5, 3.7, 1.4)), ((0.05, 0.7, -0.7, 0.1), (0.25, -5.0, 2.75))]


def _cameras(scale=1.2, distortion=True):
    """One Camera per entry of RES, tilted and rolled, metres from the origin; the intrinsics of tests.test_distortion_gpu._cameras."""
    from uplift_upsample_3dhpe_amd import predict
    return [predict.Camera(scale * w, scale * w + 3.5, 0.5 * w + 0.25, 0.5 * h - 0.75, distortion=SETS[i % len(SETS)] if distortion else None,
                           orientation=POSES[i][0], translation=POSES[i][1]) for i, (w, h) in enumerate(RES)]


def _minus(cams):
    return [c.without(extrinsics=True) for c in cams]


# ---- 1. the launch alone ---------------------------------------------------------------------------------------------------------------
def _scene(rows, J, seed):
    rng = np.random.default_rng(seed)
    poses = rng.normal(0.0, 0.6, size=(rows, J, 3)).astype(np.float32)
    poses[:, 0] = 0.0
    roots = rng.normal(0.0, 3.0, size=(rows, 3)).astype(np.float32)
    state = ((np.arange(rows) + 2) % 3).astype(np.uint8)                # 0, 1 and 2 present from three rows on; one row: held (2)
    roots[state == 0] = 0.0
    if rows > 4:
        poses[2], poses[4, J // 2, 1], roots[3, 0] = np.nan, np.nan, np.nan
    return poses, roots, state


@pytest.mark.parametrize("shape", [(1, 1), (19, 17), (11, 25), "tracks"])
def test_camera_to_world_equals_the_mirror(shape):
    from uplift_upsample_3dhpe_amd import predict
    cams = _cameras()
    if shape == "tracks":
        rows, J, lens, camera = 19, 17, [5, 1, 13], cams
    else:
        (rows, J), lens, camera = shape, None, cams[1]
    poses, roots, state = _scene(rows, J, 40 + rows)
    want_p, want_r = predict.camera_to_world_host(poses, roots, state, camera, lens=lens)
    whole = ~np.isnan(poses[:, 0]).any(axis=1)                          # (a NaN pose is NaN at its root joint as well)
    assert (J == 1 or not _same(want_p, poses)) and not _same(want_r, roots) and not want_p[whole, 0].any() and not want_r[state == 0].any()
    dp, dr, ds = torch.from_numpy(poses).cuda(), torch.from_numpy(roots).cuda(), torch.from_numpy(state).cuda()
    before = dp.clone(), dr.clone()
    got_p, got_r = predict.camera_to_world(dp, dr, ds, camera, lens=lens)
    assert got_p.dtype == got_r.dtype == torch.float32 and tuple(got_p.shape) == poses.shape and tuple(got_r.shape) == roots.shape
    assert got_p.data_ptr() != dp.data_ptr() and got_r.data_ptr() != dr.data_ptr()
    assert _same(got_p, want_p) and _same(got_r, want_r)
    assert np.array_equal(_host(got_p)[whole, 0].view(np.uint32), np.zeros((int(whole.sum()), 3), np.uint32))       # +0.0
    assert _same(dp, before[0]) and _same(dr, before[1])                                                            # only read
    # poses only, roots only
    only_p, none = predict.camera_to_world(dp, None, None, camera, lens=lens)
    assert none is None and _same(only_p, want_p)
    none, only_r = predict.camera_to_world(None, dr, ds, camera, lens=lens)
    assert none is None and _same(only_r, want_r)
    # in place: every lane reads its own element before it writes it
    rows7 = np.stack([c.pose_row() for c in (camera if lens is not None else [camera])])
    same_p, same_r = predict.camera_to_world_rows(dp, dr, ds, rows7, lens, in_place=True)
    assert same_p.data_ptr() == dp.data_ptr() and same_r.data_ptr() == dr.data_ptr() and _same(dp, want_p) and _same(dr, want_r)
    with pytest.raises(ValueError):
        predict.camera_to_world(torch.from_numpy(poses), None, None, camera, lens=lens)                             # a host tensor
    with pytest.raises(ValueError):
        predict.camera_to_world(dp, dr, None, camera, lens=lens)
    with pytest.raises(ValueError):
        predict.camera_to_world(dp, None, None, camera.without(extrinsics=True) if lens is None else cams[:2], lens=lens)


# ---- 2. offline -------------------------------------------------------------------------------------------------------------------------
FORMS = {"plain": ({}, 50), "keyframes_only": (dict(keyframes_only=True, lengths=LENS), 50), "fps30": (dict(fps=30), 30),
         "fps25_out50": (dict(fps=25, out_fps=50), 50), "finite_repair2": (dict(valid="finite", repair_joints=2), 50),
         "coco17": (dict(keypoints="coco17"), 50), "cubic": (dict(interpolation="cubic"), 50)}


def _world_of(ref, cams, rate, full):
    """The section's invariant: what the call with extrinsics must return, from the call without them (poses, roots, root_state)."""
    from uplift_upsample_3dhpe_amd import predict
    lens = [int(p.shape[0]) for p in ref[0]]
    poses, roots, state = (_host(torch.cat(r, 0)) for r in ref)
    wp, wr = predict.camera_to_world_host(poses, roots, state, cams, lens=lens)
    if not full:
        return (wp, wr, state), lens
    pose_filter, root_filter = predict.check_smooth(True, True)
    wp = predict.one_euro_host(wp, lens, rate, pose_filter)
    wr = predict.one_euro_host(wr, lens, rate, root_filter, state=state)
    return (wp, wr, state, predict.joint_rotations_host(wp)[0]), lens


@pytest.mark.parametrize("form", list(FORMS))
def test_predict_tracks_is_the_world_of_the_call_without_extrinsics(form):
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model("h36m_81")
    more, rate = FORMS[form]
    kw = dict(resolutions=RES, mask_stride=MS, **more)
    cams = _cameras()
    tracks = _lens_tracks(LENS, 71, cams)
    if form == "finite_repair2":
        tracks[0][3, 2], tracks[1][10:12, 5], tracks[2][20, 7, 1], tracks[2][30] = np.nan, np.nan, np.inf, np.nan
    if form == "keyframes_only":
        tracks = [t[::MS] for t in tracks]
    for full in (False, True):
        extra = dict(bones="track") if full else {}
        ref = predict.predict_tracks(model, cfg, tracks, camera=_minus(cams), **extra, **kw)
        assert isinstance(ref, tuple) and len(ref) == 3
        want, lens = _world_of(ref, cams, rate, full)
        got = predict.predict_tracks(model, cfg, tracks, camera=cams, **extra, **(dict(smooth=True, rotations=True) if full else {}), **kw)
        assert len(got) == len(want) and [int(p.shape[0]) for p in got[0]] == lens
        for name, g, r in zip(("poses", "roots", "root_state", "rotations"), got, want):
            assert _same(torch.cat(g, 0), r), (form, full, name)
        state = want[2]
        print(f"{form} full={full}: root states 0 / 1 / 2: {np.bincount(state, minlength=3).tolist()}")
        assert (state == 1).any() and not _same(torch.cat(got[0], 0), torch.cat(ref[0], 0)) and not _same(torch.cat(got[1], 0), torch.cat(ref[1], 0))
        assert not _host(torch.cat(got[0], 0))[:, int(cfg.ROOT_KEYTPOINT)].any() or full          # (unfiltered: the root joint's zeros)
    if form == "plain":
        # the Camera minus extrinsics is the Camera that never had any; one Camera for all tracks
        fresh = [predict.Camera(*c.intrinsics, distortion=c.distortion, tol=c.tol) for c in cams]
        assert _all_same(predict.predict_tracks(model, cfg, tracks, camera=_minus(cams), **kw), predict.predict_tracks(model, cfg, tracks, camera=fresh, **kw))
        one = predict.predict_tracks(model, cfg, tracks, camera=cams[1], **kw)
        want, _ = _world_of(predict.predict_tracks(model, cfg, tracks, camera=cams[1].without(extrinsics=True), **kw), cams[1:2] * 3, rate, False)
        assert all(_same(torch.cat(g, 0), r) for g, r in zip(one, want))
        with pytest.raises(ValueError, match="all have extrinsics or all have none"):
            predict.predict_tracks(model, cfg, tracks, camera=[cams[0], _minus(cams)[1], cams[2]], **kw)


def test_predict_detections_is_the_world_of_the_call_without_extrinsics():
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model("h36m_81")
    cams = [predict.Camera(1.1 * 1920, 1.1 * 1920 + 2.0, 960.5, 539.25, distortion=SETS[2], orientation=POSES[0][0], translation=POSES[0][1]),
            predict.Camera(1.3 * 1920, 1.3 * 1920, 958.0, 541.0, distortion=SETS[0], orientation=POSES[1][0], translation=POSES[1][1])]
    people = _two_people()
    dets = [predict.distort_points_host(people, cams[0]).astype(np.float32), predict.distort_points_host(people[:20], cams[1]).astype(np.float32)]
    kw = dict(slots=2, resolutions=(1920, 1080), mask_stride=MS)
    for full in (False, True):
        extra = dict(bones="track") if full else {}
        ref = predict.predict_detections(model, cfg, dets, camera=_minus(cams), **extra, **kw)
        got = predict.predict_detections(model, cfg, dets, camera=cams, **extra, **(dict(smooth=True, rotations=True) if full else {}), **kw)
        assert [len(v) for v in got] == [2, 2]
        for v, (video, ref_video) in enumerate(zip(got, ref)):
            for person, base in zip(video, ref_video):
                assert person[:2] == base[:2] and len(person) == (6 if full else 5)
                want, _ = _world_of([[t] for t in base[2:]], cams[v], 50, full)
                assert all(_same(g, r) for g, r in zip(person[2:], want)), (full, v, person[:2])
                assert not _same(person[2], base[2])
    # one Camera for both videos
    one = predict.predict_detections(model, cfg, dets, camera=cams[0], **kw)
    base = predict.predict_detections(model, cfg, dets, camera=cams[0].without(extrinsics=True), **kw)
    for video, ref_video in zip(one, base):
        for person, b in zip(video, ref_video):
            assert all(_same(g, r) for g, r in zip(person[2:], _world_of([[t] for t in b[2:]], cams[0], 50, False)[0]))


# ---- 3. live ----------------------------------------------------------------------------------------------------------------------------
TICKS = 60


@pytest.mark.parametrize("form", ["one_camera", "per_slot", "per_slot_fps30"])
def test_session_is_the_world_of_the_session_without_extrinsics(form):
    from uplift_upsample_3dhpe_amd import predict, stream
    cfg, arch, w, model = _model("h36m_81")
    fps = 30 if form.endswith("fps30") else None
    rate = 50 if fps is None else fps
    a = 2 if fps is None else max(2, stream.rate_plan(cfg, fps, None, MS).min_lookahead)
    cams = _cameras()
    frames = _lens_tracks([TICKS] * S, 81, cams)
    camera = cams if form != "one_camera" else cams[1]
    each = cams if form != "one_camera" else [cams[1]] * S
    minus = _minus(cams) if form != "one_camera" else cams[1].without(extrinsics=True)
    common = dict(slots=S, resolutions=RES, mask_stride=MS, flip=True, lookahead=a, **({} if fps is None else {"fps": fps}))
    ref = stream.StreamSession(model, cfg, camera=minus, **common)
    s = stream.StreamSession(model, cfg, camera=camera, **common)
    full = stream.StreamSession(model, cfg, camera=camera, smooth=True, rotations=True, **common)
    assert not hasattr(ref, "_world") and ref.world is None and s.world.shape == (S, 7)
    table = lambda t: [fn.__name__ for fn, args in (t._tick_steps if fps is None else t._push_after) if args is not None]
    at = table(ref).index("uu3d_stream_root")
    assert table(s) == table(ref)[:at + 1] + ["uu3d_camera_to_world"] + table(ref)[at + 1:]                         # directly behind the root solve
    assert table(full) == table(s) + ["uu3d_stream_one_euro"] * 2 + ["uu3d_joint_rotations"]
    pose_filter, root_filter = predict.check_smooth(True, True)
    hp, hq = stream.LiveOneEuroHost(S, 3 * J17, rate, pose_filter, a), stream.LiveOneEuroHost(S, 3, rate, root_filter, a)
    rows = []
    for k in range(TICKS):
        kp = np.stack([f[k] for f in frames])
        out = [[t.clone() for t in x.push(kp)] for x in (ref, s, full)]
        assert ref.captures == s.captures == full.captures == 1
        rows.append([[_host(t) for t in o] for o in out] + [[_host(t.clone()) for t in (ref.raw_poses, ref.raw_roots, s.raw_poses, s.raw_roots,
                     s.camera_poses, s.camera_roots, full.raw_poses, full.raw_roots, full.source_frames)]])
    for k, (r, g, f, (ref_p, ref_r, raw_p, raw_r, cam_p, cam_r, full_p, full_r, count)) in enumerate(rows):
        assert len(r) == len(g) == 4 and len(f) == 5
        assert np.array_equal(r[1], g[1]) and np.array_equal(r[3], g[3]) and np.array_equal(r[1], f[1]) and np.array_equal(r[3], f[3]), k
        want_p, want_r = predict.camera_to_world_host(r[0], r[2], r[3], each, lens=[1] * S)
        assert _same(g[0], want_p) and _same(g[2], want_r), k
        assert _same(raw_p, want_p) and _same(raw_r, want_r) and _same(cam_p, ref_p) and _same(cam_r, ref_r), k
        assert _same(ref_p, r[0]) and _same(ref_r, r[2]) and _same(full_p, want_p) and _same(full_r, want_r), k
        ones = np.ones(S, bool)
        assert _same(f[0], hp.step(want_p.reshape(S, -1), count, r[1], ones).reshape(S, J17, 3)), k
        assert _same(f[2], hq.step(want_r, count, r[1], ones, r[3])), k
        assert _same(f[4], predict.joint_rotations_host(f[0])[0]), k
    fresh, states = np.stack([r[0][1] for r in rows]), np.stack([r[0][3] for r in rows])
    print(f"{form} lookahead {a}: fresh {int(fresh.sum())}, root states 0 / 1 / 2: {np.bincount(states.ravel(), minlength=3).tolist()}")
    assert fresh.all(axis=0).any() or fresh.sum(axis=0).min() >= 3
    assert (states != 0).any() and not all(_same(r[1][0], r[0][0]) for r in rows)
    if fps is None:                                                      # finish(): the same step behind uu3d_stream_root_drain
        tails = [[_host(t.clone()) for t in x.finish()] for x in (ref, s, full)]
        assert ref.captures == s.captures == full.captures == 2
        names = [fn.__name__ for fn, args in s._drain_steps if args is not None]
        assert names[names.index("uu3d_stream_root_drain") + 1] == "uu3d_camera_to_world"
        t0, t1, t2 = tails
        assert t1[0].shape == (S, a, J17, 3) and np.array_equal(t0[1], t1[1]) and np.array_equal(t0[3], t1[3]) and np.array_equal(t0[1], t2[1])
        flat = lambda x: x.reshape((S * a,) + x.shape[2:])
        want_p, want_r = predict.camera_to_world_host(flat(t0[0]), flat(t0[2]), flat(t0[3]), each, lens=[a] * S)
        assert _same(flat(t1[0]), want_p) and _same(flat(t1[2]), want_r)
        assert _same(flat(_host(s.drain_raw_poses)), want_p) and _same(flat(_host(s.drain_raw_roots)), want_r)
        assert _same(s.drain_camera_poses, t0[0]) and _same(s.drain_camera_roots, t0[2]) and _same(ref.drain_raw_poses, t0[0])
        assert _same(flat(_host(full.drain_raw_poses)), want_p) and _same(flat(_host(full.drain_raw_roots)), want_r)
        want_p, want_r, count = want_p.reshape(S, a, -1), want_r.reshape(S, a, 3), rows[-1][3][-1]
        for row in range(a):
            drained, ones = np.full(S, row + 1), np.ones(S, bool)
            assert _same(t2[0][:, row], hp.drain(want_p[:, row], count, drained, t0[1][:, row], ones).reshape(S, J17, 3)), row
            assert _same(t2[2][:, row], hq.drain(want_r[:, row], count, drained, t0[1][:, row], ones, t0[3][:, row])), row
        assert _same(flat(t2[4]), predict.joint_rotations_host(flat(t2[0]))[0]) and t0[1].any()
    for x in (ref, s, full):
        assert x.check_range() is False
        x.close()


# ---- 4. without extrinsics ----------------------------------------------------------------------------------------------------------------
def test_a_camera_without_extrinsics_launches_nothing_new():
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model = _model("h36m_81")
    cams = _minus(_cameras())
    s = stream.StreamSession(model, cfg, slots=S, resolutions=RES, mask_stride=MS, flip=True, lookahead=2, camera=cams, smooth=True)
    try:
        names = [fn.__name__ for fn, args in s._tick_steps if args is not None]
        assert "uu3d_camera_to_world" not in names and s.world is None and not any(isinstance(st, stream.LiveWorld) for st in s._post)
        world, camera = s._scenes["world"], s._scenes["camera"]
        assert world.poses is camera.poses and world.roots is camera.roots and s.raw_roots is s.camera_roots and s.raw_poses is s.camera_poses
    finally:
        s.close()
    plain = stream.StreamSession(model, cfg, slots=S, resolutions=RES, mask_stride=MS, flip=True)
    try:
        for name in ("camera_poses", "camera_roots", "raw_roots"):
            with pytest.raises(AttributeError):
                getattr(plain, name)
    finally:
        plain.close()
