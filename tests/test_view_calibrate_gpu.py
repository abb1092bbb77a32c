"""GPU: where the cameras stand, on the device (include/uu3d.h, WHERE THE CAMERAS STAND; views.py).  The references are the rules in numpy,
predict.view_moment_sums_host, predict.view_position_sums_host, predict.solve_view_pose_host and predict.calibrate_views_host
(tests/test_view_calibrate_cpu.py pins them against the truth of seeded scenes and against np.linalg.eigh); every comparison is on the bits.
  1. the three launches alone on random inputs: R in {1, 255, 256, 257, 4096, 4097, 8193} (one lane, the edges of the 256 lanes and of the
     4096-row chunks, three chunks), V in {1, 2, 3, 8}, J 17 and 13, with and without flags, NaN and Inf keypoints, a view without terms, a
     chunk without terms, a view the first stage refused; the inputs are unchanged afterwards
  2. predict.calibrate_views equals predict.calibrate_views_host on the seeded scenes of tests/view_calibrate_util.py, one and two persons
  3. every guard of the C ABI returns its code and leaves the outputs alone
  4. predict_views(calibrate=True) (h36m_81 at mask stride 4, seeded weights, 3 views, 2 persons of 60 and 80 frames) equals, bit for bit,
     the call on the cameras it returns, and those equal the host composition on predict_tracks of the flattened tracks: plain, with
     triangulate=True, with valid="finite" and repair_joints, with keypoints="coco17", with align=[0, -3, 5], with a lens
  5. predict_views(calibrate=None) returns the bits of the call without the keyword and of the parent's host composition
  6. a view that cannot be calibrated is a ValueError that names it"""
import ctypes as C

import numpy as np
import pytest

from tests import view_calibrate_util as CU
from tests import views_util as VU
from tests.test_distortion_gpu import _host, _same
from tests.tracks_util import _model

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
MS, J17 = 4, 17
LENS = [60, 80]
ROWS = (1, 255, 256, 257, 4096, 4097, 8193)
VIEWS = (1, 2, 3, 8)


def _bits(a, b):
    a, b = _host(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _made_up_pose(V, seed):
    """Rows as the first stage writes them: random unit quaternions with w >= 0, zeros, state 1 -- and state 0 for view 1 of three or more."""
    rng = np.random.default_rng(seed)
    pose = np.zeros((V, 8), np.float64)
    q = rng.normal(0.0, 1.0, (V, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    pose[:, :4] = np.where(q[:, :1] < 0, -q, q)
    pose[0, :4] = (1.0, 0.0, 0.0, 0.0)
    pose[:, 7] = 1.0
    if V >= 3:
        pose[1, 7] = 0.0
    return pose


# ---- 1. the launches alone -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", VIEWS)
@pytest.mark.parametrize("R", ROWS)
def test_the_launches_equal_the_mirrors(R, V):
    from uplift_upsample_3dhpe_amd import predict, views
    J = 17 if (ROWS.index(R) + VIEWS.index(V)) % 2 == 0 else 13
    for with_flags in (True, False):
        poses, kp, flags, intr = CU.random_inputs(V, R, J, 100 * R + V, with_flags)
        dp, dk = torch.from_numpy(poses).cuda(), torch.from_numpy(kp).cuda()
        df = None if flags is None else torch.from_numpy(flags).cuda()
        before = dp.clone(), dk.clone(), None if df is None else df.clone()
        m = VU.min_joints(J)
        # the rotation sums
        want = predict.view_moment_sums_host(poses, kp, flags, m)
        got = predict.view_moment_sums(dp, dk, df, m)
        assert got.dtype == torch.float64 and tuple(got.shape) == (V, views.calibrate_chunks(R), 10)
        assert _bits(got, want), ("moment sums", R, V, J, with_flags)
        if V >= 3 and R >= 255:
            assert not want[V - 1, :, 9].any() and want[1, 0, 9] > 0      # a view without terms beside one with
        if R > 4096:
            assert not want[:, 1].any() and (V == 1 or want[1, 0, 9] > 0)  # a chunk without terms
        # the first stage, on the device's sums
        for min_terms in (1, 50):
            want_pose, want_terms = predict.solve_view_pose_host(want, None, min_terms)
            got_pose, got_terms = predict.solve_view_pose(got, None, min_terms)
            assert got_pose.dtype == torch.float64 and got_terms.dtype == torch.int32
            assert _bits(got_pose, want_pose) and _bits(got_terms, want_terms), ("first stage", R, V, J, with_flags, min_terms)
        # the position sums, on a made-up first stage and on the real one
        for pose in (_made_up_pose(V, R + V), want_pose):
            dq = torch.from_numpy(pose).cuda()
            want_sums = predict.view_position_sums_host(poses, kp, intr, pose, flags, m)
            got_sums = predict.view_position_sums(dp, dk, intr, dq, df, m)
            assert _bits(got_sums, want_sums), ("position sums", R, V, J, with_flags)
            assert _bits(dq, pose)                                                                                    # only read
            want_placed, want_n = predict.solve_view_pose_host(want_sums, pose)
            got_placed, got_n = predict.solve_view_pose(got_sums, dq)
            assert _bits(got_placed, want_placed) and _bits(got_n, want_n), ("second stage", R, V, J, with_flags)
            assert _bits(dq, pose)
        if V >= 3:
            assert not want_sums[0].any() and not predict.view_position_sums_host(poses, kp, intr, _made_up_pose(V, 1), flags, m)[1].any()
        # the whole stage
        want_all = predict.calibrate_views_host(poses, kp, intr, flags, m, 1)
        got_all = predict.calibrate_views(dp, dk, intr, df, m, 1)
        assert _bits(got_all[0], want_all[0]) and _bits(got_all[1], want_all[1])
        assert _bits(dp, _host(before[0])) and _bits(dk, _host(before[1])) and (df is None or _bits(df, _host(before[2])))
    if (R, V) == (257, 3):
        print(f"R {R} V {V}: states {want_all[0][:, 7].tolist()}, terms {want_all[1].tolist()}")
        # the wrappers' refusals, on inputs of their own
        poses, kp, flags, intr = CU.random_inputs(V, R, J, 7, True)
        dp, dk, df = (torch.from_numpy(a).cuda() for a in (poses, kp, flags))
        dq = torch.from_numpy(_made_up_pose(V, 7)).cuda()
        got = predict.view_moment_sums(dp, dk, df)
        with pytest.raises(ValueError):
            predict.view_moment_sums(dp.cpu(), dk, df)                                                                # a host tensor
        with pytest.raises(ValueError):
            predict.view_position_sums(dp, dk, intr[:2], dq, df)
        with pytest.raises(ValueError):
            predict.view_position_sums(dp, dk, intr, dq[:2], df)
        with pytest.raises(ValueError):
            predict.solve_view_pose(got.float())
        with pytest.raises(ValueError):
            predict.solve_view_pose(got, dq, min_terms=0)


# ---- 2. the stage on the seeded scenes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c + (1.0, False) for c in CU.EXACT] + [c + (True,) for c in CU.NOISY], ids=lambda c: "-".join(str(x) for x in c))
def test_calibrate_views_equals_the_mirror_on_the_seeded_scenes(case):
    from uplift_upsample_3dhpe_amd import predict
    s, pose, terms = CU.host_rules(*case)
    dp, dk = torch.from_numpy(s["poses"].copy()).cuda(), torch.from_numpy(s["kp"].copy()).cuda()
    got_pose, got_terms = predict.calibrate_views(dp, dk, s["bare"])
    assert tuple(got_pose.shape) == (s["V"], 8) and tuple(got_terms.shape) == (s["V"],)
    assert _bits(got_pose, pose) and _bits(got_terms, terms), case
    assert (pose[:, 7] == 1.0).all() and (terms[1:] == s["R"]).all()                                                  # not compared on refusals
    cams = predict.calibrated_cameras(s["bare"], _host(got_pose))
    assert all(c.has_extrinsics for c in cams) and len(cams) == s["V"]


# ---- 3. the guards -------------------------------------------------------------------------------------------------------------------------
def test_every_guard_returns_its_code_and_leaves_the_outputs_alone():
    from uplift_upsample_3dhpe_amd import _capi
    lib = _capi.load_library()
    V, R, J = 2, 10, 5
    poses = torch.zeros((V * R * J * 3 + 1,), dtype=torch.float32, device="cuda")
    kp = torch.zeros((V, R, J, 2), dtype=torch.float32, device="cuda")
    intr = torch.ones((V * 4 + 1,), dtype=torch.float64, device="cuda")
    pose = torch.zeros((V * 8 + 1,), dtype=torch.float64, device="cuda")
    partial = torch.full((V * 10 + 1,), -7.0, dtype=torch.float64, device="cuda")
    out = torch.full((V * 8 + 1,), -7.0, dtype=torch.float64, device="cuda")
    terms = torch.full((V + 1,), 9, dtype=torch.int32, device="cuda")
    p = (lambda t, o=0: C.c_void_p(t.data_ptr() + o))
    assert lib.uu3d_view_calibrate_chunks(0) == 0 and lib.uu3d_view_calibrate_chunks(4096) == 1 and lib.uu3d_view_calibrate_chunks(4097) == 2
    assert lib.uu3d_view_calibrate_chunks(2 ** 31) == 0
    good = dict(poses=p(poses), kp=p(kp), flags=None, views=V, rows=R, J=J, m=3, partial=p(partial))
    cases = [(dict(views=9), 2), (dict(J=65), 2), (dict(views=0), 1), (dict(J=0), 1), (dict(rows=0), 1), (dict(rows=2 ** 31), 1), (dict(m=1), 1),
             (dict(poses=None), 1), (dict(kp=None), 1), (dict(partial=None), 1), (dict(poses=p(poses, 2)), 1), (dict(kp=p(kp, 4)), 1),
             (dict(partial=p(partial, 4)), 1)]
    order = ("poses", "kp", "flags", "views", "rows", "J", "m", "partial")
    for change, code in cases:
        args = dict(good)
        args.update(change)
        assert lib.uu3d_view_moment_sums(*[args[k] for k in order], None) == code, change
    good = dict(poses=p(poses), kp=p(kp), flags=None, views=V, rows=R, J=J, intr=p(intr), m=3, pose=p(pose), partial=p(partial))
    cases += [(dict(intr=None), 1), (dict(pose=None), 1), (dict(intr=p(intr, 4)), 1), (dict(pose=p(pose, 4)), 1)]
    order = ("poses", "kp", "flags", "views", "rows", "J", "intr", "m", "pose", "partial")
    for change, code in cases:
        args = dict(good)
        args.update(change)
        assert lib.uu3d_view_position_sums(*[args[k] for k in order], None) == code, change
    good = dict(partial=p(partial), views=V, chunks=1, stage=1, min_terms=1, pose=p(pose), out=p(out), terms=p(terms))
    cases = [(dict(views=9), 2), (dict(views=0), 1), (dict(chunks=0), 1), (dict(chunks=2 ** 20), 1), (dict(stage=2), 1), (dict(stage=-1), 1),
             (dict(min_terms=0), 1), (dict(partial=None), 1), (dict(pose=None), 1), (dict(out=None), 1), (dict(terms=None), 1), (dict(out=p(pose)), 1),
             (dict(partial=p(partial, 4)), 1), (dict(pose=p(pose, 4)), 1), (dict(out=p(out, 4)), 1), (dict(terms=p(terms, 2)), 1)]
    order = ("partial", "views", "chunks", "stage", "min_terms", "pose", "out", "terms")
    for change, code in cases:
        args = dict(good)
        args.update(change)
        assert lib.uu3d_solve_view_pose(*[args[k] for k in order], None) == code, change
    torch.cuda.synchronize()
    assert (partial == -7.0).all() and (out == -7.0).all() and (terms == 9).all()


# ---- 4. predict_views(calibrate=True) ------------------------------------------------------------------------------------------------------
def _views(cams, seed, K=J17):
    """Two persons who walk and turn, 60 and 80 frames, seen by every camera: views[v][i] (T_i, K, 2) float32 pixels."""
    joints, _ = CU.walkers(2, LENS[1], K, np.random.default_rng(seed))
    world = [joints[:LENS[0]], joints[LENS[1]:]]
    views = [[] for _ in cams]
    for v, c in enumerate(cams):
        for w in world:
            px = VU.project(w, c)[0]
            views[v].append((px if not c.has_distortion else predict_distort(px, c)).astype(np.float32))
    return views


def predict_distort(px, cam):
    from uplift_upsample_3dhpe_amd import predict
    return predict.distort_points_host(px, cam)


def _host_cameras(model, cfg, views, bare, kw, lens):
    """``calibrated_cameras`` of ``calibrate_views_host`` on the lifts of predict_tracks of the flattened tracks."""
    from uplift_upsample_3dhpe_amd import predict
    V, N = len(views), len(views[0])
    flat = [predict.undistort_points_host(t, bare[v]) if bare[v].has_distortion else t for v in range(V) for t in views[v]]
    valid = kw.get("valid")
    pinhole = [bare[v].without(distortion=True, extrinsics=True) for v in range(V) for _ in range(N)]
    front = {k: kw[k] for k in ("resolutions", "mask_stride", "repair_joints", "keypoints") if k in kw}
    ref = predict.predict_tracks(model, cfg, flat, camera=pinhole, valid=valid, smooth=None, rotations=None, **front)
    assert [int(p.shape[0]) for p in ref[0]] == lens * V
    if kw.get("keypoints") is not None:
        source, flags = predict.map_keypoints_host(kw["keypoints"], flat, valid)
    else:
        source, flags = flat, None
    R = sum(lens)
    kp = np.concatenate([np.asarray(s, np.float32) for s in source]).reshape(V, R, J17, 2)
    flags = None if flags is None else np.concatenate([np.asarray(f) != 0 for f in flags]).reshape(V, R, J17).astype(np.uint8)
    lifts = _host(torch.cat(ref[0], 0)).reshape(V, R, J17, 3)
    pose, terms = predict.calibrate_views_host(lifts, kp, bare, flags)
    return predict.calibrated_cameras(bare, pose), pose, terms


def _same_cameras(a, b):
    return len(a) == len(b) and all(x.intrinsics == y.intrinsics and np.array_equal(x.distortion, y.distortion) and
                                    np.array_equal(np.asarray(x.orientation).view(np.uint64), np.asarray(y.orientation).view(np.uint64)) and
                                    np.array_equal(np.asarray(x.translation).view(np.uint64), np.asarray(y.translation).view(np.uint64))
                                    for x, y in zip(a, b))


FORMS = ["plain", "triangulate", "finite_repair", "coco17", "align", "lens"]


@pytest.mark.parametrize("form", FORMS)
def test_predict_views_with_calibrate_equals_the_call_on_its_cameras(form):
    from uplift_upsample_3dhpe_amd import predict
    from tests.test_distortion_cpu import SETS
    cfg, arch, w, model = _model("h36m_81")
    true = VU.ring_cameras(3, 41, distortion={1: SETS[0]} if form == "lens" else None)
    bare = [c.without(extrinsics=True) for c in true]
    views = _views(true, 43)
    kw = dict(resolutions=(1024, 1024), mask_stride=MS)
    lens = LENS
    if form == "triangulate":
        kw.update(triangulate=True)
    if form == "finite_repair":
        views[1][0][10:14, 3] = np.nan                                    # lost joints, repaired for the model, not used by the stage
        views[2][1][20] = np.nan                                          # view 2 does not see person 1 at frame 20
        kw.update(valid="finite", repair_joints=3)
    if form == "coco17":
        kw.update(keypoints="coco17")
    if form == "align":
        # known offsets only crop: one length per view, three lengths (the frames then do not belong together, which no bit depends on)
        offsets = [0, -3, 5]
        views = [[t[:LENS[0]] for t in tracks] for tracks in views]
        views = [[t[max(0, -o):LENS[0] - max(0, o)] for t in tracks] for tracks, o in zip(views, offsets)]
        kw.update(align=offsets)
    got = predict.predict_views(model, cfg, views, bare, calibrate=True, **kw)
    cams, calibration = got[-2], got[-1]
    assert len(cams) == 3 and all(isinstance(c, predict.Camera) and c.has_extrinsics for c in cams)
    assert [s for s, _ in calibration] == [1, 1, 1] and calibration[0][1] == 0
    again = predict.predict_views(model, cfg, views, cams, **kw)
    assert len(got) == len(again) + 2
    for i, (g, r) in enumerate(zip(got[:-2], again)):
        if isinstance(g[0], torch.Tensor):
            assert len(g) == len(r) and all(_bits(a, _host(b)) for a, b in zip(g, r)), (form, i)
        else:
            assert g == r, (form, i)                                                                                  # offsets and first
    # the world of the call is camera 0's own space
    assert np.array_equal(cams[0].orientation, [1.0, 0.0, 0.0, 0.0]) and not np.asarray(cams[0].translation).any()
    if form == "align":
        views, _, first = predict.crop_views(views, offsets)
        assert got[-4] == offsets and got[-3] == first
        lens = [int(views[0][0].shape[0])] * 2
    want, pose, terms = _host_cameras(model, cfg, views, bare, kw, lens)
    assert _same_cameras(cams, want), form
    assert calibration == [(int(pose[v, 7]), int(terms[v])) for v in range(3)]
    print(f"{form}: terms {[t for _, t in calibration]}, positions {[np.round(np.asarray(c.translation), 3).tolist() for c in cams]}")
    if form == "plain":
        # camera 0 with extrinsics defines the world: the host composition once more, and the call on ITS cameras
        got0 = predict.predict_views(model, cfg, views, [true[0]] + bare[1:], calibrate=predict.CalibrateViews(min_terms=10), **kw)
        assert got0[-2][0] is true[0] and _same_cameras(got0[-2], predict.calibrated_cameras([true[0]] + bare[1:], pose))
        again0 = predict.predict_views(model, cfg, views, got0[-2], **kw)
        assert all(_bits(a, _host(b)) for g, r in zip(got0[:-2], again0) for a, b in zip(g, r))
        # one view calibrates nothing and returns camera 0 as the world
        one = predict.predict_views(model, cfg, views[:1], bare[:1], calibrate=True, **kw)
        assert one[-1] == [(1, 0)] and len(one[-2]) == 1 and one[-2][0].has_extrinsics
        same = predict.predict_views(model, cfg, views[:1], one[-2], **kw)
        assert all(_bits(a, _host(b)) for g, r in zip(one[:-2], same) for a, b in zip(g, r))


# ---- 5. the unchanged call -----------------------------------------------------------------------------------------------------------------
def test_predict_views_without_calibrate_returns_what_it_returned():
    from tests.test_views_gpu import LENS as LENS2, _composition, _views as _views2
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model("h36m_81")
    cams = VU.ring_cameras(2, 41)
    views = _views2(cams, 43)
    kw = dict(resolutions=(1024, 1024), mask_stride=MS, bones="track", rotations=True)
    without = predict.predict_views(model, cfg, views, cams, **kw)
    got = predict.predict_views(model, cfg, views, cams, calibrate=None, **kw)
    assert len(got) == len(without) == 5
    for name, g, r in zip(("poses", "roots", "root_state", "view_count", "rotations"), got, without):
        assert [int(t.shape[0]) for t in g] == LENS2 and _bits(torch.cat(g, 0), _host(torch.cat(r, 0))), name
    want, _, _ = _composition(model, cfg, views, cams, dict(resolutions=(1024, 1024), mask_stride=MS), False)        # the parent's composition
    plain = predict.predict_views(model, cfg, views, cams, calibrate=None, resolutions=(1024, 1024), mask_stride=MS)
    assert len(plain) == 4 and all(_same(torch.cat(g, 0), r) for g, r in zip(plain, want))


# ---- 6. a view that cannot be calibrated ---------------------------------------------------------------------------------------------------
def test_a_view_without_a_pose_is_a_value_error_that_names_it():
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model("h36m_81")
    true = VU.ring_cameras(3, 41)
    bare = [c.without(extrinsics=True) for c in true]
    views = _views(true, 43)
    views[2] = [np.full_like(t, np.nan) for t in views[2]]                # view 2 saw nobody
    with pytest.raises(ValueError, match="view 2 cannot be calibrated"):
        predict.predict_views(model, cfg, views, bare, calibrate=True, valid="finite", resolutions=(1024, 1024), mask_stride=MS)
    with pytest.raises(ValueError, match="view 1 cannot be calibrated"):
        predict.predict_views(model, cfg, _views(true, 43), bare, calibrate=predict.CalibrateViews(min_terms=141), resolutions=(1024, 1024), mask_stride=MS)
