"""CPU: where the cameras stand (include/uu3d.h, WHERE THE CAMERAS STAND; views.py) -- the numpy mirrors against the truth of the seeded
scenes of tests/view_calibrate_util.py, the Jacobi step against np.linalg.eigh, the host logic of predict_views(calibrate=...) and every
refusal, none of which touches a device.  The bounds next to "measured" are 16 times (exact scenes: platform differences in numpy's sums)
or 4 times (noisy scenes) the figure this file printed when it was written; the figures say what the mechanism does on synthetic scenes
and claim no accuracy on footage."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import view_calibrate_util as CU
from tests import views_util as VU

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- 1. the mirror against the truth -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CU.EXACT, ids=lambda c: "-".join(str(x) for x in c))
def test_exact_lifts_and_pixels_give_the_true_poses_to_rounding(case):
    s, pose, terms = CU.host_rules(*case)
    assert (pose[:, 7] == 1.0).all() and terms.tolist() == [0] + [s["R"]] * (s["V"] - 1)
    assert pose[0].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    dq = float(np.abs(pose[:, :4] - s["q"]).max())
    dc = float(np.abs(pose[:, 4:7] - s["c"]).max())
    print(f"exact {case}: max |q - q_true| {dq:.3e}, max |c - c_true| {dc:.3e} m at up to {np.linalg.norm(s['c'], axis=1).max():.2f} m")
    # measured (the inputs are float32: lifts to 3e-8 m, pixels to 6e-5 px): |dq| 1.5e-10 / 2.5e-10 / 4.7e-10, |dc| 3.4e-9 / 1.2e-8 / 1.9e-8 m
    assert dq <= 16 * 4.7e-10 and dc <= 16 * 1.9e-8
    assert np.abs(np.linalg.norm(pose[:, :4], axis=1) - 1.0).max() <= 4e-16 and (pose[:, 0] >= 0).all()


@pytest.mark.parametrize("case", CU.EXACT + [c[:3] for c in CU.NOISY[:1]], ids=lambda c: "-".join(str(x) for x in c))
def test_the_jacobi_step_against_eigh(case):
    from uplift_upsample_3dhpe_amd import predict, views
    noisy = len(case) == 3 and case in [c[:3] for c in CU.NOISY] and case not in CU.EXACT
    s = CU.host_rules(*case, 1.0, noisy)[0]
    sums = predict.view_moment_sums_host(s["poses"], s["kp"])
    ten, _ = predict.solve_view_pose_host(sums, None, 50)
    nine, _ = predict.solve_view_pose_host(sums, None, 50, sweeps=9)
    assert np.array_equal(ten, nine)                                      # CALIBRATE_SWEEPS = 10: nothing moves between 9 and 10 sweeps
    assert np.array_equal(ten, predict.solve_view_pose_host(sums, None, 50, sweeps=6)[0])      # ... nor between 6 and 10 on these scenes
    x = sums.sum(axis=1)
    worst_q, worst_l = 0.0, 0.0
    for v in range(1, s["V"]):
        N = views.horn_matrix(x[v, :9])
        assert np.array_equal(N, N.T)
        lam, E = np.linalg.eigh(N)
        e = E[:, -1] if E[0, -1] >= 0 else -E[:, -1]                      # up to sign
        worst_q = max(worst_q, float(np.abs(e - ten[v, :4]).max()))
        got_lam, got_E = views.jacobi_eigen4(N)
        worst_l = max(worst_l, float(np.abs(np.sort(got_lam) - lam).max() / np.abs(lam).max()))
        assert np.abs(got_E.T @ got_E - np.eye(4)).max() <= 1e-14
    print(f"jacobi {case}: max |q - q_eigh| {worst_q:.3e}, eigenvalues {worst_l:.3e} of the largest")
    # measured: |dq| 2.2e-16 / 2.2e-16 / 3.3e-16 / 6.4e-16, eigenvalues 3.1e-16 / 3.3e-16 / 5.1e-16 / 5.7e-16 of the largest
    assert worst_q <= 16 * 6.4e-16 and worst_l <= 16 * 5.7e-16


@pytest.mark.parametrize("case", CU.NOISY, ids=lambda c: "-".join(str(x) for x in c))
def test_scaled_lifts_scale_the_rig_and_noise_stays_small(case):
    V, persons, T, scale = case
    # exact lifts scaled by s: every camera stands s times as far away, the rotations are the true ones
    s, pose, _ = CU.host_rules(V, persons, T, scale, False)
    dq, dc = float(np.abs(pose[:, :4] - s["q"]).max()), float(np.abs(pose[:, 4:7] - scale * s["c"]).max())
    print(f"scaled {case}: max |q - q_true| {dq:.3e}, max |c - s c_true| {dc:.3e} m")
    # measured: |dq| 3.7e-10 / 1.8e-10 / 3.2e-10, |dc| 1.21e-8 / 1.44e-8 / 5.8e-9 m
    assert dq <= 16 * 3.7e-10 and dc <= 16 * 1.44e-8
    # 1 cm of noise on the lifts, 0.5 px on the pixels
    s, pose, terms = CU.host_rules(V, persons, T, scale, True)
    assert (pose[:, 7] == 1.0).all()
    ang = [CU.angle_deg(pose[v, :4], s["q"][v]) for v in range(1, V)]
    off = [float(np.linalg.norm(pose[v, 4:7] - scale * s["c"][v])) for v in range(1, V)]
    far = [float(np.linalg.norm(s["c"][v])) for v in range(1, V)]
    print(f"noisy {case}: rotation {np.round(ang, 4).tolist()} degrees, position {np.round(np.array(off) * 1e3, 2).tolist()} mm off s times "
          f"{np.round(far, 2).tolist()} m")
    # measured: 0.116 / 0.074, 0.105 / 0.067 and 0.100 / 0.056 degrees; 4.11 / 3.99, 4.09 / 3.98 and 4.57 / 4.36 mm at 5.8 to 7.6 m
    assert max(ang) <= 4 * 0.116 and max(off) <= 4 * 4.57e-3


def test_the_returned_cameras_reproduce_the_scene():
    from uplift_upsample_3dhpe_amd import predict
    s, pose, _ = CU.host_rules(3, 2, 129)
    cams = predict.calibrated_cameras(s["bare"], pose)
    assert len(cams) == 3 and all(c.has_extrinsics for c in cams)
    # the scene in the space of camera 0: its lift is the fused pose there; with the true cameras the same pose in world axes
    fused0 = s["poses"][0]
    fused_w, _ = predict.camera_to_world_host(fused0, None, None, s["cams"][0])
    roots0, solved0 = predict.solve_view_roots_host(fused0, s["kp"], cams)
    roots_w, solved_w = predict.solve_view_roots_host(fused_w, s["kp"], s["cams"])
    assert solved0.all() and solved_w.all()
    d_root = float(np.abs(roots0 - predict.world_to_camera_host(roots_w, s["cams"][0])).max())
    truth0 = predict.world_to_camera_host(s["truth"], s["cams"][0])
    d_truth = float(np.abs(roots0 - truth0[:, CU.ROOT]).max())
    sees = predict.fuse_views_host(s["poses"], s["kp"])[2]
    X0, n0 = predict.triangulate_joints_host(s["kp"], cams, sees)
    Xw, nw = predict.triangulate_joints_host(s["kp"], s["cams"], sees)
    assert (n0 == 3).all() and (nw == 3).all()
    d_x = float(np.abs(X0 - predict.world_to_camera_host(Xw, s["cams"][0])).max())
    d_xt = float(np.abs(X0 - truth0).max())
    print(f"scene: roots {d_root:.3e} m from the true cameras' and {d_truth:.3e} m from the truth; joints {d_x:.3e} m and {d_xt:.3e} m")
    # measured: roots 9.8e-9 and 3.3e-8 m, joints 7.1e-9 and 1.4e-7 m (the lifts and pixels are float32)
    assert d_root <= 16 * 9.8e-9 and d_truth <= 16 * 3.3e-8 and d_x <= 16 * 7.1e-9 and d_xt <= 16 * 1.4e-7


# ---- 2. state 0 ----------------------------------------------------------------------------------------------------------------------------
def test_the_views_that_cannot_be_calibrated():
    from uplift_upsample_3dhpe_amd import predict
    s = CU.host_rules(3, 1, 257)[0]
    poses, kp = s["poses"].copy(), s["kp"].copy()
    # fewer than min_terms shared rows: view 1 sees 49 rows
    few = kp.copy()
    few[1, 49:] = np.nan
    pose, terms = predict.calibrate_views_host(poses, few, s["bare"])
    assert pose[:, 7].tolist() == [1.0, 0.0, 1.0] and terms.tolist() == [0, 49, 257] and pose[1].tolist() == [1.0, 0, 0, 0, 0, 0, 0, 0.0]
    assert predict.calibrate_views_host(poses, few, s["bare"], min_terms=49)[0][:, 7].tolist() == [1.0, 1.0, 1.0]
    # a view that is all NaN; cleared flags do the same
    lost = kp.copy()
    lost[2] = np.nan
    pose, terms = predict.calibrate_views_host(poses, lost, s["bare"])
    assert pose[:, 7].tolist() == [1.0, 1.0, 0.0] and terms.tolist() == [0, 257, 0]
    flags = np.ones(kp.shape[:3], np.uint8)
    flags[2] = 0
    again = predict.calibrate_views_host(poses, kp, s["bare"], flags)
    assert np.array_equal(again[0], pose) and np.array_equal(again[1], terms)
    # view 0 lost: nobody has a term
    lost = kp.copy()
    lost[0] = np.nan
    assert predict.calibrate_views_host(poses, lost, s["bare"])[0][:, 7].tolist() == [1.0, 0.0, 0.0]
    # all used joints of view 1 on one pixel: the rotation comes from the lifts, but every ray of the view is one ray and no position follows
    one = kp.copy()
    one[1] = one[1, 0, 3]
    pose, terms = predict.calibrate_views_host(poses, one, s["bare"])
    assert pose[:, 7].tolist() == [1.0, 0.0, 1.0] and terms[1] == 257 and not pose[1, 4:7].any()
    assert np.array_equal(pose[1, :4], CU.host_rules(3, 1, 257)[1][1, :4])      # the quaternion stays
    # lifts that are all zeros: the eigenvalues are all zero, and their gap fails
    flat = poses.copy()
    flat[1] = 0.0
    pose, _ = predict.calibrate_views_host(flat, kp, s["bare"])
    assert pose[:, 7].tolist() == [1.0, 0.0, 1.0]
    # NaN lifts are not finite sums
    bad = poses.copy()
    bad[2, 100, 5, 1] = np.nan
    assert predict.calibrate_views_host(bad, kp, s["bare"])[0][:, 7].tolist() == [1.0, 1.0, 0.0]
    # one view calibrates nothing
    pose, terms = predict.calibrate_views_host(poses[:1], kp[:1], s["bare"][:1])
    assert pose.tolist() == [[1.0, 0, 0, 0, 0, 0, 0, 1.0]] and terms.tolist() == [0]


# ---- 3. the host logic ---------------------------------------------------------------------------------------------------------------------
def test_camera_0_with_extrinsics_composes():
    from uplift_upsample_3dhpe_amd import predict
    s, pose, _ = CU.host_rules(3, 2, 129)
    own = predict.calibrated_cameras(s["bare"], pose)                     # the world is camera 0's space
    assert np.array_equal(own[0].orientation, [1.0, 0.0, 0.0, 0.0]) and not own[0].translation.any() and own[0].intrinsics == s["bare"][0].intrinsics
    placed = predict.calibrated_cameras([s["cams"][0]] + s["bare"][1:], pose)
    assert placed[0] is s["cams"][0]
    rng = np.random.default_rng(5)
    points = rng.normal(0.0, 2.0, (64, 3)).astype(np.float32)
    state = np.ones(64, np.uint8)
    worst = 0.0
    for v in (1, 2):
        _, in0 = predict.camera_to_world_host(None, points, state, own[v])                  # to the space of camera 0 ...
        _, two_steps = predict.camera_to_world_host(None, in0, state, s["cams"][0])         # ... and from there to the world
        _, one_step = predict.camera_to_world_host(None, points, state, placed[v])
        worst = max(worst, float(np.abs(two_steps.astype(np.float64) - one_step).max()))
        # ... which is where the true camera puts them, to the error of the calibration (2e-8 rad, 2e-8 m) and of float32 at 10 m
        _, true = predict.camera_to_world_host(None, points, state, s["cams"][v])
        assert np.abs(one_step.astype(np.float64) - true).max() <= 4e-6
        assert np.abs(np.linalg.norm(placed[v].orientation) - 1.0) <= 4e-16
    print(f"composition: {worst:.3e} m between one step and two")
    # float32 is spaced 9.5e-7 at 8 to 16 m: the intermediate rounding of the two-step path and the two final roundings stay below 4 of them
    assert worst <= 4 * 9.5e-7
    # distortion and tol travel with the camera
    bent = [predict.Camera(*VU.FX, distortion=(0.1, 0.0, 0.0, 0.0, 0.0), tol=1e-4)] + s["bare"][1:]
    out = predict.calibrated_cameras(bent, pose)
    assert out[0].has_distortion and out[0].tol == 1e-4 and out[0].has_extrinsics and not out[1].has_distortion
    with pytest.raises(ValueError):
        predict.calibrated_cameras(s["bare"], pose[:2])
    with pytest.raises(ValueError, match="camera 2 comes with extrinsics"):
        predict.calibrated_cameras(s["bare"][:2] + [s["cams"][2]], pose)


def test_the_parameters_and_the_constants():
    from uplift_upsample_3dhpe_amd import _capi, predict, views
    assert predict.VIEW_CALIBRATE_DEFAULTS == dict(min_terms=50) and predict.check_calibrate(None) is None
    assert predict.check_calibrate(True).min_terms == 50 and predict.CalibrateViews(min_terms=7).min_terms == 7
    keep = predict.CalibrateViews(3)
    assert predict.check_calibrate(keep) is keep and repr(keep) == "CalibrateViews(min_terms=3)"
    for bad in (0, -1, 1.5, "50", True, None, 2 ** 31):
        with pytest.raises(ValueError):
            predict.CalibrateViews(min_terms=bad)
    for bad in (False, 1, "yes", dict(min_terms=5)):
        with pytest.raises(ValueError):
            predict.check_calibrate(bad)
    text = open(os.path.join(HERE, "..", "uplift-upsample-3dhpe_amd", "csrc", "uu3d_view_calibrate.h")).read()
    for name, value in (("kCalibrateChunk", views.CALIBRATE_CHUNK), ("kCalibrateLanes", views.MATCH_LANES), ("kCalibrateSums", views.CALIBRATE_SUMS),
                        ("kCalibrateSweeps", views.CALIBRATE_SWEEPS), ("kCalibratePose", views.CALIBRATE_POSE)):
        assert int(re.search(name + r"\s*=\s*(\d+)", text).group(1)) == value, name
    assert re.search(r"kCalibrateGap\s*=\s*0x1p-20", text) and views.CALIBRATE_GAP == 2.0 ** -20
    assert [views.calibrate_chunks(n) for n in (1, 4096, 4097, 8193)] == [1, 1, 2, 3]
    header = open(os.path.join(HERE, "..", "include", "uu3d.h")).read()
    assert "WHERE THE CAMERAS STAND" in header
    lib = _capi.load_library()
    for s in ("uu3d_view_calibrate_chunks", "uu3d_view_moment_sums", "uu3d_view_position_sums", "uu3d_solve_view_pose"):
        assert s in _capi.EXPORTED_SYMBOLS and hasattr(lib, s) and re.search(r"\b" + s + r"\s*\(", header)
    for name in ("calibrate_views", "calibrate_views_host", "view_moment_sums", "view_moment_sums_host", "view_position_sums",
                 "view_position_sums_host", "solve_view_pose", "solve_view_pose_host", "CalibrateViews", "VIEW_CALIBRATE_DEFAULTS",
                 "calibrated_cameras"):
        assert getattr(predict, name) is getattr(views, name), name


def test_the_mirrors_refuse_wrong_shapes():
    from uplift_upsample_3dhpe_amd import predict
    s = CU.host_rules(2, 1, 257)[0]
    poses, kp = s["poses"], s["kp"]
    with pytest.raises(ValueError):
        predict.view_moment_sums_host(poses[:, :10], kp)
    with pytest.raises(ValueError):
        predict.view_moment_sums_host(poses, kp, np.ones((2, 257, 16), np.uint8))
    with pytest.raises(ValueError):
        predict.view_moment_sums_host(poses, kp, min_root_joints=1)
    with pytest.raises(ValueError):
        predict.view_position_sums_host(poses, kp, s["bare"][:1], np.zeros((2, 8)))
    with pytest.raises(ValueError):
        predict.view_position_sums_host(poses, kp, s["bare"], np.zeros((2, 7)))
    with pytest.raises(ValueError):
        predict.view_position_sums_host(poses, kp, [VU.FX, VU.FX], np.zeros((2, 8)))
    with pytest.raises(ValueError):
        predict.solve_view_pose_host(np.zeros((2, 1, 9)))
    with pytest.raises(ValueError):
        predict.solve_view_pose_host(np.zeros((2, 1, 10)), np.zeros((3, 8)))
    with pytest.raises(ValueError):
        predict.solve_view_pose_host(np.zeros((2, 1, 10)), min_terms=0)
    # the intrinsics may come as rows
    rows = np.array([c.intrinsics for c in s["bare"]], np.float64)
    a = predict.calibrate_views_host(poses, kp, rows)
    b = predict.calibrate_views_host(poses, kp, s["bare"])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 4. the refusals of predict_views(calibrate=...), none of which touches a device ------------------------------------------------------
def test_every_refusal_fires_without_a_device():
    from uplift_upsample_3dhpe_amd import predict
    true = VU.ring_cameras(3, 41)
    bare = [c.without(extrinsics=True) for c in true]
    views = [[np.zeros((60, 17, 2), np.float32), np.zeros((80, 17, 2), np.float32)] for _ in range(3)]
    call = (lambda cams=bare, v=views, **kw: predict.predict_views(None, None, v, cams, calibrate=kw.pop("calibrate", True), **kw))
    with pytest.raises(ValueError, match="camera 1 comes with extrinsics"):
        call([bare[0], true[1], bare[2]])
    with pytest.raises(ValueError, match="camera 2 comes with extrinsics"):
        call([true[0], bare[1], true[2]])
    with pytest.raises(ValueError, match="list of Camera objects"):
        call([VU.FX] * 3)
    with pytest.raises(ValueError, match="list of Camera objects"):
        call([bare[0], VU.FX, bare[2]])
    with pytest.raises(ValueError, match="one Camera per view"):
        call(bare[:2])
    with pytest.raises(ValueError, match="does not take match"):
        call(match=True)
    with pytest.raises(ValueError, match="does not take match"):
        call(match=predict.MatchViews())
    with pytest.raises(ValueError, match="does not take align=True"):
        call(align=True)
    with pytest.raises(ValueError, match="does not take align=True"):
        call(align=predict.AlignViews(max_lag=5))
    with pytest.raises(ValueError, match="calibrate must be None, True or a CalibrateViews"):
        call(calibrate=1)
    with pytest.raises(ValueError, match="calibrate must be None, True or a CalibrateViews"):
        call(calibrate=False)
    # keyframes_only and out_fps stay refused, in today's words, on the plain route and with known offsets
    one_length = [[t[:60] for t in tracks] for tracks in views]
    for kw, v in ((dict(), views), (dict(align=[0, -3, 5]), one_length)):
        with pytest.raises(ValueError, match="predict_views does not take keyframes_only: the fusion needs one returned frame per given frame"):
            call(v=v, keyframes_only=True, **kw)
        with pytest.raises(ValueError, match="predict_views does not take out_fps: the fusion needs one returned frame per given frame"):
            call(v=v, out_fps=25, **kw)
    # what the call refused about the views, it still refuses
    with pytest.raises(ValueError, match="every view must hold the same persons"):
        call(v=[views[0], views[1][:1], views[2]])
    with pytest.raises(ValueError, match="same number of frames"):
        call(v=[views[0], views[1][::-1], views[2]])
    with pytest.raises(ValueError, match="one offset per view"):
        call(v=one_length, align=[0, 1])
    with pytest.raises(ValueError, match="triangulate must be"):
        call(triangulate=1)


def test_without_calibrate_the_arguments_are_handled_as_before():
    from uplift_upsample_3dhpe_amd import predict
    sig = inspect.signature(predict.predict_views)
    assert list(sig.parameters)[-1] == "calibrate" and sig.parameters["calibrate"].default is None
    assert list(sig.parameters)[-4:-1] == ["match", "align", "triangulate"]
    true = VU.ring_cameras(2, 41)
    bare = [c.without(extrinsics=True) for c in true]
    views = [[np.zeros((30, 17, 2), np.float32)] for _ in range(2)]
    for kw in (dict(), dict(calibrate=None)):
        with pytest.raises(ValueError, match="every view's Camera needs extrinsics"):
            predict.predict_views(None, None, views, bare, **kw)
        with pytest.raises(ValueError, match="every view's Camera needs extrinsics"):
            predict.predict_views(None, None, views, [true[0], bare[1]], **kw)
        with pytest.raises(ValueError, match="predict_views does not take keyframes_only"):
            predict.predict_views(None, None, views, true, keyframes_only=True, **kw)
        with pytest.raises(ValueError, match="every view's Camera needs extrinsics"):
            predict.predict_views(None, None, views, bare, align=[0, 1], **kw)
        with pytest.raises(ValueError, match="every view's Camera needs extrinsics"):
            predict.predict_views(None, None, views, bare, match=True, **kw)
    with pytest.raises(ValueError, match="every view's Camera needs extrinsics"):
        predict.check_view_cameras(bare)
