"""CPU: who is who without a world (include/uu3d.h, WHO IS WHO WITHOUT A WORLD; views.py) -- the numpy mirrors against the true partition
of the seeded scenes of tests/lift_match_util.py, the edges of the rule, the consistency with the ray rule of WHO IS WHO behind a
calibration, and every refusal of predict_views(match=MatchLifts(...)), none of which touches a device.  The figures say what the
mechanism does on synthetic scenes and claim no accuracy on footage."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import lift_match_util as LU
from tests import view_calibrate_util as CU
from tests import views_util as VU

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- 1. the mirror against the truth -----------------------------------------------------------------------------------------------------
def test_exact_lifts_give_the_true_partition():
    from uplift_upsample_3dhpe_amd import predict
    s = CU.scene(3, 2, 129)
    who = [[1, 0], [0, 1], [1, 0]]
    poses, kp, view_of, truth = LU.tracks_of(s["poses"], s["kp"], 2, 129, who)
    person, n, table, sums, terms = predict.match_lifts_host(poses, kp, view_of)
    assert n[0] == 2 and LU.same_partition(person, truth)
    assert person.tolist() == [0, 1, 1, 0, 0, 1] and table[:, :2].tolist() == [[0, 1], [3, 2], [4, 5]]
    mean = sums / np.maximum(terms, 1)
    same = (truth[:, None] == truth[None]) & (view_of[:, None] != view_of[None])
    other = (truth[:, None] != truth[None]) & (view_of[:, None] != view_of[None])
    assert (terms[same] == 129).all() and (terms[other] == 129).all()
    print(f"exact lifts: true pairs S / n up to {mean[same].max():.3e} m^2, wrong pairs from {mean[other].min():.3e} m^2")
    assert mean[same].max() < 1e-12                                       # the lifts are float32: (3e-8 m)^2
    assert np.sqrt(mean[other].min()) > predict.LIFT_MATCH_DEFAULTS["max_dist"]


def test_the_shared_body_scene_splits_in_the_right_order():
    from uplift_upsample_3dhpe_amd import predict
    s = LU.shared_body()
    params = predict.MatchLifts(max_dist=0.06)
    person, n, table, sums, terms = predict.match_lifts_host(s["poses"], s["kp"], s["view_of"], max_dist=params.max_dist, min_terms=params.min_terms)
    true, wrong = LU.pair_rms(sums, terms, s["truth"], s["view_of"])
    print(f"shared body: the largest true-pair rms {true:.4f} m, the smallest wrong-pair rms {wrong:.4f} m")
    assert true < params.max_dist < wrong                                 # only the ORDER: the README quotes the two figures
    assert n[0] == 3 and LU.same_partition(person, s["truth"])
    assert (table[2, :3] >= 0).sum() == 2                                 # view 2 does not hold one of the persons


# ---- 2. the two matchings agree ------------------------------------------------------------------------------------------------------------
def test_the_lift_rule_and_the_ray_rule_agree_behind_the_calibration():
    from uplift_upsample_3dhpe_amd import predict
    s = LU.shared_body()
    T, J, V = s["T"], s["J"], 3
    M = len(s["view_of"])
    person, n, table, _, _ = predict.match_lifts_host(s["poses"], s["kp"], s["view_of"], max_dist=0.06)
    P = int(n[0])
    own, px, flags = predict.gather_view_tracks_host(table[:, :P], s["poses"].reshape(M * T, J, 3), s["kp"].reshape(M * T, J, 2), None, T)
    pose, terms = predict.calibrate_views_host(own, px, s["bare"], flags)
    assert (pose[:, 7] == 1.0).all() and terms.tolist() == [0, 3 * T, 2 * T]      # a (view, person) pair without a track is rows nobody SEES
    ang = [CU.angle_deg(pose[v, :4], s["q"][v]) for v in range(1, V)]
    off = [float(np.linalg.norm(pose[v, 4:7] - s["scale"] * s["c"][v])) for v in range(1, V)]
    print(f"calibrated behind the match: rotation {np.round(ang, 4).tolist()} degrees, position {np.round(np.array(off) * 1e3, 2).tolist()} mm off")
    # the bound tests/test_view_calibrate_cpu.py records for its noisy scenes (the same noise: 1 cm on the lifts, 0.5 px), not a new one
    assert max(ang) <= 4 * 0.116 and max(off) <= 4 * 4.57e-3
    cams = predict.calibrated_cameras(s["bare"], pose)
    starts = np.concatenate([[0], np.cumsum([len(w) for w in s["who"]])])
    views = [[s["kp"][m] for m in range(starts[v], starts[v + 1])] for v in range(V)]
    by_rays = predict.match_views_host(views, cams)
    assert by_rays[1][0] == P and np.array_equal(by_rays[0], person) and np.array_equal(by_rays[2], table)


# ---- 3. the edges of the rule --------------------------------------------------------------------------------------------------------------
def test_the_edges_of_the_rule():
    from uplift_upsample_3dhpe_amd import predict
    view_of = np.array([0, 0, 1, 2, 2], np.int32)
    poses, kp, flags = LU.random_inputs(view_of, 300, 17, 5, True)       # nobody sees track 4
    sums, terms = predict.lift_pair_sums_host(poses, kp, view_of, flags)
    assert sums.dtype == np.float64 and terms.dtype == np.int32 and sums.shape == terms.shape == (5, 5)
    assert np.array_equal(sums, sums.T) and np.array_equal(terms, terms.T)
    for p, q in ((0, 0), (0, 1), (3, 4), (2, 2), (0, 4), (2, 4)):         # the diagonal, same-view pairs, a track nobody sees
        assert sums[p, q] == 0.0 and terms[p, q] == 0 and not np.signbit(sums[p, q]), (p, q)
    assert (terms[[0, 0, 1, 1, 2], [2, 3, 2, 3, 3]] > 0).all() and (sums >= 0.0).all()
    assert (terms <= 300).all()                                           # frames, not joints
    # S is never negative: a track against its own copy in another view has E = 2 top up to rounding
    twin = np.stack([poses[0], poses[0]])
    s2, n2 = predict.lift_pair_sums_host(twin, np.stack([kp[0], kp[0]]), [0, 1])
    assert n2[0, 1] > 0 and 0.0 <= s2[0, 1] / n2[0, 1] < 1e-12 and not np.signbit(s2[0, 1])
    # swapping p and q gives the same bits: the two tracks in the other order -- M becomes its transpose, Horn's matrix changes the sign of
    # its first row and column, and every Jacobi statement is symmetric under that
    a = predict.lift_pair_sums_host(poses[[0, 2]], kp[[0, 2]], [0, 1], flags[[0, 2]])
    b = predict.lift_pair_sums_host(poses[[2, 0]], kp[[2, 0]], [0, 1], flags[[2, 0]])
    assert a[0][0, 1] == sums[0, 2] and a[1][0, 1] == terms[0, 2]
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1])
    # T = 1
    s1, n1 = predict.lift_pair_sums_host(poses[[0, 2], :1], kp[[0, 2], :1], [0, 1], np.ones((2, 1, 17), np.uint8))
    seen = bool(np.isfinite(kp[[0, 2], 0]).all(axis=2).sum(axis=1).min() >= 6)
    assert n1[0, 1] == (1 if seen else 0) and s1[0, 1] >= 0.0
    # a lift that is not finite: zero terms and 0.0, whichever track holds it
    for bad in (np.nan, np.inf):
        broken = poses.copy()
        broken[2, 7, 3, 1] = bad
        s3, n3 = predict.lift_pair_sums_host(broken, kp, view_of)
        assert not n3[2].any() and not s3[2].any() and n3[0, 3] > 0
    # ... unless no pair sees the frame that holds it
    lost = kp.copy()
    lost[2, 7] = np.nan
    s4, n4 = predict.lift_pair_sums_host(broken, lost, view_of)
    assert n4[2, 0] > 0 and np.isfinite(s4).all()


@pytest.mark.parametrize("R", [1, 200, 256, 600])
def test_the_moment_sums_are_those_of_the_calibration(R):
    """With two tracks the nine moment sums equal ``view_moment_sums_host``'s for R <= 256: every lane then holds at most one row, and the
    order of summation is the tree alone.  Only then is the order the same by construction; it stays the same while one chunk of 4096 rows
    holds all of them (600 here), and beyond that WHERE THE CAMERAS STAND adds chunks, which this rule does not have."""
    from uplift_upsample_3dhpe_amd import predict
    poses, kp, flags, _ = CU.random_inputs(2, R, 17, 31 + R, True)
    _, terms, every = predict.lift_pair_sums_host(poses, kp, [0, 1], flags, totals=True)
    partial = predict.view_moment_sums_host(poses, kp, flags)
    assert partial.shape == (2, 1, 10)
    # track 0 is p and view 0: a[j][i] b[j][k] here is p_0[j][i] p_1[j][k], the transpose of the calibration's p_1 (x) p_0
    mine = every[0, 1, :9].reshape(3, 3)
    theirs = partial[1, 0, :9].reshape(3, 3).T
    assert np.array_equal(mine.view(np.uint64), theirs.view(np.uint64))
    assert every[0, 1, 10] == partial[1, 0, 9] == terms[0, 1]


# ---- 4. the parameters, the constants and the names ----------------------------------------------------------------------------------------
def test_the_parameters_and_the_constants():
    from uplift_upsample_3dhpe_amd import _capi, predict, views
    assert predict.LIFT_MATCH_DEFAULTS == dict(max_dist=0.1, min_terms=50)
    keep = predict.MatchLifts(max_dist=0.06, min_terms=7)
    assert predict.check_match(keep) is keep and repr(keep) == "MatchLifts(max_dist=0.06, min_terms=7)"
    assert predict.MatchLifts().max_dist == 0.1 and predict.MatchLifts().min_terms == 50
    assert isinstance(predict.check_match(True), predict.MatchViews) and predict.check_match(None) is None
    for bad in (dict(max_dist=-1.0), dict(max_dist=np.nan), dict(max_dist="far"), dict(min_terms=0), dict(min_terms=1.5), dict(min_terms=True)):
        with pytest.raises(ValueError):
            predict.MatchLifts(**bad)
    with pytest.raises(ValueError, match="match must be None, True or a MatchViews"):
        predict.check_match("lifts")
    text = open(os.path.join(HERE, "..", "uplift-upsample-3dhpe_amd", "csrc", "uu3d_lift_match.h")).read()
    assert int(re.search(r"kLiftPairSums\s*=\s*(\d+)", text).group(1)) == views.LIFT_PAIR_SUMS == 11
    assert "horn_jacobi(" in text and "lift_moment_products(" in text and "UU3D_JACOBI_ROT4" not in text      # the shared functions, no copy
    header = open(os.path.join(HERE, "..", "include", "uu3d.h")).read()
    assert header.index("WHERE THE CAMERAS STAND (") < header.index("WHO IS WHO WITHOUT A WORLD (") < header.index("ANY FRAME RATE (")
    lib = _capi.load_library()
    assert "uu3d_lift_pair_sums" in _capi.EXPORTED_SYMBOLS and hasattr(lib, "uu3d_lift_pair_sums") and re.search(r"\buu3d_lift_pair_sums\s*\(", header)
    for name in ("MatchLifts", "LIFT_MATCH_DEFAULTS", "lift_pair_sums", "lift_pair_sums_host", "match_lifts", "match_lifts_host"):
        assert getattr(predict, name) is getattr(views, name), name
    sig = inspect.signature(predict.predict_views)
    assert list(sig.parameters)[-4:] == ["match", "align", "triangulate", "calibrate"]


def test_the_mirror_refuses_wrong_shapes():
    from uplift_upsample_3dhpe_amd import predict
    poses, kp, flags = LU.random_inputs([0, 1], 20, 17, 3, True)
    with pytest.raises(ValueError):
        predict.lift_pair_sums_host(poses[:, :10], kp, [0, 1])
    with pytest.raises(ValueError):
        predict.lift_pair_sums_host(poses, kp, [0, 1], flags[:, :, :16])
    with pytest.raises(ValueError):
        predict.lift_pair_sums_host(poses, kp, [1, 0])
    with pytest.raises(ValueError):
        predict.lift_pair_sums_host(poses, kp, [0, 1, 1])
    with pytest.raises(ValueError):
        predict.lift_pair_sums_host(poses, kp, [0, 1], min_root_joints=1)
    with pytest.raises(ValueError):
        predict.lift_pair_sums_host(poses, kp, [0, 9])
    with pytest.raises(ValueError, match="at most 64 tracks"):
        predict.lift_pair_sums_host(np.zeros((65, 1, 17, 3), np.float32), np.zeros((65, 1, 17, 2), np.float32), np.zeros(65, np.int32))
    with pytest.raises(ValueError):
        predict.match_lifts_host(poses, kp, [0, 1], max_dist=-1.0)


# ---- 5. the refusals of predict_views(match=MatchLifts(...)), none of which touches a device ----------------------------------------------
def test_every_refusal_fires_without_a_device():
    from uplift_upsample_3dhpe_amd import predict
    true = VU.ring_cameras(3, 41)
    bare = [c.without(extrinsics=True) for c in true]
    track = np.zeros((60, 17, 2), np.float32)
    views = [[track, track], [track, track], [track]]
    lifts = predict.MatchLifts()
    call = (lambda cams=bare, v=views, **kw: predict.predict_views(None, None, v, cams, calibrate=kw.pop("calibrate", True),
                                                                   match=kw.pop("match", lifts), **kw))
    # match=True and a MatchViews with calibrate keep their words
    with pytest.raises(ValueError, match="does not take match: matching needs the rays in one world"):
        call(match=True)
    with pytest.raises(ValueError, match="does not take match: matching needs the rays in one world"):
        call(match=predict.MatchViews())
    # an estimating align, with and without calibrate
    for kw in (dict(), dict(calibrate=None, cams=true)):
        with pytest.raises(ValueError, match=r"match=MatchLifts\(\.\.\.\)\) does not take align=True or an AlignViews"):
            call(align=True, **kw)
        with pytest.raises(ValueError, match=r"match=MatchLifts\(\.\.\.\)\) does not take align=True or an AlignViews"):
            call(align=predict.AlignViews(max_lag=5), **kw)
    # an empty view 0 with calibrate: view 0 defines the world
    with pytest.raises(ValueError, match="view 0 holds no track, and view 0 defines the world"):
        call(v=[[], [track, track], [track]])
    # the per-person bones list, in the words of the matched route
    with pytest.raises(ValueError, match="does not take bones as a per-person list"):
        call(bones=[np.ones(17), np.ones(17)])
    with pytest.raises(ValueError, match="does not take bones as a per-person list"):
        call(bones=[np.ones(17), np.ones(17)], calibrate=None, cams=true)
    # more than 64 tracks
    with pytest.raises(ValueError, match="at most 64 tracks"):
        call(v=[[track] * 33, [track] * 32, []])
    # today's checks of the matched route
    with pytest.raises(ValueError, match="one common number of frames"):
        call(v=[[track, track[:50]], [track], [track]])
    with pytest.raises(ValueError, match="takes one fps for all tracks"):
        call(fps=[50.0, 25.0])
    with pytest.raises(ValueError, match="predict_views does not take keyframes_only"):
        call(keyframes_only=True)
    with pytest.raises(ValueError, match="predict_views does not take out_fps"):
        call(out_fps=25)
    with pytest.raises(ValueError, match="camera 1 comes with extrinsics"):
        call([bare[0], true[1], bare[2]])
    with pytest.raises(ValueError, match="every view's Camera needs extrinsics"):
        call(calibrate=None)                                              # without calibrate the cameras need a world
    with pytest.raises(ValueError, match="one offset per view"):
        call(align=[0, 1])
