"""No GPU: the rule of WHERE RAYS MEET (include/uu3d.h; views.py) in its numpy mirrors, predict.triangulate_joints_host and
predict.place_joints_host, on the seeded scenes of tests/triangulate_util.py.  tests/test_triangulate_gpu.py holds the device to these
mirrors bit for bit, so what is pinned here is that the mirrors compute a triangulation at all, and that the scenes reach every branch:
  1. a 2-view, 1-joint case by hand against numpy.linalg.lstsq
  2. every scene with two or more distinct cameras has at least half of its (frame, joint) pairs triangulated, and every planted edge case
     takes its intended branch
  3. with lifts scaled by 1.1 the placed joints are closer to the truth than the same joints of the fused pose (synthetic: the mechanism)
  4. check_triangulate, the refusals of the mirrors and of the C ABI (every guard comes before any device call)
  5. triangulate=None reaches no new code"""
import ctypes as C

import numpy as np
import pytest

from tests import triangulate_util as TU
from tests import views_util as VU


def _bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. by hand ----------------------------------------------------------------------------------------------------------------------------
def test_two_views_one_joint_against_lstsq():
    """The two passes written as two least-squares problems for numpy.linalg.lstsq (an SVD, not normal equations and cofactors): rows
    n . X = n . t and m . X = m . t per view, unweighted, then every view's rows divided by its depth at the first solution.  The bound is
    float64 rounding: 2.2e-16 times the squared condition number of a two-camera system at 60 to 120 degrees (below 1e2, squared 1e4) times
    |X| + |t| (below 10 m) is 2e-11 m, taken with a factor of 50: 1e-9 m.  Measured: 2.2e-16 m without noise and 4.4e-16 m with 0.5 px of
    noise -- float64 rounding; without noise the point is 8.7e-8 m from the truth (the pixels are float32)."""
    from uplift_upsample_3dhpe_amd import predict
    cams = VU.ring_cameras(2, 5)
    rows = predict.view_rows(cams)
    truth = np.array([0.2, -0.1, 1.1])
    rng = np.random.default_rng(9)
    for noise in (0.0, TU.NOISE_PX):
        kp = np.stack([VU.project(truth, c)[0] for c in cams]) + rng.normal(0.0, noise, (2, 2))
        kp = kp.astype(np.float32).reshape(2, 1, 1, 2)
        X, count = predict.triangulate_joints_host(kp, cams, np.ones((2, 1), np.uint8))
        assert count.tolist() == [[2]]

        def system(q):
            A, b = [], []
            for v in range(2):
                fx, fy, cx, cy = rows[v, :4]
                r1, r2, r3, t = rows[v, 4:7], rows[v, 7:10], rows[v, 10:13], rows[v, 13:16]
                n = (r1 - (np.float64(kp[v, 0, 0, 0]) - cx) / fx * r3) * q[v]
                m = (r2 - (np.float64(kp[v, 0, 0, 1]) - cy) / fy * r3) * q[v]
                A += [n, m]
                b += [n @ t, m @ t]
            return np.linalg.lstsq(np.array(A), np.array(b), rcond=None)[0]

        first = system([1.0, 1.0])
        z = [rows[v, 10:13] @ (first - rows[v, 13:16]) for v in range(2)]
        want = system([1.0 / z[0], 1.0 / z[1]])
        gap = float(np.abs(X[0, 0] - want).max())
        print(f"noise {noise} px: the mirror against lstsq {gap:.2e} m, against the truth {float(np.abs(X[0, 0] - truth).max()):.2e} m")
        assert gap <= 1e-9
        if noise == 0.0:
            assert np.abs(X[0, 0] - truth).max() <= 1e-4                  # (float32 pixels: 1e-5 px at 4 m)


# ---- 2. the scenes do not pass on nothing --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in TU.SHAPES if c[2] >= 2], ids=lambda c: "-".join(str(int(x)) for x in c))
def test_at_least_half_is_triangulated_and_every_edge_case_takes_its_branch(case):
    R, J, V = case
    s, fused, sees, X, count, placed, joint_views = TU.host_rules(R, J, V)
    share = float((count > 0).mean())
    print(f"{case}: triangulated {share:.3f}, counts {np.bincount(count.ravel(), minlength=V + 1).tolist()}")
    assert share >= 0.5
    assert count.max() <= V and not X[count == 0].any()
    if not s["edges"]:
        return
    at = TU.AT
    # views 0 and 1 alone, distinct cameras: triangulated by the two (the twin scenes below refuse the same candidates)
    assert count[TU.TWIN, at] == 2
    # every line meets in a point behind camera 0
    behind = s["truth"][TU.BEHIND, at] + 1.5 * (np.asarray(s["cams"][0].translation) - s["truth"][TU.BEHIND, at])
    assert VU.project(behind, s["cams"][0])[1] < 0 and count[TU.BEHIND, at] == 0
    # three candidates, one 40 px off: it is dropped, the two honest views place the joint (0.5 px at 4.5 m and f = 1145 px is 2 mm)
    if V >= 3:
        assert count[TU.OUTLIER3, at] == 2 and np.abs(X[TU.OUTLIER3, at] - s["truth"][TU.OUTLIER3, at]).max() < 0.02
    # two candidates, one 40 px off: rejected -- and placed by the two without the outlier (the same scene, the pixel put back)
    assert count[TU.OUTLIER2, at] == 0
    from uplift_upsample_3dhpe_amd import predict
    kp = s["kp"].copy()
    kp[1, TU.OUTLIER2, at, 1] -= TU.OUTLIER_PX
    assert predict.triangulate_joints_host(kp[:, TU.OUTLIER2:TU.OUTLIER2 + 1], s["cams"], sees[:, TU.OUTLIER2:TU.OUTLIER2 + 1],
                                           s["flags"][:, TU.OUTLIER2:TU.OUTLIER2 + 1])[1][0, at] == 2
    # one candidate; its fused lift is NaN and stays NaN
    assert count[TU.ONE, at] == 0 and joint_views[TU.ONE, at] == 0 and np.isnan(placed[TU.ONE, at, 1])
    assert np.array_equal(_bits32(placed[TU.ONE, at]), _bits32(fused[TU.ONE, at]))
    assert count[TU.ONE, TU.ROOT] > 0 and joint_views[TU.ONE, at + 1] > 0                    # (the rest of that frame is placed)
    # a view below min_root_joints does not SEE the frame and is no candidate
    assert not sees[0, TU.LOW] and sees[1:, TU.LOW].all() and count[TU.LOW].max() == (V - 1 if V >= 3 else 0)
    # the root joint is lost: joints are triangulated, none is placed, the frame keeps the fused bits
    assert count[TU.NO_ROOT, TU.ROOT] == 0 and count[TU.NO_ROOT].max() >= 2 and not joint_views[TU.NO_ROOT].any()
    assert np.array_equal(_bits32(placed[TU.NO_ROOT]), _bits32(fused[TU.NO_ROOT]))
    # placement everywhere: the root joint's zeros are +0.0, and a joint is placed iff it and its frame's root joint are triangulated
    take = (count > 0) & (count[:, TU.ROOT] > 0)[:, None]
    assert np.array_equal(joint_views, np.where(take, count, 0)) and not _bits32(placed[take[:, TU.ROOT], TU.ROOT]).any()
    assert np.array_equal(_bits32(placed[~take]), _bits32(fused[~take]))


@pytest.mark.parametrize("case", TU.TWINS, ids=lambda c: "-".join(str(int(x)) for x in c[:3]) + "-twin")
def test_twin_cameras_are_refused_by_the_rank_guard(case):
    R, J, V = case[:3]
    s, fused, sees, X, count, placed, joint_views = TU.host_rules(R, J, V, True)
    assert count[TU.TWIN, TU.AT] == 0                                    # views 0 and 1 alone: two rays that are one ray
    if V == 2:
        assert not count.any() and np.array_equal(_bits32(placed), _bits32(fused))           # nothing but twins: nothing is triangulated
    else:
        assert (count > 0).mean() >= 0.5                                 # a third camera gives the twins their distance


def test_one_view_is_taken_and_nothing_is_triangulated():
    s, fused, sees, X, count, placed, joint_views = TU.host_rules(70, 17, 1)
    assert not count.any() and not X.any() and not joint_views.any() and np.array_equal(_bits32(placed), _bits32(fused))


def test_min_views_and_max_residual_bind():
    R, J, V = 70, 17, 3
    loose = TU.host_rules(R, J, V)[4]
    three = TU.host_rules(R, J, V, False, True, 3, 8.0)[4]
    tight = TU.host_rules(R, J, V, False, True, 2, 0.25)[4]
    assert set(np.unique(three)) <= {0, 3} and (three == 3).any() and ((loose == 2) & (three == 0)).any()
    assert (tight > 0).sum() < (loose > 0).sum() and (tight > 0).any()   # 0.5 px of noise against a quarter of a pixel


# ---- 3. accuracy as mechanism --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(257, 17, 2), (257, 17, 3), (257, 17, 8)], ids=lambda c: "-".join(str(int(x)) for x in c))
def test_placed_joints_are_closer_to_the_truth_than_the_fused_lifts(case):
    """Synthetic: the mechanism, not an accuracy claim.  Lifts scaled by 1.1 with 1 cm of noise, 0.5 px of pixel noise; the mean distance
    of the placed joints (the root joint apart) from the true root-relative joints, beside that of the same joints in the fused pose.
    Measured: 2 views 3.75 mm beside 49.36 mm, 3 views 3.28 mm beside 49.60 mm, 8 views 1.94 mm beside 48.80 mm."""
    s, fused, sees, X, count, placed, joint_views = TU.host_rules(*case)
    rel = s["truth"] - s["truth"][:, TU.ROOT][:, None]
    which = joint_views > 0
    which[:, TU.ROOT] = False
    which &= np.isfinite(fused).all(axis=2)
    assert which.mean() >= 0.5
    err_placed = float(np.linalg.norm(placed[which].astype(np.float64) - rel[which], axis=1).mean())
    err_fused = float(np.linalg.norm(fused[which].astype(np.float64) - rel[which], axis=1).mean())
    print(f"{case}: {int(which.sum())} placed joints, mean error {1e3 * err_placed:.2f} mm placed, {1e3 * err_fused:.2f} mm fused")
    assert err_placed < err_fused


# ---- 4. parameters and refusals ------------------------------------------------------------------------------------------------------------
def test_check_triangulate():
    from uplift_upsample_3dhpe_amd import predict
    assert predict.check_triangulate(None) is None
    t = predict.check_triangulate(True)
    assert isinstance(t, predict.Triangulate) and (t.max_residual, t.min_views) == (8.0, 2) == tuple(predict.TRIANGULATE_DEFAULTS.values())
    given = predict.Triangulate(max_residual=0.25, min_views=3)
    assert predict.check_triangulate(given) is given and repr(given) == "Triangulate(max_residual=0.25, min_views=3)"
    for bad in (False, 1, 8.0, "yes", dict(max_residual=8.0), predict.MatchViews()):
        with pytest.raises(ValueError):
            predict.check_triangulate(bad)
    for kw in (dict(max_residual=0.0), dict(max_residual=-1.0), dict(max_residual=np.nan), dict(max_residual=np.inf), dict(max_residual="wide"),
               dict(max_residual=True), dict(min_views=1), dict(min_views=9), dict(min_views=2.0), dict(min_views=True)):
        with pytest.raises(ValueError):
            predict.Triangulate(**kw)


def test_refusals_of_the_mirrors():
    from uplift_upsample_3dhpe_amd import predict
    s, fused, sees, X, count, _, _ = TU.host_rules(70, 5, 2)
    kp, cams, flags = s["kp"], s["cams"], s["flags"]
    for args, kw in (((kp[0], cams, sees), {}), ((kp, cams[:1], sees), {}), ((kp, cams, sees[:1]), {}), ((kp, cams, sees, flags[:, :1]), {}),
                     ((kp, [c.without(extrinsics=True) for c in cams], sees), {}), ((kp, cams, sees), dict(min_views=1)),
                     ((kp, cams, sees), dict(max_residual=0.0)), ((np.zeros((9, 2, 5, 2), np.float32), cams, sees), {})):
        with pytest.raises(ValueError):
            predict.triangulate_joints_host(*args, **kw)
    for args in ((fused, X[:1], count, 0), (fused, X, count[:, :1], 0), (fused, X, count, 5), (fused, X, count, -1), (fused, X, count, True),
                 (fused[0], X, count, 0)):
        with pytest.raises(ValueError):
            predict.place_joints_host(*args)


def test_the_c_abi_declares_binds_and_guards_before_any_device_call():
    from uplift_upsample_3dhpe_amd import _capi
    from uplift_upsample_3dhpe_amd import synthetic as util
    lib = _capi.load_library()
    header = open(util.ROOT + "/include/uu3d.h").read()
    assert "WHERE RAYS MEET" in header
    for sym in ("uu3d_triangulate_joints", "uu3d_place_joints"):
        assert sym in _capi.EXPORTED_SYMBOLS and hasattr(lib, sym) and "int " + sym + "(" in header, sym
    # refusals of the shape and the parameters come first: no pointer is read, no device is touched
    good = dict(views=2, rows=10, J=5, min_views=2, max_residual=8.0)
    for change, code in ((dict(views=9), 2), (dict(J=65), 2), (dict(views=0), 1), (dict(J=0), 1), (dict(rows=-1), 1), (dict(min_views=1), 1),
                         (dict(min_views=9), 1), (dict(max_residual=0.0), 1), (dict(max_residual=-1.0), 1), (dict(max_residual=float("nan")), 1),
                         (dict(max_residual=float("inf")), 1), (dict(), 1)):                 # (the last: NULL pointers)
        a = dict(good)
        a.update(change)
        assert lib.uu3d_triangulate_joints(None, None, None, a["views"], a["rows"], a["J"], None, a["min_views"], a["max_residual"], None, None,
                                           None) == code, change
    assert lib.uu3d_triangulate_joints(None, None, None, 2, 0, 5, None, 2, 8.0, None, None, None) == 0                # no rows: nothing to do
    for (rows, J, root), code in (((10, 65, 0), 2), ((10, 0, 0), 1), ((10, 5, -1), 1), ((10, 5, 5), 1), ((-1, 5, 0), 1), ((10, 5, 0), 1), ((0, 5, 4), 0)):
        assert lib.uu3d_place_joints(None, None, None, rows, J, root, None, None, None) == code, (rows, J, root)
    assert C.sizeof(C.c_double) == 8


# ---- 5. triangulate=None reaches no new code -----------------------------------------------------------------------------------------------
def test_without_triangulate_the_stage_is_not_reached(monkeypatch):
    import inspect

    torch = pytest.importorskip("torch")
    from uplift_upsample_3dhpe_amd import views
    assert inspect.signature(views.predict_views).parameters["triangulate"].default is None
    R, J, V = 6, 5, 2
    calls = []

    def fuse(world, kp2d, flags, m):
        return torch.zeros(R, J, 3), torch.full((R,), V, dtype=torch.uint8), torch.ones(V, R, dtype=torch.uint8)

    def roots(fused, kp2d, cams, flags, m):
        calls.append(("roots", fused))
        return torch.zeros(R, 3, dtype=torch.float64), torch.ones(R, dtype=torch.bool)

    def triangulate(*a):
        calls.append(("triangulate",) + a[4:])
        return "X", "count"

    def place(fused, X, count, root):
        calls.append(("place", X, count, root))
        return fused + 1.0, torch.full((R, J), 2, dtype=torch.uint8)

    class Stages(object):
        @staticmethod
        def root_trajectory(r, ok, lens, _):
            return r.float(), ok.to(torch.uint8)

    class Person(object):
        min_root_joints, rigid, pose_filter, root_filter, rotations = 3, None, None, None, None

    monkeypatch.setattr(views, "fuse_views", fuse)
    monkeypatch.setattr(views, "solve_view_roots", roots)
    monkeypatch.setattr(views, "triangulate_joints", triangulate)
    monkeypatch.setattr(views, "place_joints", place)
    world = torch.zeros(V, R, J, 3)
    got = views._fused_scene(Stages, Person, world, torch.zeros(V, R, J, 2), None, None, np.array([2, 4]), None, 50, True)
    assert len(got) == 5 and [c[0] for c in calls] == ["roots"] and len(got[4]) == V         # today's tuple, and the per-view lifts
    del calls[:]
    got = views._fused_scene(Stages, Person, world, torch.zeros(V, R, J, 2), None, None, np.array([2, 4]), None, 50, True,
                             views.Triangulate(0.25, 3), 4)
    assert [c[0] for c in calls] == ["triangulate", "place", "roots"] and calls[0][1:] == (0.25, 3) and calls[1][1:] == ("X", "count", 4)
    assert len(got) == 6 and [tuple(t.shape) for t in got[4]] == [(2, J), (4, J)] and got[4][0].dtype == torch.uint8      # behind view_count
    assert bool((calls[2][1] == 1.0).all()) and bool((torch.cat(got[0]) == 1.0).all()) and len(got[5]) == V              # the root solve reads the hybrid pose
