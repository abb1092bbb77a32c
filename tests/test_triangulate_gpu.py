"""GPU: joints placed where rays meet, on the device (include/uu3d.h, WHERE RAYS MEET; views.py).  The references are the rules in numpy,
predict.triangulate_joints_host and predict.place_joints_host (tests/test_triangulate_cpu.py pins them, and that the scenes leave at least
half of all joints triangulated and reach every branch); every comparison is on the bits.
  1. predict.triangulate_joints and predict.place_joints equal the mirrors on the seeded scenes of tests/triangulate_util.py: R in {1, 70,
     257} (one lane, more than one wave, across a 256-lane block edge), J in {5, 17}, V in {1, 2, 3, 8}, twin cameras, with and without
     flags, min_views 2 and 3, max_residual 0.25 and 8; the inputs are unchanged afterwards and the root joint's zeros are +0.0
  2. every guard of the C ABI returns its code and leaves the outputs alone
  3. predict_views(triangulate=True) (h36m_81 at mask stride 4, seeded weights, 2 persons of 23 and 40 frames, 2 views) equals the host
     composition of tests/test_views_gpu.py with the two mirrors behind fuse_views_host: plain, every option at once, and -- on the two
     persons' first 23 frames, since these routes take one length per view -- match=True on shuffled tracks and align=[0, -3]
  4. predict_views(triangulate=None) returns the bits of the call without the keyword"""
import ctypes as C

import numpy as np
import pytest

from tests import triangulate_util as TU
from tests import views_util as VU
from tests.test_distortion_gpu import _host, _same
from tests.tracks_util import _model

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
MS, J17 = 4, 17


def _bits(a, b):
    a, b = _host(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- 1. the launches alone -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TU.SHAPES + TU.TWINS, ids=lambda c: "-".join(str(int(x)) for x in c))
def test_the_launches_equal_the_mirrors(case):
    from uplift_upsample_3dhpe_amd import predict
    R, J, V = case[:3]
    twin = len(case) == 4
    s = TU.host_rules(R, J, V, twin)[0]
    dk, df, dp = (torch.from_numpy(s[k].copy()).cuda() for k in ("kp", "flags", "poses"))
    before = dk.clone(), df.clone()
    for with_flags in (True, False):
        flags = df if with_flags else None
        dev_fused, _, dev_sees = predict.fuse_views(dp, dk, flags, VU.min_joints(J))
        kept = dev_fused.clone(), dev_sees.clone()
        for min_views in (2, 3):
            for max_residual in (0.25, 8.0):
                _, fused, sees, X, count, placed, joint_views = TU.host_rules(R, J, V, twin, with_flags, min_views, max_residual)
                assert _same(dev_fused, fused) and _same(dev_sees, sees)
                got_x, got_n = predict.triangulate_joints(dk, s["cams"], dev_sees, flags, max_residual, min_views)
                assert got_x.dtype == torch.float64 and got_n.dtype == torch.uint8 and tuple(got_x.shape) == (R, J, 3) and tuple(got_n.shape) == (R, J)
                assert np.array_equal(_host(got_n), count), (with_flags, min_views, max_residual)
                assert np.array_equal(_host(got_x).view(np.uint64), X.view(np.uint64)), (with_flags, min_views, max_residual)      # float64, bit for bit
                got_p, got_v = predict.place_joints(dev_fused, got_x, got_n, TU.ROOT)
                assert got_p.dtype == torch.float32 and got_v.dtype == torch.uint8
                assert np.array_equal(_host(got_v), joint_views)
                assert np.array_equal(_host(got_p).view(np.uint32), placed.view(np.uint32)), (with_flags, min_views, max_residual)  # NaN bits included
                on = joint_views[:, TU.ROOT] > 0
                assert not _host(got_p)[on, TU.ROOT].view(np.uint32).any()                                                       # the root joint: +0.0
                if with_flags and min_views == 2 and max_residual == 8.0:
                    print(f"{case}: counts {np.bincount(count.ravel(), minlength=V + 1).tolist()}, placed {int((joint_views > 0).sum())} of {R * J}")
        assert _same(dev_fused, _host(kept[0])) and _same(dev_sees, _host(kept[1]))                                              # only read
    assert _same(dk, _host(before[0])) and _same(df, _host(before[1]))
    if case == (70, 17, 2):
        _, fused, sees, X, count, _, _ = TU.host_rules(R, J, V)
        dx, dn, ds = (torch.from_numpy(a.copy()).cuda() for a in (X, count, sees))
        root4 = predict.place_joints(dev_fused, dx, dn, 4)                                                                       # another root joint
        want = predict.place_joints_host(_host(dev_fused), X, count, 4)
        assert _bits(root4[0], want[0]) and _bits(root4[1], want[1])
        assert _bits(predict.triangulate_joints(dk, s["cams"], ds.bool(), df.bool())[0], X)                                      # bool is taken as well
        with pytest.raises(ValueError):
            predict.triangulate_joints(dk.cpu(), s["cams"], ds, df)                                             # a host tensor
        with pytest.raises(ValueError):
            predict.triangulate_joints(dk, s["cams"], ds[:1], df)
        with pytest.raises(ValueError):
            predict.triangulate_joints(dk, s["cams"][:1], ds, df)
        with pytest.raises(ValueError):
            predict.triangulate_joints(dk, s["cams"], ds, df, min_views=1)
        with pytest.raises(ValueError):
            predict.place_joints(dev_fused, dx.float(), dn, 0)
        with pytest.raises(ValueError):
            predict.place_joints(dev_fused, dx, dn, J)


# ---- 2. the guards -------------------------------------------------------------------------------------------------------------------------
def test_every_guard_returns_its_code_and_leaves_the_outputs_alone():
    from uplift_upsample_3dhpe_amd import _capi
    lib = _capi.load_library()
    V, R, J = 2, 10, 5
    kp = torch.zeros((V, R, J, 2), dtype=torch.float32, device="cuda")
    sees = torch.ones((V, R), dtype=torch.uint8, device="cuda")
    cams = torch.zeros((V, 16), dtype=torch.float64, device="cuda")
    X = torch.full((R * J * 3 + 1,), -7.0, dtype=torch.float64, device="cuda")
    count = torch.full((R, J), 9, dtype=torch.uint8, device="cuda")
    fused = torch.zeros((R * J * 3 + 1,), dtype=torch.float32, device="cuda")
    placed = torch.full((R * J * 3 + 1,), -7.0, dtype=torch.float32, device="cuda")
    jv = torch.full((R, J), 9, dtype=torch.uint8, device="cuda")
    p = (lambda t, o=0: C.c_void_p(t.data_ptr() + o))
    good = dict(kp=p(kp), flags=None, sees=p(sees), views=V, rows=R, J=J, cams=p(cams), min_views=2, max_residual=8.0, X=p(X), count=p(count))
    cases = [(dict(views=9), 2), (dict(J=65), 2), (dict(views=0), 1), (dict(J=0), 1), (dict(rows=-1), 1), (dict(min_views=1), 1), (dict(min_views=9), 1),
             (dict(max_residual=0.0), 1), (dict(max_residual=float("nan")), 1), (dict(max_residual=float("inf")), 1), (dict(kp=None), 1),
             (dict(sees=None), 1), (dict(cams=None), 1), (dict(X=None), 1), (dict(count=None), 1), (dict(kp=p(kp, 4)), 1), (dict(cams=p(cams, 4)), 1),
             (dict(X=p(X, 4)), 1)]
    order = ("kp", "flags", "sees", "views", "rows", "J", "cams", "min_views", "max_residual", "X", "count")
    for change, code in cases:
        args = dict(good)
        args.update(change)
        assert lib.uu3d_triangulate_joints(*[args[k] for k in order], None) == code, change
    good = dict(fused=p(fused), X=p(X), count=p(count), rows=R, J=J, root=0, placed=p(placed), jv=p(jv))
    cases = [(dict(J=65), 2), (dict(J=0), 1), (dict(rows=-1), 1), (dict(root=-1), 1), (dict(root=J), 1), (dict(fused=None), 1), (dict(X=None), 1),
             (dict(count=None), 1), (dict(placed=None), 1), (dict(jv=None), 1), (dict(placed=p(fused)), 1), (dict(fused=p(fused, 2)), 1),
             (dict(X=p(X, 4)), 1), (dict(placed=p(placed, 2)), 1)]
    order = ("fused", "X", "count", "rows", "J", "root", "placed", "jv")
    for change, code in cases:
        args = dict(good)
        args.update(change)
        assert lib.uu3d_place_joints(*[args[k] for k in order], None) == code, change
    torch.cuda.synchronize()
    assert (X == -7.0).all() and (count == 9).all() and (placed == -7.0).all() and (jv == 9).all()


# ---- 3. predict_views(triangulate=...) -----------------------------------------------------------------------------------------------------
def _hybrid_composition(model, cfg, views, cams, kw, full, params):
    """tests/test_views_gpu.py::_composition with the two mirrors behind fuse_views_host -> (want with joint_views behind view_count, the
    per-view lifts)."""
    from tests.test_views_gpu import LENS, _composition
    from uplift_upsample_3dhpe_amd import predict
    m = kw.get("min_root_joints", predict.DEFAULT_MIN_ROOT_JOINTS)
    base, world, sees = _composition(model, cfg, views, cams, {k: v for k, v in kw.items() if k != "bones"}, False)
    V, R = len(views), sum(LENS)
    valid = kw.get("valid")
    flat = [predict.undistort_points_host(t, cams[v]) if cams[v].has_distortion else t for v in range(V) for t in views[v]]
    flat_valid = valid if valid is None or isinstance(valid, str) else [f for per_view in valid for f in per_view]
    if kw.get("keypoints") is not None:
        source, flags = predict.map_keypoints_host(kw["keypoints"], flat, flat_valid)
    else:
        source, flags = flat, None if flat_valid is None or isinstance(flat_valid, str) else flat_valid
    kp = np.concatenate([np.asarray(t, np.float32) for t in source]).reshape(V, R, J17, 2)
    flags = None if flags is None else np.concatenate([np.asarray(f) != 0 for f in flags]).reshape(V, R, J17).astype(np.uint8)
    fused, count = base[0], base[3]
    X, agreed = predict.triangulate_joints_host(kp, cams, sees, flags, params.max_residual, params.min_views)
    hybrid, joint_views = predict.place_joints_host(fused, X, agreed, int(cfg.ROOT_KEYTPOINT))
    if kw.get("bones") is not None:
        hybrid = predict.fix_bones_host(hybrid, LENS, predict.bone_lengths_host(hybrid, LENS))
    roots64, solved = predict.solve_view_roots_host(hybrid, kp, cams, flags, m)
    roots, state = predict.root_trajectory_host(roots64, solved, LENS)
    want = [hybrid, roots, state, count, joint_views]
    if full:
        rate = kw.get("fps", 50)
        pose_filter, root_filter = predict.check_smooth(True, True)
        want[0] = predict.one_euro_host(hybrid, LENS, rate, pose_filter)
        want[1] = predict.one_euro_host(roots, LENS, rate, root_filter, state=state)
        want.append(predict.joint_rotations_host(want[0])[0])
    return want, world, fused


NAMES = ("poses", "roots", "root_state", "view_count", "joint_views", "rotations")


@pytest.mark.parametrize("form", ["plain", "all_options"])
def test_predict_views_with_triangulate_equals_the_host_composition(form):
    from tests.test_views_gpu import LENS, _views
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model("h36m_81")
    cams = VU.ring_cameras(2, 41)
    views = _views(cams, 43)
    kw = dict(resolutions=(1024, 1024), mask_stride=MS)
    full = form == "all_options"
    if full:
        rng = np.random.default_rng(47)
        valid = [[(rng.uniform(size=(n, J17)) > 0.06).astype(np.uint8) for n in LENS] for _ in cams]
        valid[0][0][5:9] = 0                                             # view 0 does not see person 0 at frames 5 .. 8
        valid[1][1][12, 3:] = 0                                          # view 1 keeps three joints of person 1 at frame 12: below min_root_joints
        views[0][0][6] = np.nan
        kw.update(fps=30, repair_joints=3, keypoints="coco17", bones="track", smooth=True, rotations=True, interpolation="cubic", valid=valid)
    params = predict.Triangulate()
    want, world, fused = _hybrid_composition(model, cfg, views, cams, kw, full, params)
    got = predict.predict_views(model, cfg, views, cams, return_views=True, triangulate=True, **kw)
    assert len(got) == len(want) + 1
    for name, g, r in zip(NAMES, got, want):
        assert [int(t.shape[0]) for t in g] == LENS and _same(torch.cat(g, 0), r), (form, name)
    assert got[4][0].dtype == torch.uint8 and tuple(got[4][1].shape) == (LENS[1], J17)
    assert len(got[-1]) == 2 and all(_same(torch.cat(got[-1][v], 0), world[v]) for v in range(2))                    # still the per-view lifts
    jv = want[4]
    print(f"{form}: joint_views 0 / 2: {np.bincount(jv.ravel(), minlength=3).tolist()}, root states {np.bincount(want[2], minlength=3).tolist()}")
    assert (jv == 2).mean() >= 0.5 and set(np.unique(jv)) <= {0, 2}                                                   # not compared on lifts alone
    if full:
        # frames one view alone saw stay lifted; the pelvis of keypoints="coco17" is the midpoint of two pixels, not the projection of a
        # point, and is 2 to 8 px off its rays: it is the root joint here, and placed within the default 8 px
        assert (jv == 0).any() and not jv[5:9].any() and (jv[:, int(cfg.ROOT_KEYTPOINT)] == 2).mean() >= 0.5
    else:
        assert (jv == 2).all() and not _bits(torch.cat(got[0], 0), fused)


def test_predict_views_with_triangulate_on_the_match_and_align_routes():
    from tests.test_views_gpu import LENS, _views
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model("h36m_81")
    cams = VU.ring_cameras(2, 41)
    kw = dict(resolutions=(1024, 1024), mask_stride=MS)
    # (match and align take tracks of one length per view: both persons' first 23 frames)
    T = LENS[0]
    # align=[0, -3]: view 1's frame f was taken at common time f - 3; the call is the call on the cropped views
    views = [[t[:T] for t in tracks] for tracks in _views(cams, 43)]
    cropped, _, first = predict.crop_views(views, [0, -3])
    assert first == [0, 3]
    lens = [T - 3, T - 3]
    want = predict.predict_views(model, cfg, cropped, cams, triangulate=True, **kw)
    got = predict.predict_views(model, cfg, views, cams, triangulate=True, align=[0, -3], **kw)
    assert len(got) == 7 and got[-2] == [0, -3] and got[-1] == first
    for name, g, r in zip(NAMES, got[:5], want):
        assert [int(t.shape[0]) for t in g] == lens and _same(torch.cat(g, 0), _host(torch.cat(r, 0))), ("align", name)
    # ... and the call on the cropped views is the host composition (frames that do not belong together: the residual decides)
    flat = [t for tracks in cropped for t in tracks]
    ref = predict.predict_tracks(model, cfg, flat, camera=[cams[v].without(extrinsics=True) for v in range(2) for _ in range(2)], **kw)
    R = sum(lens)
    world, _ = predict.camera_to_world_host(_host(torch.cat(ref[0], 0)), None, None, [cams[v] for v in range(2) for _ in range(2)], lens=lens * 2)
    kp = np.concatenate(flat).reshape(2, R, J17, 2)
    fused, count, sees = predict.fuse_views_host(world.reshape(2, R, J17, 3), kp)
    X, agreed = predict.triangulate_joints_host(kp, cams, sees)
    hybrid, joint_views = predict.place_joints_host(fused, X, agreed, int(cfg.ROOT_KEYTPOINT))
    roots64, solved = predict.solve_view_roots_host(hybrid, kp, cams)
    roots, state = predict.root_trajectory_host(roots64, solved, lens)
    for name, g, r in zip(NAMES, got[:5], (hybrid, roots, state, count, joint_views)):
        assert _same(torch.cat(g, 0), r), ("align", name)
    print(f"align: joint_views {np.bincount(joint_views.ravel(), minlength=3).tolist()}")
    # match=True on shuffled tracks of one length: view 1 lists its persons in the other order
    shuffled = [views[0], views[1][::-1]]
    got = predict.predict_views(model, cfg, shuffled, cams, triangulate=True, match=True, **kw)
    assert len(got) == 6 and got[-1] == [[0, 1], [1, 0]]
    person, n, table, _, _ = predict.match_views_host(shuffled, cams)
    flat = [t for tracks in shuffled for t in tracks]
    ref = predict.predict_tracks(model, cfg, flat, camera=[cams[v].without(extrinsics=True) for v in range(2) for _ in range(2)], **kw)
    world, _ = predict.camera_to_world_host(_host(torch.cat(ref[0], 0)), None, None, [cams[v] for v in range(2) for _ in range(2)], lens=[T] * 4)
    gw, gk, gf = predict.gather_view_tracks_host(table[:, :int(n[0])], world, np.concatenate(flat), None, T)
    fused, count, sees = predict.fuse_views_host(gw, gk, gf)
    X, agreed = predict.triangulate_joints_host(gk, cams, sees, gf)
    hybrid, joint_views = predict.place_joints_host(fused, X, agreed, int(cfg.ROOT_KEYTPOINT))
    roots64, solved = predict.solve_view_roots_host(hybrid, gk, cams, gf)
    roots, state = predict.root_trajectory_host(roots64, solved, [T, T])
    for name, g, r in zip(NAMES, got[:5], (hybrid, roots, state, count, joint_views)):
        assert [int(t.shape[0]) for t in g] == [T, T] and _same(torch.cat(g, 0), r), ("match", name)
    assert (joint_views == 2).mean() >= 0.5


# ---- 4. the unchanged call -----------------------------------------------------------------------------------------------------------------
def test_predict_views_without_triangulate_returns_what_it_returned():
    from tests.test_views_gpu import LENS, _composition, _views
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model("h36m_81")
    cams = VU.ring_cameras(2, 41)
    views = _views(cams, 43)
    kw = dict(resolutions=(1024, 1024), mask_stride=MS, bones="track", rotations=True)
    without = predict.predict_views(model, cfg, views, cams, **kw)
    got = predict.predict_views(model, cfg, views, cams, triangulate=None, **kw)
    assert len(got) == len(without) == 5
    for name, g, r in zip(("poses", "roots", "root_state", "view_count", "rotations"), got, without):
        assert [int(t.shape[0]) for t in g] == LENS and _bits(torch.cat(g, 0), _host(torch.cat(r, 0))), name
    want, _, _ = _composition(model, cfg, views, cams, dict(resolutions=(1024, 1024), mask_stride=MS), False)        # the parent's composition
    plain = predict.predict_views(model, cfg, views, cams, triangulate=None, resolutions=(1024, 1024), mask_stride=MS)
    assert len(plain) == 4 and all(_same(torch.cat(g, 0), r) for g, r in zip(plain, want))
