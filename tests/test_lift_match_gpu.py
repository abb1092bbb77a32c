"""GPU: who is who without a world, on the device (include/uu3d.h, WHO IS WHO WITHOUT A WORLD; views.py).  The references are the rules in
numpy, predict.lift_pair_sums_host and predict.match_lifts_host (tests/test_lift_match_cpu.py pins them against the truth of seeded
scenes); every comparison is on the bits.
  1. the launch alone on random inputs: view_of [0, 1], [0, 0, 1, 2, 2] and [0, 0, 2, 2] (an empty middle view), T in {1, 70, 257, 600} (idle
     lanes, one turn of the loop, two and three), J 5 and 17, with and without flags, NaN and Inf keypoints, a track nobody sees; the
     inputs are unchanged afterwards
  2. predict.match_lifts equals predict.match_lifts_host on the shared-body scene, and a second call returns the same bits
  3. every guard of the C ABI returns its code and leaves the outputs alone
  4. predict_views(match=MatchLifts(...)) (h36m_81 at mask stride 4, seeded weights, 3 views, 2 persons of 60 frames, shuffled, view 2
     missing a person) equals, bit for bit, the host composition on predict_tracks of the flattened tracks: with calibrate=True, on
     cameras with extrinsics, and on those with triangulate=True.  Seeded weights do not produce lifts that are rotations of each other,
     so max_dist is large enough that every pair is allowed, and the partition is whatever the mirror gives."""
import ctypes as C

import numpy as np
import pytest

from tests import lift_match_util as LU
from tests import views_util as VU
from tests.test_distortion_gpu import _host, _same
from tests.tracks_util import _model

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
MS, J17, T60 = 4, 17, 60
LAYOUTS = {"two": ([0, 1], 2), "five": ([0, 0, 1, 2, 2], 3), "empty_middle": ([0, 0, 2, 2], 3)}
FRAMES = (1, 70, 257, 600)


def _bits(a, b):
    a, b = _host(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- 1. the launch alone -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", FRAMES)
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_the_launch_equals_the_mirror(layout, T):
    from uplift_upsample_3dhpe_amd import predict
    view_of, V = LAYOUTS[layout]
    view_of = np.asarray(view_of, np.int32)
    M = len(view_of)
    J = 17 if (sorted(LAYOUTS).index(layout) + FRAMES.index(T)) % 2 == 0 else 5
    m = VU.min_joints(J)
    for with_flags in (True, False):
        poses, kp, flags = LU.random_inputs(view_of, T, J, 100 * T + M, with_flags)
        dp, dk = torch.from_numpy(poses).cuda(), torch.from_numpy(kp).cuda()
        df = None if flags is None else torch.from_numpy(flags).cuda()
        want = predict.lift_pair_sums_host(poses, kp, view_of, flags, V, m)
        got = predict.lift_pair_sums(dp, dk, view_of, df, V, m)
        assert got[0].dtype == torch.float64 and got[1].dtype == torch.int32 and tuple(got[0].shape) == tuple(got[1].shape) == (M, M)
        assert _bits(got[0], want[0]) and _bits(got[1], want[1]), (layout, T, J, with_flags)
        assert _bits(dp, poses) and _bits(dk, kp) and (df is None or _bits(df, flags))                               # only read
        assert want[1][0, M - 1] > 0 or (M >= 3 and T >= 255) or T == 1                                               # terms beside the zeros
        if M >= 3 and T >= 255:
            assert not want[1][M - 1].any() and want[1][0, 2] > 0                                                     # a track nobody sees
    # a lift that is not finite: the pair has no terms, on the device as in the mirror
    poses[0, :, 1, 2] = np.nan
    want = predict.lift_pair_sums_host(poses, kp, view_of, None, V, m)
    got = predict.lift_pair_sums(torch.from_numpy(poses).cuda(), dk, view_of, None, V, m)
    assert _bits(got[0], want[0]) and _bits(got[1], want[1]) and not want[1][0].any()
    if (layout, T) == ("five", 257):
        print(f"{layout} T {T}: terms {want[1].tolist()}")
        with pytest.raises(ValueError):
            predict.lift_pair_sums(dp.cpu(), dk, view_of)                                                             # a host tensor
        with pytest.raises(ValueError):
            predict.lift_pair_sums(dp[:, :10].contiguous(), dk, view_of)
        with pytest.raises(ValueError):
            predict.lift_pair_sums(dp, dk, view_of[::-1].copy())
        with pytest.raises(ValueError):
            predict.lift_pair_sums(dp, dk, view_of, min_root_joints=1)


# ---- 2. the two launches -------------------------------------------------------------------------------------------------------------------
def test_match_lifts_equals_the_mirror_and_repeats_its_bits():
    from uplift_upsample_3dhpe_amd import predict
    s = LU.shared_body()
    dp, dk = torch.from_numpy(s["poses"].copy()).cuda(), torch.from_numpy(s["kp"].copy()).cuda()
    for params in (dict(max_dist=0.06), dict(), dict(max_dist=0.01), dict(max_dist=0.06, min_terms=130)):
        want = predict.match_lifts_host(s["poses"], s["kp"], s["view_of"], **params)
        got = predict.match_lifts(dp, dk, s["view_of"], **params)
        again = predict.match_lifts(dp, dk, s["view_of"], **params)
        assert len(got) == len(want) == 5
        assert all(_bits(g, w) for g, w in zip(got, want)), params
        assert all(_bits(a, _host(g)) for a, g in zip(again, got)), params
    person = _host(predict.match_lifts(dp, dk, s["view_of"], max_dist=0.06)[0])
    assert LU.same_partition(person, s["truth"])


# ---- 3. the guards -------------------------------------------------------------------------------------------------------------------------
def test_every_guard_returns_its_code_and_leaves_the_outputs_alone():
    from uplift_upsample_3dhpe_amd import _capi
    lib = _capi.load_library()
    M, T, J = 3, 10, 5
    poses = torch.zeros((M * T * J * 3 + 1,), dtype=torch.float32, device="cuda")
    kp = torch.zeros((M * T * J * 2 + 2,), dtype=torch.float32, device="cuda")
    sums = torch.full((M * M + 1,), -7.0, dtype=torch.float64, device="cuda")
    terms = torch.full((M * M + 1,), 9, dtype=torch.int32, device="cuda")
    p = (lambda t, o=0: C.c_void_p(t.data_ptr() + o))
    i32 = (lambda *v: (C.c_int32 * len(v))(*v))
    good = dict(poses=p(poses), kp=p(kp), flags=None, view_of=i32(0, 1, 1), tracks=M, frames=T, J=J, views=2, m=3, sums=p(sums), terms=p(terms))
    cases = [(dict(tracks=65), 2), (dict(J=65), 2), (dict(views=9), 2), (dict(tracks=0), 1), (dict(frames=0), 1), (dict(J=0), 1), (dict(m=1), 1),
             (dict(views=0), 1), (dict(frames=2 ** 31), 1), (dict(poses=None), 1), (dict(kp=None), 1), (dict(sums=None), 1), (dict(terms=None), 1),
             (dict(view_of=None), 1), (dict(view_of=i32(1, 0, 1)), 1), (dict(view_of=i32(0, 1, 2)), 1), (dict(view_of=i32(-1, 0, 1)), 1),
             (dict(poses=p(poses, 2)), 1), (dict(kp=p(kp, 4)), 1), (dict(sums=p(sums, 4)), 1), (dict(terms=p(terms, 2)), 1)]
    order = ("poses", "kp", "flags", "view_of", "tracks", "frames", "J", "views", "m", "sums", "terms")
    for change, code in cases:
        args = dict(good)
        args.update(change)
        assert lib.uu3d_lift_pair_sums(*[args[k] for k in order], None) == code, change
    torch.cuda.synchronize()
    assert (sums == -7.0).all() and (terms == 9).all()
    assert lib.uu3d_lift_pair_sums(*[good[k] for k in order], None) == 0
    torch.cuda.synchronize()
    assert not sums[:M * M].any() and terms[:M * M].tolist() == [0, T, T, T, 0, 0, T, 0, 0] and sums[M * M] == -7.0 and terms[M * M] == 9      # zero lifts


# ---- 4. predict_views(match=MatchLifts(...)) -----------------------------------------------------------------------------------------------
def _scene(seed):
    """3 ring cameras; two persons of 60 frames; view 1 holds them in the other order, view 2 only the first."""
    from tests.test_view_calibrate_gpu import _views
    true = VU.ring_cameras(3, 41)
    views = [[t[:T60] for t in tracks] for tracks in _views(true, seed)]
    return true, [views[0], views[1][::-1], views[2][:1]]


def _composition(model, cfg, views, cameras, kw, params, calibrate, triangulate):
    """What the call must return, from predict_tracks on the flat tracks and the rules in numpy -> (want, person, P, cams, calibration), or
    the view the calibration refuses."""
    from uplift_upsample_3dhpe_amd import predict
    V = len(views)
    counts = [len(v) for v in views]
    view_of = np.repeat(np.arange(V, dtype=np.int32), counts)
    M = len(view_of)
    flat = [t for tracks in views for t in tracks]
    pinhole = [cameras[v].without(distortion=True, extrinsics=True) for v in view_of]
    ref = predict.predict_tracks(model, cfg, flat, camera=pinhole, smooth=None, rotations=None, **kw)
    assert [int(p.shape[0]) for p in ref[0]] == [T60] * M
    lifts = _host(torch.cat(ref[0], 0))
    kp = np.concatenate(flat)
    person, n, table, sums, terms = predict.match_lifts_host(lifts.reshape(M, T60, J17, 3), kp.reshape(M, T60, J17, 2), view_of, None, V, **params)
    P = int(n[0])
    own, px, flags = predict.gather_view_tracks_host(table[:, :P], lifts, kp, None, T60)
    cams, calibration = list(cameras), None
    if calibrate:
        pose, shared = predict.calibrate_views_host(own, px, cameras, flags)
        lost = [v for v in range(V) if pose[v, 7] != 1.0]
        if lost:
            return lost[0]
        cams = predict.calibrated_cameras(cameras, pose)
        calibration = [(int(pose[v, 7]), int(shared[v])) for v in range(V)]
    world = np.stack([predict.camera_to_world_host(own[v], None, None, cams[v])[0] for v in range(V)])
    fused, count, sees = predict.fuse_views_host(world, px, flags)
    want = [fused, None, None, count]
    if triangulate:
        points, agreed = predict.triangulate_joints_host(px, cams, sees, flags)
        fused, joint_views = predict.place_joints_host(fused, points, agreed, int(cfg.ROOT_KEYTPOINT))
        want[0] = fused
        want.append(joint_views)
    roots64, solved = predict.solve_view_roots_host(fused, px, cams, flags)
    want[1], want[2] = predict.root_trajectory_host(roots64, solved, [T60] * P)
    starts = np.concatenate([[0], np.cumsum(counts)])
    return want, [[int(k) for k in person[starts[v]:starts[v + 1]]] for v in range(V)], P, cams, calibration


@pytest.mark.parametrize("form", ["calibrate", "extrinsics", "triangulate"])
def test_predict_views_with_match_lifts_equals_the_host_composition(form):
    from tests.test_view_calibrate_gpu import _same_cameras
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model("h36m_81")
    true, views = _scene(43)
    calibrate = form == "calibrate"
    cameras = [c.without(extrinsics=True) for c in true] if calibrate else true
    kw = dict(resolutions=(1024, 1024), mask_stride=MS)
    params = dict(max_dist=10.0, min_terms=50)
    extra = dict(calibrate=True) if calibrate else dict(triangulate=True) if form == "triangulate" else {}
    expect = _composition(model, cfg, views, cameras, kw, params, calibrate, form == "triangulate")
    if isinstance(expect, int):                                           # the host composition refuses a view: the call names the same one
        with pytest.raises(ValueError, match=f"view {expect} cannot be calibrated"):
            predict.predict_views(model, cfg, views, cameras, match=predict.MatchLifts(**params), **extra, **kw)
        print(f"{form}: view {expect} is refused on the host and on the device")
        return
    want, person, P, cams, calibration = expect
    got = predict.predict_views(model, cfg, views, cameras, match=predict.MatchLifts(**params), **extra, **kw)
    assert len(got) == len(want) + 1 + (2 if calibrate else 0)
    for i, (g, r) in enumerate(zip(got, want)):
        assert [int(t.shape[0]) for t in g] == [T60] * P and _same(torch.cat(g, 0), r), (form, i)
    assert got[len(want)] == person
    print(f"{form}: persons {person}, root states 0 / 1 / 2: {np.bincount(want[2], minlength=3).tolist()}, view counts "
          f"{np.bincount(want[3], minlength=4).tolist()}")
    if calibrate:
        assert _same_cameras(got[-2], cams) and got[-1] == calibration
        again = predict.predict_views(model, cfg, views, got[-2], match=predict.MatchLifts(**params), **kw)      # the call on ITS cameras
        assert all(_same(torch.cat(a, 0), torch.cat(b, 0)) for a, b in zip(again[:4], got[:4])) and again[4] == got[4]
    else:
        dev = [[torch.from_numpy(t).cuda() for t in v] for v in views]                                             # tensors on the device are taken as well
        again = predict.predict_views(model, cfg, dev, cameras, match=predict.MatchLifts(**params), **extra, **kw)
        assert again[-1] == person and all(_same(torch.cat(a, 0), torch.cat(b, 0)) for a, b in zip(again[:4], got[:4]))
