"""Absolute root position, the rule in numpy (predict.solve_roots_host, predict.root_trajectory_host) and the host plan (rates.given_positions,
rates.root_plan): nothing here touches a device.
  1. the solve recovers a known translation from projections rounded to float32
  2. each condition that leaves a frame unsolved, one at a time
  3. the trajectory: held ends, weights against Fraction arithmetic, tracks without a solved frame, track boundaries, the positions of
     keyframes_only and of fps / out_fps
  4. argument checks"""
from fractions import Fraction

import numpy as np
import pytest

CAM = (1145.0, 1143.8, 512.5, 515.5)                                     # a Human3.6M-like camera, in pixels


def _skeleton(rng, G, J=17):
    """Seeded root-relative poses of about a person's size, joint 0 the root."""
    P = rng.uniform(-0.9, 0.9, size=(G, J, 3)).astype(np.float32)
    P[:, 0] = 0.0
    return P


def _project(P, T, cam):
    """Exact pinhole projection of P + T in float64, rounded to float32."""
    X = P.astype(np.float64) + np.asarray(T, np.float64)[:, None, :]
    return np.stack([cam[0] * X[..., 0] / X[..., 2] + cam[2], cam[1] * X[..., 1] / X[..., 2] + cam[3]], axis=-1).astype(np.float32)


def test_mirror_recovers_a_known_translation():
    """Max error <= 1e-4 m: 2.7e-6 m was measured when the rule was written (17 joints, depths 2 to 10 m, 2000 draws); the margin covers
    other seeds and cameras and is still four orders below a centimetre."""
    from uplift_upsample_3dhpe_amd import predict
    rng = np.random.default_rng(0)
    G = 2000
    P = _skeleton(rng, G)
    T = np.stack([rng.uniform(-2, 2, G), rng.uniform(-1, 1, G), rng.uniform(2, 10, G)], axis=1)
    uv = _project(P, T, CAM)
    used = rng.uniform(size=(G, 17)) < 0.7
    roots, solved = predict.solve_roots_host(P, uv, CAM, used)
    enough = used.sum(axis=1) >= 6
    assert enough.sum() > 1900 and np.array_equal(solved, enough)
    err = np.abs(roots[solved] - T[solved]).max()
    print(f"max |T - T_true| = {err:.3e} m")
    assert err <= 1e-4
    assert (roots[~solved] == 0).all() and roots.dtype == np.float64
    # one camera per track gives each track's frames its own
    cam2 = (800.0, 810.0, 320.0, 240.0)
    uv2 = np.concatenate([uv[:5], _project(P[5:9], T[5:9], cam2)])
    r2, s2 = predict.solve_roots_host(P[:9], uv2, [CAM, cam2], used[:9], lens=[5, 4])
    assert np.array_equal(s2, enough[:9]) and np.abs(r2[s2] - T[:9][s2]).max() <= 1e-4
    assert np.array_equal(r2[:5].view(np.uint64), roots[:5].view(np.uint64))


def _one_frame(seed=3):
    rng = np.random.default_rng(seed)
    P = _skeleton(rng, 1)
    T = np.array([[0.3, -0.2, 4.0]])
    return P, T, _project(P, T, CAM)


def test_unsolved_too_few_joints():
    from uplift_upsample_3dhpe_amd import predict
    P, T, uv = _one_frame()
    flags = np.zeros((1, 17), bool)
    flags[0, :6] = True
    roots, solved = predict.solve_roots_host(P, uv, CAM, flags)
    assert solved[0] and np.abs(roots - T).max() <= 1e-4
    flags[0, 5] = False                                                  # n = min_root_joints - 1
    roots, solved = predict.solve_roots_host(P, uv, CAM, flags)
    assert not solved[0] and (roots == 0).all()
    roots, solved = predict.solve_roots_host(P, uv, CAM, flags, min_root_joints=5)
    assert solved[0]


def test_unsolved_all_joints_on_one_pixel():
    from uplift_upsample_3dhpe_amd import predict
    P, T, uv = _one_frame()
    uv[:] = uv[0, 3]                                                     # den = Sq - (Sa^2 + Sb^2) / n is not > 0
    roots, solved = predict.solve_roots_host(P, uv, CAM)
    assert not solved[0] and (roots == 0).all()


def test_unsolved_behind_the_camera():
    from uplift_upsample_3dhpe_amd import predict
    P, T, uv = _one_frame()
    uv = _project(P, -T, CAM)                                            # the projections of a skeleton BEHIND the camera: Tz < 0
    roots, solved = predict.solve_roots_host(P, uv, CAM)
    assert not solved[0] and (roots == 0).all()
    # Tz > 0 but one used joint behind the camera: Z_j + Tz > 0 must hold for every used joint
    P2, T2 = np.abs(P), np.array([[0.0, 0.0, 0.5]])
    P2[0, 4, 2] = -0.8                                                   # (it projects mirrored, consistently: the solve itself finds T2)
    uv2 = _project(P2, T2, CAM)
    roots, solved = predict.solve_roots_host(P2, uv2, CAM)
    assert not solved[0] and (roots == 0).all()
    flags = np.ones((1, 17), bool)
    flags[0, 4] = False
    roots, solved = predict.solve_roots_host(P2, uv2, CAM, flags)
    assert solved[0] and np.abs(roots - T2).max() <= 1e-4


def test_non_finite_coordinate_on_a_flagged_joint_is_not_used():
    from uplift_upsample_3dhpe_amd import predict
    P, T, uv = _one_frame()
    flags = np.ones((1, 17), bool)
    spoiled = uv.copy()
    spoiled[0, 2, 0], spoiled[0, 9, 1] = np.nan, np.inf
    a, sa = predict.solve_roots_host(P, spoiled, CAM, flags)
    flags[0, [2, 9]] = False
    b, sb = predict.solve_roots_host(P, uv, CAM, flags)                  # the same joints unflagged instead
    assert sa[0] and sb[0] and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    flags[:] = False
    flags[0, [2, 9, 3, 4, 5, 6, 7]] = True                               # 7 flagged, 5 finite
    assert not predict.solve_roots_host(P, spoiled, CAM, flags)[1][0]
    assert predict.solve_roots_host(P, uv, CAM, flags)[1][0]


# ---- 3. the trajectory -------------------------------------------------------------------------------------------------------------------
def _roots(G, seed=5):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-2, 2, G), rng.uniform(-1, 1, G), rng.uniform(2, 10, G)], axis=1)


def _mix(a, b, w):
    """root[L] * (1 - w) + root[R] * w with an exact weight, correctly rounded steps: the reference value in Fractions."""
    w = np.float64(w.numerator) / np.float64(w.denominator)
    return (a * (1.0 - w) + b * w).astype(np.float32)


def test_trajectory_holds_the_ends_and_interpolates():
    from uplift_upsample_3dhpe_amd import predict
    roots = _roots(10)
    solved = np.zeros(10, bool)
    solved[[2, 3, 7]] = True
    out, state = predict.root_trajectory_host(roots, solved)
    assert out.dtype == np.float32 and state.dtype == np.uint8
    assert state.tolist() == [2, 2, 1, 1, 2, 2, 2, 1, 2, 2]
    for i in (0, 1):                                                     # held before the first solved frame
        assert np.array_equal(out[i], roots[2].astype(np.float32))
    for i in (8, 9):                                                     # and behind the last one
        assert np.array_equal(out[i], roots[7].astype(np.float32))
    for i in (2, 3, 7):
        assert np.array_equal(out[i], roots[i].astype(np.float32))
    for i in (4, 5, 6):
        assert np.array_equal(out[i], _mix(roots[3], roots[7], Fraction(i - 3, 4)))


def test_trajectory_without_a_solved_frame_and_of_one_frame():
    from uplift_upsample_3dhpe_amd import predict
    roots = _roots(6)
    solved = np.array([0, 0, 0, 1, 0, 0], bool)
    out, state = predict.root_trajectory_host(roots, solved, lens=[3, 1, 1, 1])
    assert state.tolist() == [0, 0, 0, 1, 0, 0] and (out[[0, 1, 2, 4, 5]] == 0).all()
    assert np.array_equal(out[3], roots[3].astype(np.float32))


def test_trajectory_does_not_leak_across_a_track_boundary():
    from uplift_upsample_3dhpe_amd import predict
    roots = _roots(10)
    solved = np.array([1, 1, 0, 0, 0, 0, 0, 0, 1, 1], bool)             # the touching ends of both tracks are unsolved
    out, state = predict.root_trajectory_host(roots, solved, lens=[5, 5])
    assert state.tolist() == [1, 1, 2, 2, 2, 2, 2, 2, 1, 1]
    for i in (2, 3, 4):
        assert np.array_equal(out[i], roots[1].astype(np.float32))       # held, not mixed with the next track's frame 8
    for i in (5, 6, 7):
        assert np.array_equal(out[i], roots[8].astype(np.float32))


def test_keyframes_only_positions():
    """s_in = 5, a video of 13 frames: keyframes 0, 5, 10 are given; returned frame i sits at i / 5."""
    from uplift_upsample_3dhpe_amd import predict, rates
    pos = rates.given_positions([13], [Fraction(1, 5)])
    assert [Fraction(int(n), int(d)) for n, d in zip(pos[1], pos[2])] == [Fraction(i, 5) for i in range(13)]
    base, wnum, wden = rates.root_plan([3], pos)
    assert base.tolist() == [i // 5 for i in range(13)] and wnum.tolist() == [i % 5 for i in range(13)] and (wden == 5).all()
    roots = _roots(3)
    out, state = predict.root_trajectory_host(roots, [1, 0, 1], [3], pos)
    assert state.tolist() == [1] + [2] * 9 + [1, 2, 2]
    for i in range(1, 10):                                               # across the unsolved keyframe 1: L = 0, R = 2, w = i / 10
        assert np.array_equal(out[i], _mix(roots[0], roots[2], Fraction(i, 10)))
    for i in (11, 12):                                                   # behind the last given frame: held, and not "solved here"
        assert np.array_equal(out[i], roots[2].astype(np.float32))
    out, state = predict.root_trajectory_host(roots, [0, 1, 0], [3], pos)
    assert state.tolist() == [2] * 5 + [1] + [2] * 7 and all(np.array_equal(o, roots[1].astype(np.float32)) for o in out)


@pytest.mark.parametrize("out_fps", [60, 24])
def test_out_fps_positions(out_fps):
    """fps = 30: returned frame i sits at given-frame position i * 30 / out_fps."""
    from uplift_upsample_3dhpe_amd import predict, rates
    T = 9
    n = (T - 1) * out_fps // 30 + 1
    out_lens, _ = rates.output_positions([T], 30, out_fps)
    assert out_lens.tolist() == [n]
    pos = rates.given_positions(out_lens, [Fraction(30, out_fps)])
    want = [Fraction(i * 30, out_fps) for i in range(n)]
    assert [Fraction(int(a), int(b)) for a, b in zip(pos[1], pos[2])] == want
    roots = _roots(T)
    solved = np.ones(T, bool)
    solved[[3, 4]] = False
    out, state = predict.root_trajectory_host(roots, solved, [T], pos)
    for i, p in enumerate(want):
        whole = p.denominator == 1
        if whole and solved[int(p)]:
            assert state[i] == 1 and np.array_equal(out[i], roots[int(p)].astype(np.float32))
            continue
        L = max(g for g in range(T) if solved[g] and g <= p)
        R = min(g for g in range(T) if solved[g] and g > p)
        assert state[i] == 2 and np.array_equal(out[i], _mix(roots[L], roots[R], (p - L) / (R - L))), (i, p)


# ---- 4. argument checks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", [(1.0, 1.0, 0.0), [(1.0, 1.0, 0.0, 0.0)] * 3, (0.0, 1.0, 0.0, 0.0), (1.0, -1.0, 0.0, 0.0),
                                    (np.nan, 1.0, 0.0, 0.0), (1.0, 1.0, np.inf, 0.0), "pinhole", None])
def test_bad_cameras(camera):
    from uplift_upsample_3dhpe_amd import predict
    P, T, uv = _one_frame()
    with pytest.raises(ValueError):
        predict.check_cameras(camera, 2)
    with pytest.raises(ValueError):
        predict.solve_roots_host(np.repeat(P, 2, 0), np.repeat(uv, 2, 0), camera, lens=[1, 1])


@pytest.mark.parametrize("m", [1, 0, -3, 2.5, True, None])
def test_bad_min_root_joints(m):
    from uplift_upsample_3dhpe_amd import predict
    P, T, uv = _one_frame()
    with pytest.raises(ValueError):
        predict.solve_roots_host(P, uv, CAM, min_root_joints=m)
    assert predict.solve_roots_host(P, uv, CAM, min_root_joints=2)[1][0]


def test_plan_refuses_what_the_device_could_not_index():
    from uplift_upsample_3dhpe_amd import rates
    with pytest.raises(ValueError):
        rates.root_plan([3], (np.array([0]), np.array([3]), np.array([1])))          # behind the last given frame
    with pytest.raises(ValueError):
        rates.root_plan([3], (np.array([1]), np.array([0]), np.array([1])))          # no such track
    with pytest.raises(ValueError):
        rates.root_plan([2 ** 30], (np.array([0]), np.array([1]), np.array([2 ** 23])))   # the weight's integers reach 2^53
    with pytest.raises(ValueError):
        rates.given_positions([2 ** 40], [Fraction(2 ** 20, 3)])
    base, wnum, wden = rates.root_plan([2, 3])
    assert base.tolist() == [0, 1, 2, 3, 4] and not wnum.any() and (wden == 1).all()
