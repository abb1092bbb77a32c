"""CPU: the live absolute root (include/uu3d.h, LIVE ABSOLUTE ROOT; stream.StreamSession(camera=...)) -- the rule in numpy
(stream.LiveRootHost) against the offline rule, the hold, the refusals that need no device, the command line."""
import types

import numpy as np
import pytest

from tests import util

CAMERA = (1145.0, 1143.5, 512.25, 515.75)
J = 17


def synthetic(frames, seed, J=J, camera=CAMERA):
    """Geometry that solves: random root-relative poses P (extent about 1), a root T with Tz well above that extent, and the projection
    of P + T through the camera, rounded to float32 -> (poses (frames, J, 3) f32, kp2d (frames, J, 2) f32, T (frames, 3) f64)."""
    rng = np.random.default_rng(seed)
    P = rng.uniform(-0.8, 0.8, size=(frames, J, 3)).astype(np.float32)
    T = np.stack([rng.uniform(-1.5, 1.5, frames), rng.uniform(-1.0, 1.0, frames), rng.uniform(4.0, 7.0, frames)], axis=1)
    X = P.astype(np.float64) + T[:, None]
    fx, fy, cx, cy = camera
    uv = np.stack([fx * X[..., 0] / X[..., 2] + cx, fy * X[..., 1] / X[..., 2] + cy], axis=-1).astype(np.float32)
    return P, uv, T


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("lookahead", [0, 5])
def test_mirror_equals_the_offline_rule_where_every_frame_is_solved(lookahead):
    from uplift_upsample_3dhpe_amd import predict, stream
    n = 30
    P, uv, T = synthetic(n, seed=11)
    want, solved = predict.solve_roots_host(P, uv, CAMERA)
    assert solved.all()
    host = stream.LiveRootHost(J, lookahead, CAMERA)
    got, states = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)
    for t in range(n + lookahead):                                    # the pose of frame c comes back at the push of frame c + lookahead
        c = t - lookahead
        frame = uv[t] if t < n else np.full((J, 2), np.nan, np.float32)      # (frames behind the end: never read by a solve)
        root, state = host.step(frame, None, P[c] if c >= 0 else None)
        if c < 0:
            assert state == 0 and not root.any()
            continue
        got[c], states[c] = root, state
        assert state == 1 and np.array_equal(bits(root), bits(want[c].astype(np.float32))), c
    traj, traj_state = predict.root_trajectory_host(want, solved)
    assert np.array_equal(bits(got), bits(traj)) and np.array_equal(states, traj_state)
    dev = float(np.abs(got.astype(np.float64) - T).max() / np.abs(T).max())
    print(f"lookahead {lookahead}: largest deviation of the solved root from T, relative: {dev:.3e}")
    assert np.allclose(got, T, rtol=1e-5, atol=1e-5 * float(np.abs(T).max()))


@pytest.mark.parametrize("lookahead", [0, 3])
def test_hold(lookahead):
    """Frames that cannot be solved -- too few flags, NaN coordinates, a missing frame flag -- return the previous solved root's bits with
    state 2, and zeros with state 0 before the first solved frame; a joint whose flag is clear is never used."""
    from uplift_upsample_3dhpe_amd import predict, stream
    n, m = 24, 6
    P, uv, _ = synthetic(n, seed=5)
    uv = uv.copy()
    flags = np.ones((n, J), bool)
    flags[0:2, m - 1:] = False                                        # m - 1 used joints: below min_root_joints, before any solved frame
    flags[6, 3:] = False                                              # too few flags
    uv[9, 2:] = np.nan                                                # too few finite joints
    frame_flag = np.ones(n, bool)
    frame_flag[12:14] = False                                         # a missing frame: its flag stands for all of its joints
    flags[16, 4] = False                                              # a filled joint, moved far away: using it would change the root
    uv[16, 4] += 300.0
    used = flags & frame_flag[:, None]
    want, solved = predict.solve_roots_host(P, uv, CAMERA, flags=used, min_root_joints=m)
    unsolved = [0, 1, 6, 9, 12, 13]
    assert np.flatnonzero(~solved).tolist() == unsolved
    clean = uv.copy()
    clean[16, 4] -= 300.0
    assert not np.array_equal(predict.solve_roots_host(P[16:17], uv[16:17], CAMERA)[0], want[16:17])       # the moved joint would show
    assert np.array_equal(want[16], predict.solve_roots_host(P[16:17], clean[16:17], CAMERA, flags=used[16:17])[0][0])
    host = stream.LiveRootHost(J, lookahead, CAMERA, m)
    last = None
    for t in range(n + lookahead):
        c = t - lookahead
        k = min(t, n - 1)
        # the frame flag as one flag for the whole frame on even pushes, folded into the per-joint flags on odd ones
        root, state = (host.step(uv[k], frame_flag[k], P[c] if c >= 0 else None) if flags[k].all() and t % 2 == 0 else
                       host.step(uv[k], used[k], P[c] if c >= 0 else None))
        if c < 0:
            assert state == 0 and not root.any()
        elif c in unsolved:
            assert state == (0 if last is None else 2), c
            assert np.array_equal(bits(root), bits(np.zeros(3) if last is None else last)), c
        else:
            last = want[c].astype(np.float32)
            assert state == 1 and np.array_equal(bits(root), bits(last)), c
    # a push that is not fresh returns the previous push's root and state; a reset starts again
    root, state = host.step(uv[0], None, None)
    assert state == 1 and np.array_equal(bits(root), bits(last))
    host.reset()
    root, state = host.step(uv[0], None, None)
    assert state == 0 and not root.any() and host.frames == 1


def _stub_model():
    return types.SimpleNamespace(arch=types.SimpleNamespace(compiled_dims=True), device="cpu", has_strided_input=True)


def test_refusals_need_no_device():
    from uplift_upsample_3dhpe_amd import stream
    cfg = util.load_config("h36m_81")

    def plan(fps=None, out_fps=None, lookahead=5, **kw):
        s = object.__new__(stream.StreamSession)
        s._init_plan(_stub_model(), cfg, 3, (1920, 1080), 4, True, lookahead, True, False, fps, 50, out_fps, **kw)
        return s

    with pytest.raises(ValueError, match="camera together with out_fps is not supported yet.*later change"):
        plan(fps=10, out_fps=50, lookahead=40, camera=CAMERA)
    with pytest.raises(ValueError, match="ONE camera.*shares one space"):
        plan(detections=4, camera=[CAMERA] * 3)
    for bad in ((1.0, 2.0, 3.0), (0.0, 1.0, 2.0, 3.0), (1.0, float("nan"), 2.0, 3.0), [CAMERA] * 2, "pinhole"):
        with pytest.raises(ValueError, match="camera must be"):
            plan(camera=bad)
    for bad in (1, 0, 2.5, True):
        with pytest.raises(ValueError, match="min_root_joints must be an int >= 2"):
            plan(camera=CAMERA, min_root_joints=bad)
    with pytest.raises(ValueError, match="min_root_joints needs camera"):
        plan(min_root_joints=6)
    wide = cfg.copy()
    wide.NUM_KEYPOINTS = 65
    s = object.__new__(stream.StreamSession)
    with pytest.raises(ValueError, match="at most 64 joints"):
        s._init_plan(_stub_model(), wide, 3, None, 4, True, 5, True, False, None, 50, None, camera=CAMERA)
    # through the constructor's **options gate, before any device is touched
    with pytest.raises(ValueError, match="camera together with out_fps"):
        stream.StreamSession(_stub_model(), cfg, slots=2, mask_stride=4, lookahead=40, fps=10, out_fps=50, camera=CAMERA)
    with pytest.raises(TypeError, match="unexpected keyword argument 'cameras'"):
        stream.StreamSession(_stub_model(), cfg, slots=2, mask_stride=4, cameras=CAMERA)
    # the plan of a session with a camera; one tuple serves a session with detections
    s = plan(camera=CAMERA)
    assert s.cameras.shape == (3, 4) and s.cameras.dtype == np.float64 and s.min_root_joints == 6
    s = plan(camera=[CAMERA, (1.0, 2.0, 3.0, 4.0), CAMERA], min_root_joints=4)
    assert s.cameras[1].tolist() == [1.0, 2.0, 3.0, 4.0] and s.min_root_joints == 4
    assert plan(detections=4, camera=CAMERA).cameras.shape == (3, 4)
    assert plan().cameras is None and plan().min_root_joints is None


def test_c_abi_declared_and_refusing():
    import ctypes as C
    import __graft_entry__ as ge
    ge.build()
    from uplift_upsample_3dhpe_amd import _capi
    lib = _capi.load_library()
    header = open(util.ROOT + "/include/uu3d.h").read()
    assert "LIVE ABSOLUTE ROOT" in header
    for s in ("uu3d_stream_root_bytes", "uu3d_stream_root", "uu3d_stream_root_reset"):
        assert s in _capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert lib.uu3d_stream_root_bytes(5, 17, 6) >= 5 * (24 + 7 * 17 * 9 + 1) and lib.uu3d_stream_root_bytes(5, 17, 6) % 256 == 0
    assert lib.uu3d_stream_root_bytes(0, 17, 0) == 0 and lib.uu3d_stream_root_bytes(1, 65, 0) == 0 and lib.uu3d_stream_root_bytes(1, 17, -1) == 0
    block = C.c_void_p(256)                                           # (an aligned address that is never dereferenced: the calls refuse first)
    assert lib.uu3d_stream_root_reset(1, 65, 0, block, None, None) == _capi.UU3D_ERR_UNSUPPORTED
    assert lib.uu3d_stream_root(1, 65, 0, block, None, None, None, None, None, None, 0, None, 6, None, None, None) == _capi.UU3D_ERR_UNSUPPORTED
    assert lib.uu3d_stream_root(1, 17, 0, block, None, None, None, None, None, None, 0, None, 6, None, None, None) == _capi.UU3D_ERR_INVALID_ARGUMENT
    assert lib.uu3d_stream_root_reset(1, 17, 0, None, None, None) == _capi.UU3D_ERR_INVALID_ARGUMENT


def test_command_line(tmp_path, monkeypatch):
    from uplift_upsample_3dhpe_amd import stream
    base = ["--config", "c.json", "--weights", "w.h5", "--input", "i.npz", "--output", "o.npz"]
    a = stream.parse_args(base)
    assert a.camera is None and a.min_root_joints is None
    a = stream.parse_args(base + ["--camera", "1145", "1143.5", "512.25", "515.75", "--min_root_joints", "4", "--lookahead", "7"])
    assert tuple(a.camera) == CAMERA and a.min_root_joints == 4 and a.lookahead == 7
    for bad in (["--min_root_joints", "4"], ["--camera", "1", "2", "3"], ["--camera", "1", "1", "0", "0", "--fps", "10", "--out_fps", "50"]):
        with pytest.raises(SystemExit):
            stream.parse_args(base + bad)
    # main: the refusals in front of the model, then what it hands on and writes
    cfg = util.ROOT + "/config/h36m_81.json"
    rng = np.random.default_rng(0)
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    args = ["--config", cfg, "--weights", "none.h5", "--input", inp, "--output", out]
    monkeypatch.setattr(stream, "_load_model", lambda config, weights: "model")
    seen = {}

    def fake_replay(model, config, tracks, **kw):
        seen["kw"] = kw
        res = [np.zeros((len(t), 17, 3), np.float32) for t in tracks], [np.ones(len(t), bool) for t in tracks]
        if kw.get("camera") is not None:
            res += ([np.full((len(t), 3), 2.0, np.float32) for t in tracks], [np.full(len(t), 1, np.uint8) for t in tracks])
        return res
    monkeypatch.setattr(stream, "replay_tracks", fake_replay)
    np.savez(inp, walk=rng.normal(size=(6, 17, 2)).astype(np.float32), walk__root=rng.normal(size=(6, 17, 2)).astype(np.float32))
    with pytest.raises(SystemExit, match="__root or __root_state would collide"):
        stream.main(args + ["--camera", "1145", "1143.5", "512.25", "515.75"])
    assert stream.main(args) == 0 and "camera" not in seen["kw"]      # without --camera such a key is a track like any other
    np.savez(inp, walk=rng.normal(size=(6, 17, 2)).astype(np.float32))
    with pytest.raises(SystemExit, match="--camera: camera must be finite"):
        stream.main(args + ["--camera", "0", "1143.5", "512.25", "515.75"])
    with pytest.raises(SystemExit, match="--camera: min_root_joints must be"):
        stream.main(args + ["--camera", "1145", "1143.5", "512.25", "515.75", "--min_root_joints", "1"])
    assert stream.main(args + ["--camera", "1145", "1143.5", "512.25", "515.75"]) == 0
    assert seen["kw"]["camera"] == CAMERA and seen["kw"]["min_root_joints"] == 6
    with np.load(out) as z:
        assert sorted(z.files) == ["walk", "walk__root", "walk__root_state", "walk_fresh"]
        assert z["walk__root"].shape == (6, 3) and z["walk__root"].dtype == np.float32
        assert z["walk__root_state"].shape == (6,) and z["walk__root_state"].dtype == np.uint8
