"""Any skeleton on the device: uu3d_map_keypoints, predict_tracks(keypoints=M), StreamSession(keypoints=M).
  1. the kernel alone, bit for bit against predict.map_keypoints_host
  2. predict_tracks(keypoints=M, valid=V) == predict_tracks(*map_keypoints_host(M, tracks, V)), bit for bit
  3. a live session with keypoints == the same session without, pushed the host-mapped frames and flags, bit for bit at every tick"""
import ctypes as C

import numpy as np
import pytest

from tests.tracks_util import RES, _bits, _model, _pixel_tracks, _same_bits

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
T = 3
SENTINEL = 7.0


def _hand_map():
    """K_in = 13 < J = 17: single sources, pairs, one joint with 8 sources and one negative weight, source 12 unlisted."""
    from uplift_upsample_3dhpe_amd import predict
    sources = [[j % 12] for j in range(17)]
    weights = [[1.0] for _ in range(17)]
    sources[4], weights[4] = [0, 1, 2, 3, 4, 5, 6, 7], [0.25, 0.25, 0.125, 0.125, 0.125, 0.25, -0.25, 0.125]
    sources[9], weights[9] = [11, 3], [1.5, -0.5]
    sources[13], weights[13] = [2, 8, 5], [1.0 / 3, 1.0 / 3, 1.0 - 2.0 / 3]
    return predict.KeypointMap(13, sources, weights)


def _spoiled(x, flags, seed):
    """NaN / Inf coordinates in place, in listed sources and (where the map has one) an unlisted one; Inf of both signs in one joint."""
    rng = np.random.default_rng(seed)
    F, K = x.shape[:2]
    for f in range(F):
        k = int(rng.integers(K))
        x[f, k, int(rng.integers(2))] = [np.nan, np.inf, -np.inf][f % 3]
    if F > 2:
        x[2, 0], x[2, 1] = [np.inf, 1.0], [-np.inf, 2.0]                 # Inf - Inf inside a sum: an invalid sum's NaN
    x[0, K - 1] = np.nan                                                 # (unlisted in the hand-made map and in body25's toes and heels)
    x[F - 1, 0, 1] = np.nan                                              # (source 0 is listed in every map here)
    return x


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 7, 257])
@pytest.mark.parametrize("name", ["body25", "coco17", "hand"])
def test_kernel_alone_bit_for_bit(name, F):
    from uplift_upsample_3dhpe_amd import _capi, predict
    from uplift_upsample_3dhpe_amd._capi import ptr
    cfg, arch, w, model = _model("h36m_81")
    lib, h, dev = _capi.load_library(), model._h, model.device
    M = _hand_map() if name == "hand" else predict.KEYPOINT_PRESETS[name]
    K, J = M.inputs, 17
    x = _pixel_tracks([F], seed=F, J=K)[0] - np.float32(300.0)
    flags = np.random.default_rng(F + 1).uniform(size=(F, K)) >= 0.15
    x = _spoiled(x, flags, F)
    src = torch.from_numpy(x).to(dev)
    before = src.clone()
    table = M.device_table(dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for with_flags in (False, True):
        out = torch.full((F + 1, J, 2), SENTINEL, dtype=torch.float32, device=dev)        # one row behind the end: nobody's
        fl_out = torch.full((F + 1, J), 9, dtype=torch.uint8, device=dev)
        fl_in = torch.from_numpy(flags.view(np.uint8)).to(dev) if with_flags else None
        _capi.check(lib, lib.uu3d_map_keypoints(h, ptr(table), K, ptr(src), ptr(fl_in), F, ptr(out), ptr(fl_out) if with_flags else None, stream), h)
        want, want_flags = predict.map_keypoints_host(M, [x], [flags] if with_flags else None)
        got = out.cpu().numpy()
        assert np.array_equal(_bits(got[:F]), _bits(want[0])), (name, F, with_flags)
        assert (got[F] == SENTINEL).all() and (fl_out[F] == 9).all()
        if with_flags:
            assert np.array_equal(fl_out[:F].cpu().numpy(), want_flags[0].astype(np.uint8))
            assert not want_flags[0].all() and want_flags[0].any() and np.isfinite(got[:F]).all()
        else:
            assert (fl_out == 9).all() and np.isnan(got[:F]).any()
        assert torch.equal(before.view(torch.int32), src.view(torch.int32))                # the caller's memory is only read
    # predict.map_keypoints is the same launch
    a, fa = predict.map_keypoints(src, torch.from_numpy(flags.view(np.uint8)).to(dev), M, model)
    assert _same_bits(a, want[0]) and np.array_equal(fa.cpu().numpy(), want_flags[0].astype(np.uint8))
    # F = 0 returns OK and writes nothing; flags on one side only, or inputs < 1, are refused
    out = torch.full((4, J, 2), SENTINEL, dtype=torch.float32, device=dev)
    fl_out = torch.full((4, J), 9, dtype=torch.uint8, device=dev)
    assert lib.uu3d_map_keypoints(h, ptr(table), K, ptr(src), ptr(fa), 0, ptr(out), ptr(fl_out), stream) == _capi.UU3D_OK
    assert lib.uu3d_map_keypoints(h, ptr(table), K, ptr(src), None, 0, ptr(out), None, stream) == _capi.UU3D_OK
    assert lib.uu3d_map_keypoints(h, ptr(table), K, ptr(src), ptr(fa), 1, ptr(out), None, stream) == _capi.UU3D_ERR_INVALID_ARGUMENT
    assert lib.uu3d_map_keypoints(h, ptr(table), K, ptr(src), None, 1, ptr(out), ptr(fl_out), stream) == _capi.UU3D_ERR_INVALID_ARGUMENT
    assert lib.uu3d_map_keypoints(h, ptr(table), 0, ptr(src), None, 1, ptr(out), None, stream) == _capi.UU3D_ERR_INVALID_ARGUMENT
    assert (out == SENTINEL).all() and (fl_out == 9).all()


# ---- 2. predict_tracks -----------------------------------------------------------------------------------------------------------------
LENS = [1, 9, 130]


@pytest.fixture(scope="module")
def coco_case():
    """Tracks of COCO-17 joints with lost joints as NaN, (T, K_in) flags at a 10 % share, and both through the host rule."""
    from uplift_upsample_3dhpe_amd import predict
    tracks = _pixel_tracks(LENS, seed=21)
    flags = [np.random.default_rng(30 + i).uniform(size=(n, 17)) >= 0.10 for i, n in enumerate(LENS)]
    flags[0][:] = True                                                   # (a lone frame with a lost joint is a lost track)
    holes = [t.copy() for t in tracks]
    flags[2][40:46, 5] = False                                           # l_sho lost for 6 frames: neck and torso with it, too long to fill
    for t, f in zip(holes[1:], flags[1:]):
        t[~f] = np.nan
    return tracks, holes, flags


@pytest.mark.parametrize("case", ["none", "finite", "repair", "repair_fps", "keyframes"])
def test_predict_tracks_identity(coco_case, case):
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model("h36m_81")
    tracks, holes, flags = coco_case
    kw = {"resolutions": RES, "mask_stride": 4}
    if case == "none":
        given, valid = tracks, None
    elif case == "finite":
        given, valid = holes, "finite"
    else:
        given, valid = tracks, flags
        kw["repair_joints"] = 3
    if case == "repair_fps":
        kw["fps"] = 30
    if case == "keyframes":
        kw.update(keyframes_only=True, lengths=[(n - 1) * 4 + 1 for n in LENS])
    got = predict.predict_tracks(model, cfg, given, keypoints="coco17", valid=valid, return_valid=True, **kw)
    mapped, mapped_valid = predict.map_keypoints_host("coco17", given, valid)
    want = predict.predict_tracks(model, cfg, mapped, valid=mapped_valid, return_valid=True, **kw)
    assert len(got) == len(want) == (3 if "repair_joints" in kw else 2)
    for part_got, part_want in zip(got, want):                           # poses, frame flags (, joint states): the same bits
        assert len(part_got) == len(part_want) == len(LENS)
        for a, b in zip(part_got, part_want):
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert all(torch.isfinite(p).all() for p in got[0]) or case == "none"
    if case != "none":
        assert not all(bool(f.all()) for f in got[1])                    # the cases do lose frames
    if "repair_joints" in kw:
        assert got[2][2].shape == (LENS[2], 17) and (got[2][2] == 2).any()                # joint_state per MODEL joint, with fills


def test_predict_tracks_refusals_and_none(coco_case):
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model("h36m_81")
    tracks, holes, flags = coco_case
    with pytest.raises(ValueError, match="17 keypoints.*takes 25"):
        predict.predict_tracks(model, cfg, tracks, keypoints="body25", resolutions=RES, mask_stride=4)
    with pytest.raises(ValueError, match=r"valid\[0\] must be \(1,\)"):  # per-joint flags are per detector joint
        predict.predict_tracks(model, cfg, _pixel_tracks(LENS, seed=3, J=25), keypoints="body25", valid=flags, repair_joints=3, mask_stride=4)
    # keypoints=None is today's call; the identity map onto the model's own joints gives its bits as well
    plain = predict.predict_tracks(model, cfg, tracks, resolutions=RES, mask_stride=4)
    none = predict.predict_tracks(model, cfg, tracks, resolutions=RES, mask_stride=4, keypoints=None)
    same = predict.predict_tracks(model, cfg, tracks, resolutions=RES, mask_stride=4,
                                  keypoints=predict.KeypointMap(17, [[j] for j in range(17)], [[1.0]] * 17))
    for a, b, c in zip(plain, none, same):
        assert _same_bits(a, b) and _same_bits(a, c)


# ---- 3. live ---------------------------------------------------------------------------------------------------------------------------
def _push_all(s, frames, flags, ticks, device_flags=False, reset_at=None):
    """Push frames[i][k] (and flags[i][k]) into slot i at tick k -> (poses, fresh, joint states or None) per tick, as host arrays."""
    J = 17
    poses = torch.zeros((ticks, T, J, 3), dtype=torch.float32, device="cuda")
    fresh = torch.zeros((ticks, T), dtype=torch.bool, device="cuda")
    states = torch.zeros((ticks, T, J), dtype=torch.uint8, device="cuda") if s.repair_joints is not None else None
    for k in range(ticks):
        if reset_at is not None and k == reset_at[0]:
            s.reset([reset_at[1]])
        v = None
        if flags is not None:
            v = np.stack([np.asarray(flags[i][k]) for i in range(T)])
            v = torch.from_numpy(v).cuda() if device_flags else v
        p, f = s.push(np.stack([frames[i][k] for i in range(T)]), valid=v)
        assert s.captures == int(s.graph)
        poses[k].copy_(p)
        fresh[k].copy_(f)
        if states is not None:
            states[k].copy_(s.joint_state)
    assert s.check_range() is False
    return poses.cpu().numpy(), fresh.cpu().numpy(), None if states is None else states.cpu().numpy()


def _equal(a, b):
    return np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and (a[2] is None) == (b[2] is None) and \
        (a[2] is None or np.array_equal(a[2], b[2]))


@pytest.mark.parametrize("kind", ["plain", "repair", "fps"])
def test_live_session_equals_the_host_mapped_session(kind):
    from uplift_upsample_3dhpe_amd import predict, stream
    cfg, arch, w, model = _model("h36m_81")
    ms, ticks = 4, 124                                                   # about 1.5 spans of the 41 x 2 frame window
    name = "body25" if kind == "plain" else "coco17"
    M = predict.KEYPOINT_PRESETS[name]
    tracks = _pixel_tracks([ticks] * T, seed=40, J=M.inputs)
    rng = np.random.default_rng(41)
    kw, flags, lookahead = {}, None, 3
    if kind == "repair":
        kw = {"repair_joints": 3}
        flags = [rng.uniform(size=(ticks, M.inputs)) >= 0.10 for _ in range(T)]
        tracks[1][17, 5] = np.nan                                        # a non-finite source is an unobserved one, whatever its flag
    if kind == "fps":
        kw = {"fps": 30, "missed_detections": True}
        lookahead = stream.rate_plan(cfg, 30, None, ms).min_lookahead + 1
        flags = [rng.uniform(size=ticks) >= 0.10 for _ in range(T)]      # (slots,) frame flags pass through
        tracks[2][30, 0, 1] = np.inf                                     # ... and a non-finite nose loses its frame: head and head top
    mapped, mapped_flags = predict.map_keypoints_host(M, tracks, flags)
    new = lambda graph=True, **more: stream.StreamSession(model, cfg, slots=T, resolutions=RES, mask_stride=ms, flip=True, lookahead=lookahead,
                                                          graph=graph, **kw, **more)
    s = new()
    want = _push_all(s, mapped, mapped_flags, ticks)
    s.close()
    assert want[1].any() and (kind != "repair" or (want[2] == 2).any())
    s = new(keypoints=name)
    assert s.captures == 1
    got = _push_all(s, tracks, flags, ticks, device_flags=kind == "repair")
    assert s.captures == 1
    if M.inputs != 17:                                                   # the model's own layout is refused once the session has a map
        with pytest.raises(ValueError, match=r"kp2d must be \(3, 25, 2\)"):
            s.push(mapped[0][:T])
    s.close()
    assert _equal(got, want)
    # graph on equals graph off
    s = new(graph=False, keypoints=name)
    off = _push_all(s, tracks, flags, ticks)
    assert s.captures == 0
    s.close()
    assert _equal(off, got)
    # a reset of one slot leaves the others' bits alone (and the slot itself starts a new track: the first ticks' bits again)
    at = 50
    s = new(keypoints=name)
    again = _push_all(s, [tracks[0], np.concatenate([tracks[1][:at], tracks[1]]), tracks[2]],
                      None if flags is None else [flags[0], np.concatenate([flags[1][:at], flags[1]]), flags[2]], ticks, reset_at=(at, 1))
    s.close()
    for i in (0, 2):
        assert np.array_equal(_bits(again[0][:, i]), _bits(got[0][:, i])) and np.array_equal(again[1][:, i], got[1][:, i])
    n = ticks - at
    assert np.array_equal(again[1][at:, 1], got[1][:n, 1])
    live = got[1][:n, 1]
    assert live.any() and np.array_equal(_bits(again[0][at:, 1][live]), _bits(got[0][:n, 1][live]))
