"""GPU: the zero-lag, two-pass One-Euro filter on the device (include/uu3d.h, STEADY OUTPUT, ZERO LAG).  The reference is
predict.one_euro_host with a ``OneEuro(zero_lag=True)``, the rule in numpy (tests/test_smooth_zero_lag_cpu.py pins it to its definition);
every comparison with it is exact (the same IEEE float64 operations in the same order, no contraction).
  1. predict.one_euro with a zero-lag filter equals the mirror: tracks of 1, 2, 3, 40 and 65 rows and one without a usable row in one call,
     C = 3 / 51 / 75, per-track rates, NaN / Inf samples and state zeros at a track's first row, last row and middle, beta = 0 and
     beta > 0; the input is only read; the causal filter on the same input still equals the causal mirror
  2. predict_tracks(smooth=zero-lag filters) equals one_euro_host on predict_tracks(smooth=None): h36m_81 with seeded weights, missed
     detections and return_valid=True in every case -- the tuple's layout, the flags, root_state and the root joint's zero are unchanged
  3. predict_detections(smooth=OneEuro(zero_lag=True)) equals predict_tracks on the mirror's tracks"""
import numpy as np
import pytest

from tests import detections_util as du
from tests.tracks_util import RES, _bits, _model, _same_bits
from tests.zero_lag_util import composition, hard_input

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
LENS = [1, 2, 3, 40, 65, 4]                                           # (the last one: no usable row)
RATES = [50, 29.97, (30000, 1001), 50, 30, 29.97]


# ---- 1. the launch alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [3, 51, 75])
@pytest.mark.parametrize("params", [(1.0, 0.0, 1.0), (0.7, 2.5, 1.3)])
def test_two_pass_equals_the_mirror_bit_for_bit(channels, params):
    from uplift_upsample_3dhpe_amd import predict
    Z, F = predict.OneEuro(*params, zero_lag=True), predict.OneEuro(*params)
    G = sum(LENS)
    x, state = hard_input(LENS, channels, seed=channels)
    more, _ = hard_input(LENS, channels, seed=channels, long=4)        # the same rows, with the 65-row track's samples spoilt as well
    x[~np.isfinite(more)] = more[~np.isfinite(more)]
    state[sum(LENS[:4]) + 30:sum(LENS[:4]) + 33] = 0
    dx, ds = torch.from_numpy(x).cuda(), torch.from_numpy(state).cuda()
    before = dx.clone()
    for st, dst in ((None, None), (state, ds), (state, ds.view(torch.bool))):
        want = predict.one_euro_host(x, LENS, RATES, Z, state=st)
        got = predict.one_euro(dx, LENS, RATES, Z, state=dst)
        assert got.dtype == torch.float32 and tuple(got.shape) == (G, channels) and got.data_ptr() != dx.data_ptr()
        assert torch.equal(got.view(torch.int32).cpu(), torch.from_numpy(want).view(torch.int32)), np.argwhere(_bits(got) != _bits(want))[:5]
        # the old instantiation did not move, and the two differ
        causal = predict.one_euro_host(x, LENS, RATES, F, state=st)
        assert _same_bits(predict.one_euro(dx, LENS, RATES, F, state=dst), causal) and not np.array_equal(_bits(want), _bits(causal))
        bad = ~np.isfinite(x)
        assert bad.sum() == 8 and np.array_equal(_bits(want[bad]), _bits(x[bad])) and np.isfinite(want[~bad]).all()
        if st is not None:
            assert np.array_equal(_bits(want[state == 0]), _bits(x[state == 0]))
    assert np.array_equal(_bits(predict.one_euro_host(x, LENS, RATES, Z, state=state)), _bits(composition(x, LENS, RATES, Z, state)))
    assert torch.equal(before.view(torch.int32), dx.view(torch.int32))           # only read
    # one rate for all tracks, one track, a (G, J, 3) shape
    assert _same_bits(predict.one_euro(dx, None, 50, Z), predict.one_euro_host(x, None, 50, Z))
    if channels % 3 == 0:
        got = predict.one_euro(dx.view(G, channels // 3, 3), LENS, 25, Z)
        assert tuple(got.shape) == (G, channels // 3, 3) and _same_bits(got.view(G, channels), predict.one_euro_host(x, LENS, 25, Z))


# ---- 2. predict_tracks -------------------------------------------------------------------------------------------------------------------
TRACK_LENS = [1, 7, 101]
CAMS = [(1145.0, 1143.8, 512.5, 515.5), (1400.0, 1390.0, 960.0, 540.0), (600.0, 610.0, 320.0, 240.0)]


def _far_tracks(lens, seed, J=17):
    """People far from the camera, in pixels (tests/test_smooth_gpu.py): solved and unsolved frames mix whatever the weights.  The second
    track has every joint of a frame on one pixel: none of its frames can be solved."""
    rng = np.random.default_rng(seed)
    tracks = []
    for i, n in enumerate(lens):
        centre = rng.uniform(0.3, 0.7, size=2) * RES[i % len(RES)] + np.arange(n)[:, None] * np.array([1.5, 0.5])
        spread = rng.uniform(-4.0, 4.0, size=(n, J, 2)) if i != 1 else 0.0
        tracks.append(np.ascontiguousarray(np.broadcast_to(centre[:, None, :] + spread, (n, J, 2))).astype(np.float32))
    return tracks


def _case(name):
    """-> (tracks, keywords, the rate of the returned frames, with camera)."""
    tracks, kw, rate, placed = _far_tracks(TRACK_LENS, seed=61), {"mask_stride": 4}, 50, False
    if name == "keyframes":
        tracks = [t[::4] for t in tracks]
        kw.update(keyframes_only=True, lengths=TRACK_LENS)
    elif name == "fps30_out60":
        kw.update(fps=30, out_fps=60)
        rate = 60
    elif name in ("camera_both", "camera_mixed"):
        placed = True
    else:
        assert name == "plain"
    return tracks, kw, rate, placed


@pytest.mark.parametrize("name", ["plain", "keyframes", "fps30_out60", "camera_both", "camera_mixed"])
def test_predict_tracks_with_zero_lag_filters(name):
    from uplift_upsample_3dhpe_amd import predict
    tracks, kw, rate, placed = _case(name)
    cfg, arch, w, model = _model("h36m_81")
    kw["resolutions"] = [RES[i % len(RES)] for i in range(len(tracks))]
    P = predict.OneEuro(1.2, 0.8, 1.0, zero_lag=name != "camera_mixed")                # camera_mixed: causal poses, zero-lag roots
    R = predict.OneEuro(0.4, 0.3, 2.0, zero_lag=True)
    if placed:
        kw["camera"] = CAMS
    smooth = (P, R) if placed else P
    # missed detections in every case, so that the flags are not all True: frames 5 and 6 of the long track, frame 3 of a 7-frame one
    valid = [np.ones(len(t), np.uint8) for t in tracks]
    for v in valid:
        if len(v) > 6:
            v[[5, 6]] = 0
        elif len(v) > 3:
            v[3] = 0
    assert sum(int((v == 0).sum()) for v in valid) >= 2
    kw.update(valid=valid, return_valid=True)
    raw = predict.predict_tracks(model, cfg, tracks, **kw)
    got = predict.predict_tracks(model, cfg, tracks, smooth=smooth, rotations=True, **kw)
    # the tuple: (poses, flags[, roots, root_state]) and the rotations behind it
    assert isinstance(raw, tuple) and len(raw) == (4 if placed else 2) and isinstance(got, tuple) and len(got) == len(raw) + 1
    raw_poses, got_poses, turned = raw[0], got[0], got[-1]
    n = len(tracks)
    assert all(isinstance(part, list) and len(part) == n for part in got)
    assert all(tuple(q.shape) == (int(p.shape[0]), 17, 4) for p, q in zip(got_poses, turned))
    # the flags are those of the call without smooth, bit for bit, and some are False
    for a, b in zip(raw[1], got[1]):
        assert a.dtype == torch.bool and b.dtype == torch.bool and a.shape == b.shape and torch.equal(a, b)
    assert not torch.cat(got[1], 0).all() and torch.cat(got[1], 0).any()
    if placed:                                                        # roots (n_i, 3) float32 and root_state (n_i,) uint8 behind the flags
        assert all(tuple(r.shape) == (int(p.shape[0]), 3) and r.dtype == torch.float32 for p, r in zip(got_poses, got[2]))
        assert all(tuple(t.shape) == (int(p.shape[0]),) and t.dtype == torch.uint8 for p, t in zip(got_poses, got[3]))
        raw, got = (raw[0],) + raw[2:], (got[0],) + got[2:]           # (below: poses, roots, root_state)
    lens = [int(p.shape[0]) for p in raw_poses]
    assert [int(p.shape[0]) for p in got_poses] == lens and (name in ("keyframes", "fps30_out60") or lens == TRACK_LENS)
    flat = torch.cat(raw_poses, 0).cpu().numpy()
    want = predict.one_euro_host(flat, lens, rate, P)
    twin = predict.one_euro_host(flat, lens, rate, predict.OneEuro(*P, zero_lag=not P.zero_lag))
    assert not np.array_equal(_bits(want), _bits(flat)) and not np.array_equal(_bits(want), _bits(twin))
    shown = torch.cat(got_poses, 0)
    assert np.array_equal(_bits(shown), _bits(want))
    root = int(cfg.ROOT_KEYTPOINT)
    assert not flat[:, root].any() and not shown[:, root].any()        # the root joint: exactly 0 before and after
    # the rotations are those of the RETURNED (filtered) poses
    assert np.array_equal(_bits(torch.cat(turned, 0)), _bits(predict.joint_rotations_host(shown.cpu().numpy())[0]))
    if placed:
        raw_roots, raw_state = torch.cat(raw[1], 0).cpu().numpy(), torch.cat(raw[2], 0).cpu().numpy()
        assert np.array_equal(torch.cat(got[2], 0).cpu().numpy(), raw_state)          # root_state is unchanged: the root filter's state
        want_roots = predict.one_euro_host(raw_roots, lens, rate, R, state=raw_state)
        assert np.array_equal(_bits(torch.cat(got[1], 0)), _bits(want_roots))
        print(name, "root states", np.bincount(raw_state, minlength=3).tolist())
        assert not raw[2][1].any() and not got[1][1].any()            # the track without a solved frame: zeros, still
        assert (raw_state != 0).sum() > 20 and not np.array_equal(_bits(want_roots), _bits(raw_roots))
        assert not np.array_equal(_bits(want_roots), _bits(predict.one_euro_host(raw_roots, lens, rate, predict.OneEuro(*R), state=raw_state)))
    if name == "plain":                                               # smooth=True and the causal filter keep their bits
        for causal in (True, predict.OneEuro()):
            dflt = predict.predict_tracks(model, cfg, tracks, smooth=causal, **kw)
            assert np.array_equal(_bits(torch.cat(dflt[0], 0)), _bits(predict.one_euro_host(flat, lens, rate, predict.OneEuro())))


# ---- 3. predict_detections ---------------------------------------------------------------------------------------------------------------
def test_predict_detections_hands_a_zero_lag_filter_on():
    from uplift_upsample_3dhpe_amd import predict
    cfg, arch, w, model = _model("h36m_81")
    dets, counts, _ = du.scene()
    Z = predict.OneEuro(zero_lag=True)
    tracks = predict.association_tracks_host(dets, None, predict.associate_host(dets, counts, slots=du.S, **du.RULE))
    kw = dict(resolutions=du.RESOLUTION, mask_stride=4)
    got = predict.predict_detections(model, cfg, [dets], [counts], slots=du.S, smooth=Z, **du.RULE, **kw)
    track_kw = dict(valid=[f for _, _, _, f in tracks], **kw)
    ref = predict.predict_tracks(model, cfg, [xy for _, _, xy, _ in tracks], smooth=Z, **track_kw)
    plain = predict.predict_tracks(model, cfg, [xy for _, _, xy, _ in tracks], **track_kw)
    assert len(got) == 1 and [(tid, first) for tid, first, _ in got[0]] == [(tid, first) for tid, first, _, _ in tracks]
    for (_, _, p), q, raw in zip(got[0], ref, plain):
        assert p.shape == q.shape and np.array_equal(_bits(p), _bits(q))
        assert np.array_equal(_bits(p), _bits(predict.one_euro_host(raw.cpu().numpy(), None, 50, Z)))
    assert any(not np.array_equal(_bits(p), _bits(raw)) for (_, _, p), raw in zip(got[0], plain))
