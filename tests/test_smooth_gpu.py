"""GPU: steady output on the device (include/uu3d.h, STEADY OUTPUT).  The reference is predict.one_euro_host, the rule in numpy; every
comparison with it is exact (the same IEEE float64 operations in the same order, no contraction).
  1. predict.one_euro equals one_euro_host: tracks of 1, 2, 3, 65 and 130 rows in one call, C = 3 / 51 / 75, per-track rates, a NaN sample,
     state rows, beta = 0 and beta > 0; the input is only read
  2. predict_tracks(smooth=F) equals one_euro_host on predict_tracks(smooth=None): h36m_81 with seeded weights, tracks of 1, 7 and 101 frames"""
import numpy as np
import pytest

from tests.tracks_util import RES, _bits, _model, _same_bits

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
LENS = [1, 2, 3, 65, 130]
RATES = [50, 30, (2997, 100), 50, 30]


def _signal(rows, channels, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(rows, dtype=np.float64)[:, None]
    return (np.sin(t * rng.uniform(0.02, 0.3, channels) + rng.uniform(0, 6, channels)) * rng.uniform(0.1, 3.0, channels)
            + 0.05 * rng.normal(size=(rows, channels))).astype(np.float32)


# ---- 1. the launch alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [3, 51, 75])
@pytest.mark.parametrize("params", [(1.0, 0.0, 1.0), (0.7, 2.5, 1.3)])
def test_one_euro_equals_the_mirror_bit_for_bit(channels, params):
    from uplift_upsample_3dhpe_amd import predict
    F = predict.OneEuro(*params)
    G = sum(LENS)
    x = _signal(G, channels, seed=channels)
    x[30, channels // 2] = np.nan                                     # one NaN sample, in the middle of the 65-row track
    state = np.ones(G, np.uint8)
    state[[6, 7]] = 0                                                 # the start of the 65-row track
    state[[40, 41, 42]] = 0                                           # ... and its middle
    state[3:6] = 0                                                    # the whole 3-row track
    dx, ds = torch.from_numpy(x).cuda(), torch.from_numpy(state).cuda()
    before = dx.clone()
    for st, dst in ((None, None), (state, ds), (state, ds.view(torch.bool))):
        want = predict.one_euro_host(x, LENS, RATES, F, state=st)
        got = predict.one_euro(dx, LENS, RATES, F, state=dst)
        assert got.dtype == torch.float32 and tuple(got.shape) == (G, channels) and got.data_ptr() != dx.data_ptr()
        assert torch.equal(got.view(torch.int32).cpu(), torch.from_numpy(want).view(torch.int32)), np.argwhere(_bits(got) != _bits(want))[:5]
        assert np.isnan(want[30, channels // 2]) and np.isfinite(np.delete(want.reshape(-1), 30 * channels + channels // 2)).all()
        if st is not None:
            assert np.array_equal(_bits(want[state == 0]), _bits(x[state == 0]))
    assert torch.equal(before.view(torch.int32), dx.view(torch.int32))           # only read
    # one rate for all tracks, one track, a (G, J, 3) shape
    want = predict.one_euro_host(x, None, 50, F)
    assert _same_bits(predict.one_euro(dx, None, 50, F), want)
    if channels % 3 == 0:
        got = predict.one_euro(dx.view(G, channels // 3, 3), LENS, 25, F)
        assert tuple(got.shape) == (G, channels // 3, 3) and _same_bits(got.view(G, channels), predict.one_euro_host(x, LENS, 25, F))
    with pytest.raises(ValueError):
        predict.one_euro(dx, [G - 1], 50, F)
    with pytest.raises(ValueError):
        predict.one_euro(dx, LENS, [50, 30], F)
    with pytest.raises(ValueError):
        predict.one_euro(dx, None, 50, (1.0, 0.5, 1.0))
    with pytest.raises(ValueError):
        predict.one_euro(dx.t(), None, 50, F)


# ---- 2. predict_tracks -------------------------------------------------------------------------------------------------------------------
TRACK_LENS = [1, 7, 101]
CAMS = [(1145.0, 1143.8, 512.5, 515.5), (1400.0, 1390.0, 960.0, 540.0), (600.0, 610.0, 320.0, 240.0)]


def _far_tracks(lens, seed, J=17):
    """People far from the camera, in pixels (tests/test_root_gpu.py): solved and unsolved frames mix whatever the weights.  The second
    track has every joint of a frame on one pixel: none of its frames can be solved (the denominator is not > 0)."""
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
    elif name == "fps30":
        kw["fps"], rate = 30, 30
    elif name == "fps30_out60":
        kw.update(fps=30, out_fps=60)
        rate = 60
    elif name in ("camera_both", "camera_root"):
        placed = True
    else:
        assert name == "plain"
    return tracks, kw, rate, placed


@pytest.mark.parametrize("name", ["plain", "keyframes", "fps30", "fps30_out60", "camera_both", "camera_root"])
def test_predict_tracks_with_smooth(name):
    from uplift_upsample_3dhpe_amd import predict
    tracks, kw, rate, placed = _case(name)
    cfg, arch, w, model = _model("h36m_81")
    n = len(tracks)
    kw["resolutions"] = [RES[i % len(RES)] for i in range(n)]
    P, R = predict.OneEuro(1.2, 0.8, 1.0), predict.OneEuro(0.4, 0.3, 2.0)
    if placed:
        kw["camera"] = CAMS
    smooth = {"camera_both": (P, R), "camera_root": (None, R)}.get(name, P)
    raw = predict.predict_tracks(model, cfg, tracks, **kw)
    got = predict.predict_tracks(model, cfg, tracks, smooth=smooth, **kw)
    raw_poses, got_poses = (raw[0], got[0]) if placed else (raw, got)
    lens = [int(p.shape[0]) for p in raw_poses]
    assert [int(p.shape[0]) for p in got_poses] == lens and (name in ("keyframes", "fps30", "fps30_out60") or lens == TRACK_LENS)
    flat = torch.cat(raw_poses, 0).cpu().numpy()
    if name == "camera_root":
        want = flat                                                   # no pose filter: the poses of the call without smooth
    else:
        want = predict.one_euro_host(flat, lens, rate, P)
        assert not np.array_equal(_bits(want), _bits(flat))
    assert np.array_equal(_bits(torch.cat(got_poses, 0)), _bits(want))
    root = int(cfg.ROOT_KEYTPOINT)
    assert not flat[:, root].any() and not torch.cat(got_poses, 0)[:, root].any()      # the root joint: exactly 0 before and after
    if placed:
        assert isinstance(got, tuple) and len(got) == 3
        raw_roots, raw_state = torch.cat(raw[1], 0).cpu().numpy(), torch.cat(raw[2], 0).cpu().numpy()
        assert np.array_equal(torch.cat(got[2], 0).cpu().numpy(), raw_state)          # root_state is unchanged
        want_roots = predict.one_euro_host(raw_roots, lens, rate, R, state=raw_state)
        assert np.array_equal(_bits(torch.cat(got[1], 0)), _bits(want_roots))
        print(name, "root states", np.bincount(raw_state, minlength=3).tolist())
        assert not raw[2][1].any() and not got[1][1].any()            # the track without a solved frame: zeros, still
        assert (raw_state != 0).sum() > 20 and not np.array_equal(_bits(want_roots), _bits(raw_roots))
    # a single filter serves poses and roots alike; True is the defaults
    if name == "camera_both":
        both = predict.predict_tracks(model, cfg, tracks, smooth=P, **kw)
        assert np.array_equal(_bits(torch.cat(both[0], 0)), _bits(want))
        assert np.array_equal(_bits(torch.cat(both[1], 0)), _bits(predict.one_euro_host(raw_roots, lens, rate, P, state=raw_state)))
    if name == "plain":
        dflt = predict.predict_tracks(model, cfg, tracks, smooth=True, **kw)
        assert np.array_equal(_bits(torch.cat(dflt, 0)), _bits(predict.one_euro_host(flat, lens, rate, predict.OneEuro())))
        again = predict.predict_tracks(model, cfg, tracks, smooth=None, **kw)
        assert all(_same_bits(a, b) for a, b in zip(again, raw_poses))
        with pytest.raises(ValueError, match="root filter needs camera"):
            predict.predict_tracks(model, cfg, tracks, smooth=(P, R), **kw)
