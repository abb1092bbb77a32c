"""CPU: steady output (include/uu3d.h, STEADY OUTPUT; predict.OneEuro / one_euro_host, stream.LiveOneEuroHost) -- the arguments, the
refusals that need no device, the command lines, the properties of the rule in numpy, and the live state machine against the offline rule."""
import types

import numpy as np
import pytest

from tests import util

CAMERA = (1145.0, 1143.5, 512.25, 515.75)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def noisy(rows, channels, seed):
    """A slow motion with noise on it, float32: every channel moves, so beta matters."""
    rng = np.random.default_rng(seed)
    t = np.arange(rows, dtype=np.float64)[:, None]
    return (np.sin(t * rng.uniform(0.02, 0.2, channels) + rng.uniform(0, 6, channels)) + 0.05 * rng.normal(size=(rows, channels))).astype(np.float32)


def test_one_euro_validation():
    from uplift_upsample_3dhpe_amd import predict
    f = predict.OneEuro()
    assert tuple(f) == (1.0, 0.5, 1.0) and f == predict.OneEuro(1, 0.5, 1) and "min_cutoff=1.0" in repr(f)
    assert tuple(predict.OneEuro(0.25, 0, 3)) == (0.25, 0.0, 3.0)
    for bad in ((0, 0.5, 1), (-1, 0.5, 1), (1, -0.1, 1), (1, 0.5, 0), (1, 0.5, -2), (float("nan"), 0.5, 1), (1, float("inf"), 1),
                (1, 0.5, float("nan")), ("x", 0.5, 1), (None, 0.5, 1)):
        with pytest.raises(ValueError, match="OneEuro"):
            predict.OneEuro(*bad)


def test_smooth_forms():
    from uplift_upsample_3dhpe_amd import predict
    F, R = predict.OneEuro(2.0, 0.1, 1.5), predict.OneEuro(0.5, 0.0, 1.0)
    assert predict.check_smooth(None, True) == (None, None) and predict.check_smooth(None, False) == (None, None)
    assert predict.check_smooth(True, True) == (predict.OneEuro(), predict.OneEuro())
    assert predict.check_smooth(True, False) == (predict.OneEuro(), None)
    assert predict.check_smooth(F, True) == (F, F) and predict.check_smooth(F, False) == (F, None)
    assert predict.check_smooth((F, R), True) == (F, R) and predict.check_smooth([None, R], True) == (None, R)
    assert predict.check_smooth((F, None), False) == (F, None) and predict.check_smooth((None, None), False) == (None, None)
    for pair in ((F, R), (None, R)):
        with pytest.raises(ValueError, match="root filter needs camera"):
            predict.check_smooth(pair, False)
    for bad in (1.0, "yes", (F,), (F, R, R), (1.0, 0.5), {"min_cutoff": 1}):
        with pytest.raises(ValueError, match="smooth must be"):
            predict.check_smooth(bad, True)


def test_predict_tracks_refuses_before_any_device():
    from uplift_upsample_3dhpe_amd import predict
    cfg = util.load_config("h36m_81")
    tracks = [np.zeros((4, 17, 2), np.float32)]
    with pytest.raises(ValueError, match="root filter needs camera"):
        predict.predict_tracks(None, cfg, tracks, smooth=(None, predict.OneEuro()))
    with pytest.raises(ValueError, match="smooth must be"):
        predict.predict_tracks(None, cfg, tracks, smooth=3)


def _stub_model():
    return types.SimpleNamespace(arch=types.SimpleNamespace(compiled_dims=True), device="cpu", has_strided_input=True)


def test_session_refusals_need_no_device():
    from uplift_upsample_3dhpe_amd import predict, stream
    cfg = util.load_config("h36m_81")
    F = predict.OneEuro(2.0, 0.1, 1.5)

    def plan(fps=None, out_fps=None, lookahead=5, **kw):
        s = object.__new__(stream.StreamSession)
        s._init_plan(_stub_model(), cfg, 3, (1920, 1080), 4, True, lookahead, True, False, fps, 50, out_fps, **kw)
        return s

    with pytest.raises(ValueError, match="smooth together with out_fps is not supported.*out of scope"):
        plan(fps=10, out_fps=50, lookahead=40, smooth=F)
    with pytest.raises(ValueError, match="smooth together with out_fps"):
        stream.StreamSession(_stub_model(), cfg, slots=2, mask_stride=4, lookahead=40, fps=10, out_fps=50, smooth=True)
    with pytest.raises(ValueError, match="root filter needs camera"):
        plan(smooth=(None, F))
    with pytest.raises(ValueError, match="smooth must be"):
        plan(smooth=0.5)
    with pytest.raises(TypeError, match="unexpected keyword argument 'smoothing'"):
        stream.StreamSession(_stub_model(), cfg, slots=2, mask_stride=4, smoothing=F)
    s = plan()
    assert s.pose_filter is None and s.root_filter is None
    s = plan(smooth=F)
    assert s.pose_filter == F and s.root_filter is None and float(s.smooth_rate) == 50.0
    s = plan(smooth=True, camera=CAMERA)
    assert s.pose_filter == predict.OneEuro() and s.root_filter == predict.OneEuro()
    s = plan(smooth=(None, F), camera=CAMERA, fps=30, lookahead=40)
    assert s.pose_filter is None and s.root_filter == F and float(s.smooth_rate) == 30.0
    assert float(plan(smooth=F, fps=29.97, lookahead=40).smooth_rate) == 29.97
    assert plan(smooth=F, detections=3, camera=CAMERA).root_filter == F
    for bad in (dict(slots=0, channels=3), dict(slots=2, channels=0), dict(slots=2, channels=(1 << 16) + 1), dict(slots=2, channels=3, lookahead=-1),
                dict(slots=2, channels=3, filt=(1.0, 0.5, 1.0)), dict(slots=2, channels=3, rate=0)):
        kw = dict(rate=50, filt=F, lookahead=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            stream.LiveOneEuroHost(**kw)


def test_command_lines(tmp_path, monkeypatch):
    from uplift_upsample_3dhpe_amd import predict, stream
    base = ["--config", "c.json", "--weights", "w.h5", "--input", "i.npz", "--output", "o.npz"]
    cam = ["--camera", "1145", "1143.5", "512.25", "515.75"]
    for mod in (predict, stream):
        a = mod.parse_args(base)
        assert a.smooth is None and a.smooth_root is None and predict.smooth_option(a) == {}
        a = mod.parse_args(base + ["--smooth", "2", "0.1", "1.5"])
        assert predict.smooth_option(a) == {"smooth": (predict.OneEuro(2.0, 0.1, 1.5), None)}
        a = mod.parse_args(base + cam + ["--smooth_root", "0.5", "0", "1"])
        assert predict.smooth_option(a) == {"smooth": (None, predict.OneEuro(0.5, 0.0, 1.0))}
        a = mod.parse_args(base + cam + ["--smooth", "2", "0.1", "1.5", "--smooth_root", "0.5", "0", "1"])
        assert predict.smooth_option(a) == {"smooth": (predict.OneEuro(2.0, 0.1, 1.5), predict.OneEuro(0.5, 0.0, 1.0))}
        for bad in (["--smooth_root", "0.5", "0", "1"], ["--smooth", "1", "2"], ["--smooth", "a", "b", "c"]):
            with pytest.raises(SystemExit):
                mod.parse_args(base + bad)
        with pytest.raises(SystemExit, match="--smooth / --smooth_root: OneEuro needs"):
            predict.smooth_option(mod.parse_args(base + ["--smooth", "0", "0.1", "1.5"]))
    with pytest.raises(SystemExit):
        stream.parse_args(base + ["--smooth", "2", "0.1", "1.5", "--fps", "10", "--out_fps", "50"])
    # stream.main hands the pair on
    cfg = util.ROOT + "/config/h36m_81.json"
    inp, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, walk=np.random.default_rng(0).normal(size=(6, 17, 2)).astype(np.float32))
    monkeypatch.setattr(stream, "_load_model", lambda config, weights: "model")
    seen = {}

    def fake_replay(model, config, tracks, **kw):
        seen["kw"] = kw
        return [np.zeros((len(t), 17, 3), np.float32) for t in tracks], [np.ones(len(t), bool) for t in tracks]
    monkeypatch.setattr(stream, "replay_tracks", fake_replay)
    args = ["--config", cfg, "--weights", "none.h5", "--input", inp, "--output", out]
    assert stream.main(args) == 0 and "smooth" not in seen["kw"]
    assert stream.main(args + ["--smooth", "2", "0.1", "1.5"]) == 0
    assert seen["kw"]["smooth"] == (predict.OneEuro(2.0, 0.1, 1.5), None)
    with pytest.raises(SystemExit, match="--smooth / --smooth_root"):
        stream.main(args + ["--smooth", "2", "-1", "1.5"])


def test_c_abi_declared_and_refusing():
    import ctypes as C
    import __graft_entry__ as ge
    ge.build()
    from uplift_upsample_3dhpe_amd import _capi
    lib = _capi.load_library()
    header = open(util.ROOT + "/include/uu3d.h").read()
    assert "STEADY OUTPUT" in header
    for s in ("uu3d_one_euro_tracks", "uu3d_stream_one_euro_bytes", "uu3d_stream_one_euro", "uu3d_stream_one_euro_reset"):
        assert s in _capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    n = lib.uu3d_stream_one_euro_bytes(5, 51)
    assert n >= 5 * 51 * (8 + 8 + 4 + 1) and n % 256 == 0
    assert lib.uu3d_stream_one_euro_bytes(0, 51) == 0 and lib.uu3d_stream_one_euro_bytes(1, 0) == 0 and lib.uu3d_stream_one_euro_bytes(1, (1 << 16) + 1) == 0
    block = C.c_void_p(256)                                           # (aligned addresses that are never dereferenced: the calls refuse first)
    other = C.c_void_p(512)
    BAD, UNS = _capi.UU3D_ERR_INVALID_ARGUMENT, _capi.UU3D_ERR_UNSUPPORTED
    assert lib.uu3d_stream_one_euro_reset(1, (1 << 16) + 1, block, None, None) == UNS
    assert lib.uu3d_stream_one_euro_reset(1, 51, None, None, None) == BAD
    assert lib.uu3d_stream_one_euro_reset(0, 51, block, None, None) == BAD
    live = lambda C_, rate, mc, beta, dc, state=block: lib.uu3d_stream_one_euro(1, C_, 0, state, block, block, block, block, None, rate, mc, beta, dc, other, None)
    assert live((1 << 16) + 1, 50.0, 1.0, 0.5, 1.0) == UNS
    for args in ((51, 0.0, 1.0, 0.5, 1.0), (51, float("nan"), 1.0, 0.5, 1.0), (51, 50.0, 0.0, 0.5, 1.0), (51, 50.0, 1.0, -0.5, 1.0),
                 (51, 50.0, 1.0, 0.5, 0.0), (51, 50.0, 1.0, float("inf"), 1.0), (0, 50.0, 1.0, 0.5, 1.0)):
        assert live(*args) == BAD, args
    assert live(51, 50.0, 1.0, 0.5, 1.0, state=None) == BAD
    assert lib.uu3d_stream_one_euro(1, 51, 0, block, block, block, block, block, None, 50.0, 1.0, 0.5, 1.0, block, None) == BAD     # out is values
    off = lambda C_, mc, rows=4, out=other: lib.uu3d_one_euro_tracks(block, out, rows, C_, block, block, block, 1, None, mc, 0.5, 1.0, None)
    assert off((1 << 16) + 1, 1.0) == UNS
    assert off(51, 0.0) == BAD and off(51, float("nan")) == BAD and off(0, 1.0) == BAD and off(51, 1.0, rows=-1) == BAD
    assert off(51, 1.0, out=block) == BAD                             # out may not alias in
    assert off(51, 1.0, rows=0) == _capi.UU3D_OK                      # nothing to do, nothing launched


# ---- the rule in numpy -------------------------------------------------------------------------------------------------------------------
FILTERS = [(1.0, 0.5, 1.0), (0.3, 0.0, 2.0), (4.0, 3.0, 0.5)]


@pytest.mark.parametrize("params", FILTERS)
def test_host_rule_first_sample_constants_and_zeros(params):
    from uplift_upsample_3dhpe_amd import predict
    F = predict.OneEuro(*params)
    x = noisy(40, 6, seed=1)
    x[:, 1] = np.float32(0.1)                                         # a constant that is no dyadic number
    x[:, 2] = 0.0
    x[:, 3] = -0.0
    x[:, 4] = np.float32(-1234.5678)
    lens = [1, 2, 37]
    y = predict.one_euro_host(x, lens, 50, F)
    assert y.dtype == np.float32 and y.shape == x.shape
    for first in (0, 1, 3):                                           # the first sample of every track is returned as given
        assert np.array_equal(bits(y[first]), bits(x[first]))
    for c in (1, 2, 4):                                               # a constant channel comes back bit-identical, zeros stay zeros
        assert np.array_equal(bits(y[:, c]), bits(x[:, c])), c
    assert not y[:, 3].any()
    assert not np.array_equal(bits(y[:, 0]), bits(x[:, 0]))           # (and the filter does something to a channel that moves)
    # any trailing shape is C channels; one track without lens
    z = predict.one_euro_host(x.reshape(40, 2, 3), None, 50, F)
    assert z.shape == (40, 2, 3) and np.array_equal(bits(z[:1]), bits(x[:1].reshape(1, 2, 3)))
    # the scalar recursion, written out once more in Python floats (IEEE doubles): channel 0 of the last track
    r, (mc, beta, dc) = 50.0, params
    alpha = lambda fc: 1.0 / (1.0 + r / (6.283185307179586 * fc))
    xh, dxh, want = float(x[3, 0]), 0.0, [x[3, 0]]
    for v in x[4:, 0]:
        v = float(v)
        dx = (v - xh) * r
        ad = alpha(dc)
        dxh = ad * dx + (1.0 - ad) * dxh
        a = alpha(mc + beta * abs(dxh))
        xh = a * v + (1.0 - a) * xh
        want.append(np.float32(xh))
    assert np.array_equal(bits(y[3:, 0]), bits(np.array(want, np.float32)))


@pytest.mark.parametrize("params", FILTERS)
def test_host_rule_step_response_is_monotone_and_bounded(params):
    from uplift_upsample_3dhpe_amd import predict
    F = predict.OneEuro(*params)
    lo, hi = np.float32(0.25), np.float32(1.75)
    x = np.full((80, 2), lo, np.float32)
    x[10:, 0] = hi                                                    # a step up ...
    x[:10, 1], x[10:, 1] = hi, lo                                     # ... and a step down
    y = predict.one_euro_host(x, None, 50, F).astype(np.float64)
    assert (y[:10, 0] == lo).all() and (y[:10, 1] == hi).all()
    up, down = y[9:, 0], y[9:, 1]
    assert (np.diff(up) >= 0).all() and (np.diff(down) <= 0).all()
    assert (up >= lo).all() and (up <= hi).all() and (down >= lo).all() and (down <= hi).all()
    assert up[1] > lo and down[1] < hi                                # it does move at the step


def test_host_rule_nan_and_state_rows_are_passed_through():
    from uplift_upsample_3dhpe_amd import predict
    F = predict.OneEuro(1.0, 0.5, 1.0)
    x = noisy(30, 4, seed=2)
    # a NaN sample is passed through and leaves the samples after it as if it had not been there: the same channel with the sample cut
    # out, at a rate that makes up for the gap -- offline n is always 1, so "as if it had not been there" means the row is skipped
    bad = x.copy()
    bad[7, 2] = np.nan
    bad[12, 1] = np.inf
    y = predict.one_euro_host(bad, None, 50, F)
    assert np.isnan(y[7, 2]) and np.isposinf(y[12, 1])
    cut2 = predict.one_euro_host(np.delete(x[:, 2:3], 7, axis=0), None, 50, F)
    assert np.array_equal(bits(np.delete(y[:, 2], 7)), bits(cut2[:, 0]))
    cut1 = predict.one_euro_host(np.delete(x[:, 1:2], 12, axis=0), None, 50, F)
    assert np.array_equal(bits(np.delete(y[:, 1], 12)), bits(cut1[:, 0]))
    clean = predict.one_euro_host(x, None, 50, F)
    assert np.array_equal(bits(y[:, [0, 3]]), bits(clean[:, [0, 3]]))  # the other channels never notice
    # a state == 0 row is passed through without a sample: at the start, in the middle, and a whole track
    lens = [12, 5, 13]
    state = np.ones(30, np.uint8)
    state[[0, 1, 6, 7]] = 0
    state[12:17] = 0
    marked = x.copy()
    marked[state == 0] = 0.0                                          # (a root of state 0 is zeros)
    y = predict.one_euro_host(marked, lens, 50, F, state=state)
    assert not y[state == 0].any()
    keep = state[:12] != 0
    assert np.array_equal(bits(y[:12][keep]), bits(predict.one_euro_host(x[:12][keep], None, 50, F)))
    assert np.array_equal(bits(y[17:]), bits(clean_tail := predict.one_euro_host(x[17:], None, 50, F))) and clean_tail.shape == (13, 4)
    with pytest.raises(ValueError, match="lens must add up"):
        predict.one_euro_host(x, [10, 10], 50, F)
    with pytest.raises(ValueError, match="state must be"):
        predict.one_euro_host(x, None, 50, F, state=np.ones(29))
    with pytest.raises(ValueError, match="one rate or one per track"):
        predict.one_euro_host(x, lens, [50, 30], F)


# ---- the live state machine against the offline rule ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lookahead", [0, 3])
def test_live_host_equals_offline_rule_with_every_slot_fresh(lookahead):
    from uplift_upsample_3dhpe_amd import predict, stream
    F = predict.OneEuro(1.5, 0.7, 1.0)
    T, C, ticks = 3, 6, 25
    x = noisy(ticks * T, C, seed=3).reshape(ticks, T, C)
    live = stream.LiveOneEuroHost(T, C, (2997, 100), F, lookahead)
    got = np.stack([live.step(x[k], np.full(T, k + 1), np.ones(T), None) for k in range(ticks)])
    for i in range(T):
        assert np.array_equal(bits(got[:, i]), bits(predict.one_euro_host(x[:, i], None, 29.97, F))), i


def test_live_host_n_rule_inactive_slots_and_reset():
    """Slot i is fresh at every (i + 1)-th tick only: its samples are the fresh values at rate / (i + 1).  In between it returns its last
    output; an inactive slot takes no sample even when fresh; a reset of one slot restarts only that slot."""
    from uplift_upsample_3dhpe_amd import predict, stream
    F = predict.OneEuro(1.0, 0.5, 1.0)
    T, C, ticks = 3, 5, 36
    x = noisy(ticks * T, C, seed=4).reshape(ticks, T, C)
    live = stream.LiveOneEuroHost(T, C, 50, F, 2)
    fresh = np.array([[k % (i + 1) == 0 for i in range(T)] for k in range(ticks)])
    got = np.stack([live.step(x[k], np.full(T, k + 1), fresh[k]) for k in range(ticks)])
    for i in range(T):
        want = predict.one_euro_host(x[fresh[:, i], i], None, (50, i + 1), F)
        assert np.array_equal(bits(got[fresh[:, i], i]), bits(want)), i
        held = np.maximum.accumulate(np.where(fresh[:, i], np.arange(ticks), 0))       # the last fresh tick at or before each tick
        assert np.array_equal(bits(got[:, i]), bits(got[held, i])), i
    # before the first sample: zeros; an inactive slot takes none; state 0 passes the row through and takes none either
    live = stream.LiveOneEuroHost(T, C, 50, F, 0)
    assert not live.step(x[0], np.zeros(T), np.zeros(T)).any()
    out = live.step(x[0], np.ones(T), np.ones(T), active=[1, 0, 1], state=[1, 1, 0])
    assert np.array_equal(bits(out[0]), bits(x[0, 0])) and not out[1].any() and np.array_equal(bits(out[2]), bits(x[0, 2]))
    assert live.taken[0].all() and not live.taken[1].any() and not live.taken[2].any()
    # reset of one slot: that slot starts again with its next sample, the others go on
    a, b = stream.LiveOneEuroHost(T, C, 50, F, 0), stream.LiveOneEuroHost(T, C, 50, F, 0)
    for k in range(10):
        a.step(x[k], np.full(T, k + 1), np.ones(T))
        b.step(x[k], np.full(T, k + 1), np.ones(T))
    a.reset([1])
    assert not a.step(x[10], np.full(T, 10), np.zeros(T))[1].any()   # (not fresh: nothing to return yet)
    ya, yb = a.step(x[10], np.full(T, 11), np.ones(T)), b.step(x[10], np.full(T, 11), np.ones(T))
    assert np.array_equal(bits(ya[1]), bits(x[10, 1])) and not np.array_equal(bits(yb[1]), bits(x[10, 1]))
    assert np.array_equal(bits(ya[[0, 2]]), bits(yb[[0, 2]]))
    # a counter that does not advance (n < 1) counts as one frame
    c = stream.LiveOneEuroHost(1, C, 50, F, 0)
    c.step(x[0, :1], [5], [1])
    again = c.step(x[1, :1], [5], [1])
    assert np.array_equal(bits(again), bits(predict.one_euro_host(x[:2, 0], None, 50, F)[1:]))
