"""CPU: predict_tracks at any frame rate -- the host plans (predict.resample_plan, evaluation.keyframe_plan_at) against plain-Python
``Fraction`` loops, the new C-ABI symbol's argument checks, the ``fps`` argument checks and the command line.  Nothing needs a GPU."""
import os
import re
from fractions import Fraction
from math import ceil, floor

import numpy as np
import pytest

from tests import util

LENS = [1, 2, 13, 40]
RATES = [24, 25, 30, 60, 50, Fraction(30000, 1001), 29.97, [24, 30, 25, 60]]


def _rates(fps, n):
    from uplift_upsample_3dhpe_amd import predict
    return predict.frame_rates(fps, n)


def _plain_plan(lens, rates, model_fps=50):
    """The issue's rules, one model frame at a time, in Fractions."""
    model_lens, left, right, weight, start = [], [], [], [], 0
    for T, f in zip(lens, rates):
        Tm = ceil(Fraction(T - 1) * model_fps / f) + 1
        for k in range(Tm):
            p = Fraction(k) * f / model_fps
            l = floor(p)
            w = p - l
            if l >= T - 1:
                l, w = T - 1, Fraction(0)
            left.append(start + l)
            right.append(start + l + (1 if w > 0 else 0))
            weight.append(w.numerator / w.denominator)
        model_lens.append(Tm)
        start += T
    return model_lens, left, right, weight


def test_frame_rate_forms():
    from uplift_upsample_3dhpe_amd import predict
    assert predict.frame_rate(30) == 30 and predict.frame_rate(Fraction(30000, 1001)) == Fraction(30000, 1001)
    assert predict.frame_rate((30000, 1001)) == Fraction(30000, 1001)
    assert predict.frame_rate(29.97) == Fraction(2997, 100) and predict.frame_rate(23.976) == Fraction(2997, 125)
    assert predict.frame_rate(30000 / 1001) == Fraction(30000, 1001) and predict.frame_rate(np.float32(25.0)) == 25
    assert predict.frame_rates((30000, 1001), 3) == [Fraction(30000, 1001)] * 3           # a tuple of two integers is one rate
    assert predict.frame_rates([24, 30.0], 2) == [Fraction(24), Fraction(30)]
    for bad in (0, -25, float("nan"), float("inf"), -0.5, (30, 0), (-30, 1), "fast", None, True):
        with pytest.raises(ValueError):
            predict.frame_rate(bad)
    with pytest.raises(ValueError):
        predict.frame_rates([24, 30], 3)
    with pytest.raises(ValueError):
        predict.resample_plan(LENS, 0)
    with pytest.raises(ValueError):
        predict.resample_plan(LENS, [24, 30, float("nan"), 60])
    with pytest.raises(ValueError):
        predict.resample_plan([3, 0], 30)


@pytest.mark.parametrize("fps", RATES, ids=[str(r) for r in RATES])
def test_resample_plan_against_a_fraction_loop(fps):
    from uplift_upsample_3dhpe_amd import predict
    rates = _rates(fps, len(LENS))
    model_lens, left, right, weight = predict.resample_plan(LENS, fps)
    want = _plain_plan(LENS, rates)
    assert list(model_lens) == want[0] and list(left) == want[1] and list(right) == want[2]
    assert left.dtype == np.int64 and right.dtype == np.int64 and weight.dtype == np.float64
    assert np.array_equal(weight.view(np.uint64), np.array(want[3], np.float64).view(np.uint64))         # the same division, the same bits
    assert [int(n) for n in model_lens] == [ceil(Fraction(T - 1) * 50 / f) + 1 for T, f in zip(LENS, rates)]
    assert model_lens[0] == 1 and left[0] == right[0] == 0 and weight[0] == 0.0              # one frame in, one model frame out
    assert ((weight == 0) == (left == right)).all() and (weight >= 0).all() and (weight < 1).all()
    src_start = np.concatenate([[0], np.cumsum(LENS)])
    row = 0
    for t, (T, f, Tm) in enumerate(zip(LENS, rates, model_lens)):
        l = left[row:row + Tm] - src_start[t]
        r = right[row:row + Tm] - src_start[t]
        assert l.min() >= 0 and r.max() <= T - 1                                               # never a row of another track
        clamped = np.array([Fraction(int(k)) * f / 50 > T - 1 for k in range(Tm)])
        assert not clamped[:-1].any()                                                          # only the final model frame can be clamped
        assert l[-1] == r[-1] == T - 1
        row += Tm
    assert row == len(left)


def test_resample_plan_identity_and_integral_keyframes():
    from uplift_upsample_3dhpe_amd import predict
    model_lens, left, right, weight = predict.resample_plan(LENS, 50)
    assert list(model_lens) == LENS and np.array_equal(left, np.arange(sum(LENS))) and np.array_equal(right, left) and not weight.any()
    # 30 fps: model frame 5 m is video frame 3 m, exactly
    model_lens, left, right, weight = predict.resample_plan([40], 30)
    assert model_lens[0] == 66
    k = np.arange(0, 66, 5)
    assert np.array_equal(left[k], 3 * k // 5) and np.array_equal(right[k], left[k]) and not weight[k].any()
    assert (weight[np.arange(66) % 5 != 0] > 0).all()
    # 25 fps: model frame 2 i is video frame i; 60 fps: model frame 5 m is video frame 6 m
    _, left, right, weight = predict.resample_plan([40], 25)
    assert np.array_equal(left[::2], np.arange(40)) and not weight[::2].any() and (weight[1::2] == 0.5).all()
    _, left, right, weight = predict.resample_plan([40], 60)
    assert np.array_equal(left[::5], np.arange(0, 40, 6)) and not weight[::5].any()
    # another model rate, and output positions: fps = 20, out_fps = 60 gives 3 (T - 1) + 1 frames at thirds of a source frame
    out_lens, (track, num, den) = predict.output_positions([5, 8], 20, 60)
    assert list(out_lens) == [13, 22] and list(track) == [0] * 13 + [1] * 22
    assert [Fraction(int(a), int(b)) for a, b in zip(num[:4], den[:4])] == [Fraction(0), Fraction(5, 6), Fraction(5, 3), Fraction(5, 2)]
    out_lens, _ = predict.output_positions(LENS, Fraction(30000, 1001), Fraction(30000, 1001))
    assert list(out_lens) == LENS                                                              # out_fps = fps: one pose per given frame


def _frames(lens):
    return np.concatenate([np.arange(n) for n in lens])


@pytest.mark.parametrize("stride", [1, 2, 5])
def test_keyframe_plan_at_integral_positions_is_keyframe_plan(stride):
    from uplift_upsample_3dhpe_amd import evaluation
    lens = [1, 37, 120]
    idx = _frames(lens)
    run = np.flatnonzero(idx % stride == 0)
    rows = np.full(len(idx), -1, np.int64)
    rows[run] = np.arange(len(run))
    left, right, weight, _ = evaluation.keyframe_plan(idx, stride, rows=rows)
    track = np.repeat(np.arange(len(lens)), lens)
    for den in (1, 3):                                                                         # 7 = 7/1 = 21/3
        l, r, w = evaluation.keyframe_plan_at(idx, stride, (track, idx * den, np.full(len(idx), den)), rows=rows)
        assert np.array_equal(l, left) and np.array_equal(r, right)
        assert np.array_equal(w.view(np.uint64), weight.view(np.uint64))
    l, r, w = evaluation.keyframe_plan_at(idx, stride, (track, idx, np.ones(len(idx), np.int64)))              # without rows: positions
    l0, r0, w0, _ = evaluation.keyframe_plan(idx, stride)
    assert np.array_equal(l, l0) and np.array_equal(r, r0) and np.array_equal(w, w0)


@pytest.mark.parametrize("stride", [1, 2, 5])
def test_keyframe_plan_at_fractional_positions(stride):
    """Against two steps: interpolate_between_keyframes on the dense array, then linear between the two bracketing frames.  float64 values
    of O(1), a handful of operations on either route: 1e-12 is four orders above the rounding."""
    from uplift_upsample_3dhpe_amd import evaluation
    lens = [1, 37, 120]
    idx = _frames(lens)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    rng = np.random.default_rng(11)
    pred = rng.normal(size=(len(idx), 17, 3))
    dense, key = evaluation.interpolate_between_keyframes(pred, idx, stride)
    track, num, den = [], [], []
    for t, n in enumerate(lens):
        for d in (1, 2, 3, 7, 1001):
            k = np.arange((n - 1) * d + 1)
            track.append(np.full(len(k), t)); num.append(k); den.append(np.full(len(k), d))
    track, num, den = np.concatenate(track), np.concatenate(num), np.concatenate(den)
    l, r, w = evaluation.keyframe_plan_at(idx, stride, (track, num, den))
    assert key[l].all() and key[r].all() and ((w == 0) == (l == r)).all()
    got = pred[l] * (1.0 - w)[:, None, None] + pred[r] * w[:, None, None]
    p = num // den
    frac = (num - p * den) / den
    a = starts[track] + p
    b = np.minimum(a + 1, starts[track] + np.array(lens)[track] - 1)
    want = dense[a] * (1.0 - frac)[:, None, None] + dense[b] * frac[:, None, None]
    err = float(np.abs(got - want).max())
    print(f"stride {stride}: direct plan vs two-step interpolation max-abs {err:.3e}")
    assert (frac > 0).sum() > 1000 and err <= 1e-12
    # behind a track's last predicted frame the motion repeats it
    last_key = (np.array(lens)[track] - 1) // stride * stride
    tail = num >= last_key * den
    assert tail.any() and np.array_equal(l[tail], (starts[track] + last_key)[tail]) and np.array_equal(r[tail], l[tail]) and not w[tail].any()
    # rows: a position that needs a frame that was not forwarded is refused; a position behind the track too
    rows = np.where(key, np.arange(len(idx)), -1)
    l2, r2, w2 = evaluation.keyframe_plan_at(idx, stride, (track, num, den), rows=rows)
    assert np.array_equal(l2, l) and np.array_equal(r2, r) and np.array_equal(w2, w)
    if stride > 1:
        rows[starts[2] + stride] = -1
        with pytest.raises(ValueError, match="not forwarded"):
            evaluation.keyframe_plan_at(idx, stride, (track, num, den), rows=rows)
    with pytest.raises(ValueError, match="behind the last frame"):
        evaluation.keyframe_plan_at(idx, stride, ([1], [73], [2]))                            # 36.5 in a track of 37 frames


def test_symbol_declared_exported_and_checks_its_arguments():
    import __graft_entry__ as ge
    ge.build()
    from uplift_upsample_3dhpe_amd import _capi
    lib = _capi.load_library()
    header = open(os.path.join(util.ROOT, "include", "uu3d.h")).read()
    s = "uu3d_resample_tracks"
    assert re.search(r"\b" + s + r"\s*\(", header)
    assert s in _capi.EXPORTED_SYMBOLS and hasattr(lib, s)
    bad = _capi.UU3D_ERR_INVALID_ARGUMENT
    # refused before anything is launched (no device needed): NULL arguments, sizes below 1, the in-place form, a misaligned table
    a, b, p = 1 << 20, 2 << 20, 3 << 20                                                        # (never dereferenced)
    assert lib.uu3d_resample_tracks(None, 1, None, 1, 17, None, 1, None, None, None, None, None, None, None) == bad
    for drop in range(6):
        args = [a, b, p, p, p, p]
        args[drop] = None
        src, table, rt, le, ri, we = args
        assert lib.uu3d_resample_tracks(src, 4, table, 4, 17, rt, 1, None, le, ri, we, None, None, None) == bad, drop
    assert lib.uu3d_resample_tracks(a, 4, a, 4, 17, p, 1, None, p, p, p, None, None, None) == bad              # src == table
    assert lib.uu3d_resample_tracks(a, 0, b, 4, 17, p, 1, None, p, p, p, None, None, None) == bad
    assert lib.uu3d_resample_tracks(a, 4, b, 0, 17, p, 1, None, p, p, p, None, None, None) == bad
    assert lib.uu3d_resample_tracks(a, 4, b, 4, 0, p, 1, None, p, p, p, None, None, None) == bad
    assert lib.uu3d_resample_tracks(a, 4, b, 4, 17, p, 0, None, p, p, p, None, None, None) == bad
    assert lib.uu3d_resample_tracks(a, 4, b + 8, 4, 17, p, 1, None, p, p, p, None, None, None) == bad
    assert lib.uu3d_resample_tracks(a, 4, b, 4, 17, p, 1, None, p, p, p, p, None, None) == bad                 # valid_in without valid_out
    assert lib.uu3d_resample_tracks(a, 1 << 62, b, 4, 17, p, 1, None, p, p, p, None, None, None) == bad


class _Refuses(object):
    """A model that must not be touched: the argument checks come first."""
    has_strided_input = True

    def __getattr__(self, name):
        raise AssertionError(f"the model was used ({name}) before the arguments were checked")


def test_fps_argument_checks_come_first():
    from uplift_upsample_3dhpe_amd import predict
    cfg = util.load_config("h36m_351")
    t = [np.zeros((8, 17, 2), np.float32)]
    with pytest.raises(ValueError, match=r"fps=.*out_fps="):
        predict.predict_tracks(_Refuses(), cfg, t, fps=30, keyframes_only=True, lengths=[36])
    with pytest.raises(ValueError, match="out_fps needs fps"):
        predict.predict_tracks(_Refuses(), cfg, t, out_fps=30)
    doc = predict.predict_tracks.__doc__
    assert "fps" in doc and "limit_denominator(1001)" in doc and "MODEL's grid" in doc


def test_cli_takes_rates_as_floats_or_fractions(tmp_path, monkeypatch):
    from uplift_upsample_3dhpe_amd import predict
    torch = pytest.importorskip("torch")
    base = ["--config", "c.json", "--weights", "w.h5", "--input", "i.npz", "--output", "o.npz"]
    args = predict.parse_args(base + ["--fps", "30000/1001"])
    assert args.fps == Fraction(30000, 1001) and args.out_fps is None
    args = predict.parse_args(base + ["--fps", "29.97", "--out_fps", "60"])
    assert args.fps == Fraction(2997, 100) and args.out_fps == 60
    assert predict.parse_args(base).fps is None
    for bad in ("0", "-30", "30/0", "nan", "fast"):
        with pytest.raises(SystemExit):
            predict.parse_args(base + ["--fps", bad])
    # through main: the rates reach predict_tracks, and the output has the frames predict_tracks returns
    inp, outp = str(tmp_path / "tracks.npz"), str(tmp_path / "out.npz")
    np.savez(inp, walk=np.zeros((7, 17, 2), np.float32))
    seen = {}

    def fake_predict(model, config, trs, **kw):
        seen["kw"] = kw
        return [torch.zeros((19, 17, 3), dtype=torch.float32)]
    monkeypatch.setattr(predict, "_load_model", lambda config, weights: object())
    monkeypatch.setattr(predict, "predict_tracks", fake_predict)
    cfg = os.path.join(util.ROOT, "config", "h36m_351.json")
    assert predict.main(["--config", cfg, "--weights", "w.h5", "--input", inp, "--output", outp, "--fps", "20", "--out_fps", "60"]) == 0
    assert seen["kw"]["fps"] == 20 and seen["kw"]["out_fps"] == 60
    with np.load(outp) as z:
        assert z["walk"].shape == (19, 17, 3)
    assert predict.main(["--config", cfg, "--weights", "w.h5", "--input", inp, "--output", outp, "--fps", "30000/1001"]) == 0
    assert seen["kw"]["fps"] == Fraction(30000, 1001) and "out_fps" not in seen["kw"]
    with pytest.raises(SystemExit):
        predict.main(["--config", cfg, "--weights", "w.h5", "--input", inp, "--output", outp, "--out_fps", "60"])
