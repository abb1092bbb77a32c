"""No GPU: the host planning of stream.StreamSession(fps=F, out_fps=G) -- rate_plan with an output rate and out_push_plan, the host mirror of
what a push returns -- simulated push by push with push_plan and out_push_plan only, against predict.output_positions,
evaluation.keyframe_plan_at and brute force in Fractions; the refusals; the command line; the C ABI of the new launches."""
import ctypes as C
import inspect
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import util

PAIRS = [(10, 50), (30, 60), (25, 30), (30, 24), (29.97, 50), (24, 24)]
CASES = [(name, ms) for name in ("h36m_81", "h36m_351") for ms in util.load_config(name).MASK_STRIDE]


def _rates(fps, out_fps):
    from uplift_upsample_3dhpe_amd import predict
    return predict.frame_rate(fps), predict.frame_rate(out_fps)


def _period(fps, out_fps, P):
    """Source frames in one common period of source frames, output frames and keyframes, by its definition: the smallest time that is a
    whole number of each of the three steps."""
    F, G = _rates(fps, out_fps)
    steps = (1 / F, 1 / G, Fraction(P, 50))
    t = Fraction(math.lcm(*(s.numerator for s in steps)), math.gcd(*(s.denominator for s in steps)))
    assert all((t / s).denominator == 1 for s in steps)
    return int(t * F)


def _simulate(cfg, ms, fps, out_fps, extra):
    """Pushes j = 0 .. over two periods plus the lookahead -> (plan, pushes, [(j, i, k0, k1, weight)] in the order emitted, per-push counts,
    the deepest ring place any read needed).  The sub-ticks of push_plan emit keyframes into a ring of plan.D places, tracked by what each
    place holds; every read of out_push_plan is checked against it."""
    from uplift_upsample_3dhpe_amd import stream
    lo = stream.rate_plan(cfg, fps, None, ms, out_fps=out_fps).min_lookahead
    plan = stream.rate_plan(cfg, fps, lo + extra, ms, out_fps=out_fps)
    P, L = plan.pred_stride, plan.lookahead
    n = 2 * _period(fps, out_fps, P) + L + 7
    ring, emitted, newest = {}, set(), None
    out, counts, deepest = [], [], 0
    for j in range(n):
        for k, _, _, _ in stream.push_plan(j, plan)["model"]:
            c = k - plan.a_m
            if c >= 0 and c % P == 0:                                     # the sub-tick of model frame k emits keyframe c
                emitted.add(c)
                ring[(c // P) % plan.D] = c
                newest = c
        frames = stream.out_push_plan(j, plan)
        counts.append(len(frames))
        for i, k0, k1, w in frames:
            assert k0 in emitted and k1 in emitted, (j, i, k0, k1)       # emitted by a sub-tick of this push or an earlier one
            assert ring[(k0 // P) % plan.D] == k0 and ring[(k1 // P) % plan.D] == k1, (j, i, k0, k1)
            deepest = max(deepest, (newest - k0) // P + 1)
            out.append((j, i, k0, k1, w))
    return plan, n, out, counts, deepest


@pytest.mark.parametrize("cfgname,ms", CASES)
@pytest.mark.parametrize("fps,out_fps", PAIRS)
@pytest.mark.parametrize("extra", [0, 3])
def test_every_due_frame_once_in_order_from_kept_keyframes(cfgname, ms, fps, out_fps, extra):
    from uplift_upsample_3dhpe_amd import evaluation, predict, stream
    cfg = util.load_config(cfgname)
    plan, n, out, counts, deepest = _simulate(cfg, ms, fps, out_fps, extra)
    F, G = _rates(fps, out_fps)
    L, P, R = plan.lookahead, plan.pred_stride, plan.max_out
    assert (Fraction(plan.out_c, plan.out_d), Fraction(plan.pos_num, plan.pos_den), R) == (G / F, Fraction(50) / G, math.ceil(G / F))
    assert math.gcd(plan.out_c, plan.out_d) == 1 and math.gcd(plan.pos_num, plan.pos_den) == 1
    # after m pushes the frames emitted are exactly 0 .. floor((m - 1 - L) G / F), each once, in order
    assert [o[1] for o in out] == list(range(math.floor((n - 1 - L) * G / F) + 1))
    done = np.cumsum(counts)
    for m in range(1, n + 1):
        assert done[m - 1] == (0 if m - 1 - L < 0 else math.floor((m - 1 - L) * G / F) + 1), m
    assert counts[L] == 1 and counts[L + 1:] == [math.floor((j - L) * G / F) - math.floor((j - 1 - L) * G / F) for j in range(L + 1, n)]
    assert not any(counts[:L]) and max(counts) == R                      # no push exceeds R, some push reaches it
    if (fps, out_fps) == (30, 24):
        assert 0 in counts[L:]
    # the total is predict.output_positions' for a track of n - L frames, and the weights are keyframe_plan_at's bits
    out_lens, (track, num, den) = predict.output_positions([n - L], fps, out_fps)
    assert out_lens[0] == len(out) and not track.any()
    frames = np.arange(int(num[-1] // den[-1]) + 2 * P + 1)
    left, right, weight = evaluation.keyframe_plan_at(frames, P, (track, num, den))
    assert np.array_equal(left, [o[2] for o in out]) and np.array_equal(right, [o[3] for o in out])
    assert np.array_equal(weight.view(np.uint64), np.array([o[4] for o in out], np.float64).view(np.uint64))
    for _, i, k0, k1, w in out[:400]:
        u = i * Fraction(50) / G
        assert k0 % P == 0 and k0 <= u < k0 + P and k1 == (k0 if u == k0 else k0 + P)
        assert w == float(np.float64(i * plan.pos_num - k0 * plan.pos_den) / np.float64(P * plan.pos_den))
    # D is exactly as deep as the reads need, and the input side is the fps-only session's
    assert deepest == plan.D
    base = stream.rate_plan(cfg, fps, L, ms)
    assert (plan.A, plan.B, plan.n_max, plan.a_m, plan.min_lookahead, plan.pred_stride, plan.lookahead) == \
        (base.A, base.B, base.n_max, base.a_m, base.min_lookahead, base.pred_stride, base.lookahead)


@pytest.mark.parametrize("cfgname,ms", CASES)
@pytest.mark.parametrize("fps", [24, 30, 29.97])
def test_equal_rates_return_the_source_frames_pose(cfgname, ms, fps):
    """out_fps == fps: every push past the lookahead returns one frame, push_plan's q with its k0, k1 and weight (bits), and the ring is
    the fps-only session's."""
    from uplift_upsample_3dhpe_amd import stream
    cfg = util.load_config(cfgname)
    lo = stream.rate_plan(cfg, fps, None, ms).min_lookahead
    for L in (lo, lo + 5):
        plan, base = stream.rate_plan(cfg, fps, L, ms, out_fps=fps), stream.rate_plan(cfg, fps, L, ms)
        assert plan[:8] == base[:8] and (plan.out_c, plan.out_d, plan.max_out) == (1, 1, 1) and (plan.pos_num, plan.pos_den) == (plan.A, plan.B)
        for j in range(L + 700):
            pp, frames = stream.push_plan(j, plan), stream.out_push_plan(j, plan)
            if j < L:
                assert frames == [] and pp["q"] is None
            else:
                assert len(frames) == 1 and frames[0][:3] == (pp["q"], pp["k0"], pp["k1"])
                assert np.float64(frames[0][3]).view(np.uint64) == np.float64(pp["weight"]).view(np.uint64)


def _brute(cfg, ms, fps, lookahead, periods=3):
    """a_m, D and the smallest lookahead of the fps-only session by the definitions, in Fractions, over `periods` periods of j."""
    from uplift_upsample_3dhpe_amd import predict, stream
    _, _, P = stream.session_strides(cfg, ms)
    rho = Fraction(50) / predict.frame_rate(fps)
    span = periods * rho.denominator * P

    def keys(q):
        u = q * rho
        k0 = math.floor(u / P) * P
        return k0, (k0 if u == k0 else k0 + P)

    def slack(L):
        return min(math.floor(j * rho) - keys(j - L)[1] for j in range(L, L + span))
    lo = next(L for L in range(10 ** 6) if slack(L) >= 0)
    a_m = min(stream.max_lookahead(cfg), slack(lookahead))
    D = 1 + max(((math.floor(j * rho) - a_m) // P * P - keys(j - lookahead)[0]) // P for j in range(lookahead, lookahead + span))
    return a_m, D, lo


@pytest.mark.parametrize("cfgname,ms", CASES)
@pytest.mark.parametrize("fps", [10, 25, 30, 24])
def test_without_an_output_rate_the_plan_is_what_it_was(cfgname, ms, fps):
    from uplift_upsample_3dhpe_amd import predict, stream
    cfg = util.load_config(cfgname)
    _, _, P = stream.session_strides(cfg, ms)
    rho = Fraction(50) / predict.frame_rate(fps)
    lo = stream.rate_plan(cfg, fps, None, ms).min_lookahead
    for la in (lo, lo + 4, 300):
        plan = stream.rate_plan(cfg, fps, la, ms, 50, None)
        a_m, D, lo_b = _brute(cfg, ms, fps, la)
        assert plan._fields[:8] == ("A", "B", "n_max", "a_m", "D", "min_lookahead", "pred_stride", "lookahead")
        assert tuple(plan[:8]) == (rho.numerator, rho.denominator, math.ceil(rho), a_m, D, lo_b, P, la)
        assert tuple(plan[8:]) == (None,) * 5 and plan._fields[8:] == ("out_c", "out_d", "pos_num", "pos_den", "max_out")
        assert plan == stream.rate_plan(cfg, fps, la, ms) == stream.RatePlan(*plan[:8])
        with pytest.raises(ValueError, match="no output rate"):
            stream.out_push_plan(la, plan)


def test_refusals_name_the_quantity():
    from uplift_upsample_3dhpe_amd import stream
    cfg = util.load_config("h36m_81")
    with pytest.raises(ValueError, match=r"source frames per period"):
        stream.rate_plan(cfg, (1000003, 20), None, out_fps=(1000003, 1940))     # G / F = 1/97, model_fps / F = 1000/1000003
    with pytest.raises(ValueError, match=r"out_fps / fps = 3000009/7007"):
        stream.rate_plan(cfg, (7, 3), None, out_fps=(1000003, 1001))
    with pytest.raises(ValueError, match=r"model_fps / out_fps = 1052651/1\b"):
        stream.rate_plan(cfg, (50, 1021), None, out_fps=(50, 1021 * 1031))
    with pytest.raises(ValueError, match=r"100 poses per push"):
        stream.rate_plan(cfg, 1, None, out_fps=100)
    assert stream.rate_plan(cfg, 1, None, out_fps=64).max_out == 64      # (the bound itself is fine)
    for bad in (0, -5, float("nan"), "x"):
        with pytest.raises(ValueError):
            stream.rate_plan(cfg, 30, None, out_fps=bad)
    stub = type("M", (), {"arch": type("A", (), {"compiled_dims": True})(), "device": "cpu", "has_strided_input": True})()
    with pytest.raises(ValueError, match="out_fps needs fps"):           # as predict_tracks; refused before anything touches a device
        stream.StreamSession(stub, cfg, slots=2, out_fps=50)
    with pytest.raises(ValueError, match=r"poses per push"):
        stream.StreamSession(stub, cfg, slots=2, lookahead=100, fps=1, out_fps=100)


def test_a_long_period_is_enumerated_in_numpy():
    """29.97 fps in, 50 out: 2997 source frames per period; 30000/1001 in, 60 out: 3000.  The plan comes from one vectorised pass."""
    from uplift_upsample_3dhpe_amd import rates, stream
    cfg = util.load_config("h36m_351")
    assert _period(29.97, 50, 5) == 2997 and _period((30000, 1001), 60, 5) == 3000
    plan = stream.rate_plan(cfg, (30000, 1001), None, 5, out_fps=60)
    assert (plan.out_c, plan.out_d, plan.max_out) == (1001, 500, 3) and plan.D >= 2
    src = inspect.getsource(rates._output_ring_depth)
    assert "np.arange" in src and "for " not in src.split('"""')[2]


def test_command_line_and_signatures():
    from uplift_upsample_3dhpe_amd import stream
    base = ["--config", "c.json", "--weights", "w.h5", "--input", "i.npz", "--output", "o.npz"]
    assert stream.parse_args(base + ["--fps", "10"]).out_fps is None
    assert stream.parse_args(base + ["--fps", "10", "--out_fps", "50"]).out_fps == Fraction(50)
    assert stream.parse_args(base + ["--fps", "30", "--out_fps", "24000/1001"]).out_fps == Fraction(24000, 1001)
    assert stream.parse_args(base + ["--fps", "30", "--out_fps", "29.97"]).out_fps == Fraction(2997, 100)
    for bad in (["--out_fps", "50"], ["--fps", "10", "--out_fps", "0"]):
        with pytest.raises(SystemExit):
            stream.parse_args(base + bad)
    for fn in (stream.StreamSession.__init__, stream.replay_tracks, stream.rate_plan):
        assert inspect.signature(fn).parameters["out_fps"].default is None
    assert isinstance(stream.StreamSession.out_frames, property)
    bench = open(os.path.join(util.ROOT, "tools", "stream_bench.py")).read()
    assert '"--out_fps"' in bench


SYMBOLS = ("uu3d_stream_out_state_layout", "uu3d_stream_timed_emit_multi", "uu3d_stream_out_reset")


def test_symbols_declared_exported_and_refusing():
    import __graft_entry__ as ge
    ge.build()
    from uplift_upsample_3dhpe_amd import _capi
    lib = _capi.load_library()
    header = open(os.path.join(util.ROOT, "include", "uu3d.h")).read()
    assert "LIVE TRACKS AT ANY FRAME RATE" in header
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", header), s
        assert s in _capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert C.sizeof(_capi.Uu3dStreamOut) == 20 and C.sizeof(_capi.Uu3dStreamOutLayout) == 16
    assert [f for f, _ in _capi.Uu3dStreamOut._fields_] == re.sub(r"/\*.*?\*/", "", re.search(
        r"typedef struct uu3d_stream_out \{ int32_t ([^;]*);", header).group(1)).replace(" ", "").split(",")
    assert [f for f, _ in _capi.Uu3dStreamOutLayout._fields_] == re.search(
        r"typedef struct uu3d_stream_out_layout \{\s*int64_t ([^;]*);", header).group(1).replace(" ", "").split(",")
    # the structs of the session without an output rate are untouched; arguments are refused before anything is launched (no device needed)
    assert C.sizeof(_capi.Uu3dStreamRate) == 16 and C.sizeof(_capi.Uu3dStreamRateLayout) == 64
    bad = _capi.UU3D_ERR_INVALID_ARGUMENT
    cfg, rate = _capi.Uu3dStreamConfig(3, 5, 5, 5, 0, 1, 1, 6), _capi.Uu3dStreamRate(5, 1, 4, 2)
    outp, lay = _capi.Uu3dStreamOut(5, 1, 1, 1, 5), _capi.Uu3dStreamOutLayout()
    assert lib.uu3d_stream_out_state_layout(None, C.byref(cfg), C.byref(rate), C.byref(outp), C.byref(lay)) == bad
    assert lib.uu3d_stream_timed_emit_multi(None, C.byref(cfg), C.byref(rate), C.byref(outp), None, None, None, None) == bad
    assert lib.uu3d_stream_out_reset(None, C.byref(cfg), C.byref(rate), C.byref(outp), None, None, None) == bad


def test_source_has_one_kernel_per_push_no_atomics_and_shares_the_mix():
    csrc = os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "csrc")
    code = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "uu3d_stream_rate.h")).read())
    assert "atomic" not in code.lower()
    assert "stream_timed_emit_multi_kernel(" in code and "stream_rate_reset_kernel(" in code
    assert not re.search(r"__device__[^\n]*\bresample_mix\(", code) and code.count("resample_mix(") >= 3
    body = code[code.index("stream_timed_emit_multi_kernel("):code.index("stream_rate_reset_kernel(")]
    assert "__syncthreads()" in body and "INT32_MAX" in body and "float4" in body
