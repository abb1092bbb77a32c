"""No GPU: the host planning of stream.StreamSession(fps=F) -- rate_plan and its per-push mirror push_plan -- against predict.resample_plan
and against brute-force searches in Fractions; the refusals; the command line; the C ABI of the new launches."""
import ctypes as C
import inspect
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import util

RATES = [24, 25, 30, 60, 29.97, (30000, 1001), 10, 50]
CASES = [("h36m_81", None), ("h36m_351", None), ("h36m_351", 10)]
PUSHES = 700


def _rho(fps):
    from uplift_upsample_3dhpe_amd import predict
    return Fraction(50) / predict.frame_rate(fps)


@pytest.mark.parametrize("fps", RATES)
def test_input_plan_is_resample_plan_push_by_push(fps):
    """700 pushes: every model frame at or before the newest source frame is made exactly once, at the push of its right neighbour, with
    resample_plan's left / right / weight (the weight's bits included); the counts per push are the issue's formula."""
    from uplift_upsample_3dhpe_amd import predict, stream
    cfg = util.load_config("h36m_81")
    plan = stream.rate_plan(cfg, fps, None)
    rho = _rho(fps)
    assert Fraction(plan.A, plan.B) == rho and math.gcd(plan.A, plan.B) == 1 and plan.n_max == math.ceil(rho)
    made, counts = [], []
    for j in range(PUSHES):
        m = stream.push_plan(j, plan)["model"]
        counts.append(len(m))
        for k, left, right, w in m:
            assert right == j == math.ceil(Fraction(k) / rho)            # made at the push of its right neighbour
            made.append((k, left, right, w))
    K = math.floor((PUSHES - 1) * rho)
    assert [k for k, _, _, _ in made] == list(range(K + 1))               # each exactly once, in order
    assert counts[0] == 1 and counts[1:] == [math.floor(j * rho) - math.floor((j - 1) * rho) for j in range(1, PUSHES)]
    assert max(counts) <= plan.n_max and (max(counts) == plan.n_max or rho < 1)
    model_lens, left, right, weight = predict.resample_plan([PUSHES], fps)
    assert model_lens[0] in (K + 1, K + 2)                                # (resample_plan adds one clamped frame behind a fractional end)
    assert np.array_equal(left[:K + 1], [m[1] for m in made]) and np.array_equal(right[:K + 1], [m[2] for m in made])
    assert np.array_equal(weight[:K + 1].view(np.uint64), np.array([m[3] for m in made], np.float64).view(np.uint64))
    assert all((m[3] == 0.0) == (m[1] == m[2]) for m in made)


def _brute(cfg, ms, fps, lookahead, periods=3):
    """a_m, D and the smallest lookahead by the definitions, in Fractions, over `periods` periods of j."""
    from uplift_upsample_3dhpe_amd import stream
    _, _, P = stream.session_strides(cfg, ms)
    rho = _rho(fps)
    span = periods * rho.denominator * P

    def keys(q):
        u = q * rho
        k0 = math.floor(u / P) * P
        return k0, (k0 if u == k0 else k0 + P)

    def slack(L):
        return min(math.floor(j * rho) - keys(j - L)[1] for j in range(L, L + span))
    lo = next(L for L in range(10 ** 6) if slack(L) >= 0)
    if lookahead is None:
        lookahead = lo
    a_m = min(stream.max_lookahead(cfg), slack(lookahead))
    D = 1 + max(((math.floor(j * rho) - a_m) // P * P - keys(j - lookahead)[0]) // P for j in range(lookahead, lookahead + span))
    return a_m, D, lo


@pytest.mark.parametrize("cfgname,ms", CASES)
@pytest.mark.parametrize("fps", RATES)
def test_lookahead_plan_against_brute_force(cfgname, ms, fps):
    from uplift_upsample_3dhpe_amd import stream
    cfg = util.load_config(cfgname)
    lo = stream.rate_plan(cfg, fps, None, ms).min_lookahead
    for la in (lo, lo + 1, lo + 7, lo + 40, 400):
        plan = stream.rate_plan(cfg, fps, la, ms)
        a_m, D, lo_b = _brute(cfg, ms, fps, la)
        assert (plan.a_m, plan.D, plan.min_lookahead) == (a_m, D, lo_b), (la, plan)
        assert 0 <= plan.a_m <= stream.max_lookahead(cfg) and plan.D >= 1 and plan.lookahead == la
    assert stream.rate_plan(cfg, fps, 400, ms).a_m == stream.max_lookahead(cfg)       # (a long lookahead: every window complete)
    # the plan holds push by push: both keyframes have been emitted and are still in the ring when they are read
    plan = stream.rate_plan(cfg, fps, lo + 3, ms)
    P = plan.pred_stride
    for j in range(plan.lookahead, plan.lookahead + 400):
        pp = stream.push_plan(j, plan)
        newest = ((j * plan.A) // plan.B - plan.a_m) // P * P
        assert pp["q"] == j - plan.lookahead and pp["k0"] % P == 0 and pp["k1"] in (pp["k0"], pp["k0"] + P)
        assert pp["k1"] <= newest and (newest - pp["k0"]) // P < plan.D
        u = Fraction(pp["q"] * plan.A, plan.B)
        assert pp["k0"] <= u < pp["k0"] + P and (pp["k1"] == pp["k0"]) == (u == pp["k0"])
        assert pp["weight"] == float(np.float64(pp["q"] * plan.A - pp["k0"] * plan.B) / np.float64(P * plan.B))     # one float64 division
        assert abs(Fraction(pp["weight"]) - (u - pp["k0"]) / P) <= Fraction(1, 2 ** 52)
    if plan.lookahead:
        assert stream.push_plan(plan.lookahead - 1, plan)["q"] is None


@pytest.mark.parametrize("cfgname,ms", CASES)
@pytest.mark.parametrize("fps", RATES)
def test_refusals_name_the_minimum(cfgname, ms, fps):
    from uplift_upsample_3dhpe_amd import stream
    cfg = util.load_config(cfgname)
    lo = stream.rate_plan(cfg, fps, None, ms).min_lookahead
    stream.rate_plan(cfg, fps, lo, ms)                                   # the minimum itself is fine
    if lo > 0:
        with pytest.raises(ValueError, match=rf"at least {lo} source frames"):
            stream.rate_plan(cfg, fps, lo - 1, ms)
        stub = type("M", (), {"arch": type("A", (), {"compiled_dims": True})(), "device": "cpu", "has_strided_input": True})()
        with pytest.raises(ValueError, match=rf"at least {lo} source frames"):      # the constructor refuses before it touches a device
            stream.StreamSession(stub, cfg, slots=2, mask_stride=ms, lookahead=lo - 1, fps=fps)
    else:
        assert stream.rate_plan(cfg, fps, 0, ms).a_m >= 0
    for bad in (0, -5, float("nan"), "x"):
        with pytest.raises(ValueError):
            stream.rate_plan(cfg, bad, 10, ms)


def test_25_fps_is_what_a_ratio_of_two_implies():
    """rho = 2: u = 2 q.  h36m_81 (P = 2): every output is a keyframe -- k0 == k1 == 2 q, weight 0, nothing interpolated -- so a_m = 2 L
    (up to the maximum) and one ring place is enough.  h36m_351 (P = 5): a keyframe only where 2 q is a multiple of 5."""
    from uplift_upsample_3dhpe_amd import stream
    cfg = util.load_config("h36m_81")
    for L in (0, 1, 7, 20, 33):
        plan = stream.rate_plan(cfg, 25, L)
        assert (plan.A, plan.B, plan.n_max, plan.min_lookahead) == (2, 1, 2, 0)
        assert plan.a_m == min(2 * L, stream.max_lookahead(cfg))
        assert plan.D == 1 + (2 * L - plan.a_m) // 2
        for j in range(L, L + 50):
            pp = stream.push_plan(j, plan)
            assert pp["k0"] == pp["k1"] == 2 * (j - L) and pp["weight"] == 0.0
            assert [m[0] for m in pp["model"]] == ([0] if j == 0 else [2 * j - 1, 2 * j])
    cfg = util.load_config("h36m_351")
    plan = stream.rate_plan(cfg, 25, 6)
    for j in range(6, 80):
        pp = stream.push_plan(j, plan)
        q = j - 6
        assert (pp["k0"] == pp["k1"]) == ((2 * q) % 5 == 0) and pp["k0"] == (2 * q) // 5 * 5
        assert pp["weight"] == float(np.float64((2 * q) % 5) / np.float64(5))


@pytest.mark.parametrize("cfgname,ms", CASES)
def test_50_fps_is_the_plain_session_plus_dense_output(cfgname, ms):
    """A = B = 1: every push makes exactly the model frame that IS the pushed frame, the sub-tick runs at a_m = a - (P - 1) -- the pose
    between two keyframes needs the later one -- and where q is a multiple of P (the pushes at which a plain session at lookahead a is
    fresh) the output is keyframe q itself; everywhere else it is interpolated: dense output."""
    from uplift_upsample_3dhpe_amd import stream
    cfg = util.load_config(cfgname)
    _, _, P = stream.session_strides(cfg, ms)
    assert stream.rate_plan(cfg, 50, None, ms).min_lookahead == P - 1
    for a in (P - 1, P, 2 * P - 1, 13, stream.max_lookahead(cfg)):
        plan = stream.rate_plan(cfg, 50, a, ms)
        assert (plan.A, plan.B, plan.n_max, plan.a_m) == (1, 1, 1, a - (P - 1))
        for j in range(a + 3 * P + 1):
            pp = stream.push_plan(j, plan)
            assert pp["model"] == [(j, j, j, 0.0)]
            if j >= a:
                q = j - a
                assert stream.emits(j + 1, a, cfg, ms) == (q % P == 0) == (pp["k0"] == pp["k1"])
                assert pp["k0"] == q // P * P and pp["weight"] == float(np.float64(q % P) / np.float64(P))
            else:
                assert pp["q"] is None


def test_command_line_and_signatures():
    from uplift_upsample_3dhpe_amd import stream
    base = ["--config", "c.json", "--weights", "w.h5", "--input", "i.npz", "--output", "o.npz"]
    assert stream.parse_args(base).fps is None
    assert stream.parse_args(base + ["--fps", "30000/1001"]).fps == Fraction(30000, 1001)
    assert stream.parse_args(base + ["--fps", "29.97"]).fps == Fraction(2997, 100)
    with pytest.raises(SystemExit):
        stream.parse_args(base + ["--fps", "0"])
    p = inspect.signature(stream.StreamSession.__init__).parameters
    assert p["fps"].default is None and p["model_fps"].default == 50
    p = inspect.signature(stream.replay_tracks).parameters
    assert p["fps"].default is None and p["model_fps"].default == 50
    assert isinstance(stream.StreamSession.source_frames, property)
    bench = open(os.path.join(util.ROOT, "tools", "stream_bench.py")).read()
    assert '"--fps"' in bench


SYMBOLS = ("uu3d_stream_rate_state_layout", "uu3d_stream_source_push", "uu3d_stream_resample_stage", "uu3d_stream_file_keyframe",
           "uu3d_stream_timed_emit", "uu3d_stream_rate_reset")


def test_symbols_declared_exported_and_refusing():
    import __graft_entry__ as ge
    ge.build()
    from uplift_upsample_3dhpe_amd import _capi
    lib = _capi.load_library()
    header = open(os.path.join(util.ROOT, "include", "uu3d.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", header), s
        assert s in _capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert C.sizeof(_capi.Uu3dStreamRate) == 16 and C.sizeof(_capi.Uu3dStreamRateLayout) == 64
    assert [f for f, _ in _capi.Uu3dStreamRate._fields_] == re.sub(r"/\*.*?\*/", "", re.search(
        r"typedef struct uu3d_stream_rate \{ int32_t ([^;]*);", header).group(1)).replace(" ", "").split(",")
    assert [f for f, _ in _capi.Uu3dStreamRateLayout._fields_] == re.search(
        r"typedef struct uu3d_stream_rate_layout \{\s*int64_t ([^;]*);", header).group(1).replace(" ", "").split(",")
    # the plain session's structs are untouched, and arguments are refused before anything is launched (no device needed)
    assert C.sizeof(_capi.Uu3dStreamConfig) == 32 and C.sizeof(_capi.Uu3dStreamLayout) == 56
    bad = _capi.UU3D_ERR_INVALID_ARGUMENT
    cfg, rate, lay = _capi.Uu3dStreamConfig(3, 5, 5, 5, 0, 1, 1, 6), _capi.Uu3dStreamRate(5, 3, 4, 2), _capi.Uu3dStreamRateLayout()
    assert lib.uu3d_stream_rate_state_layout(None, C.byref(cfg), C.byref(rate), C.byref(lay)) == bad
    assert lib.uu3d_stream_source_push(None, C.byref(cfg), C.byref(rate), None, None, None, None, 0, None) == bad
    assert lib.uu3d_stream_resample_stage(None, C.byref(cfg), C.byref(rate), None, None, None, None, None, None, None) == bad
    assert lib.uu3d_stream_file_keyframe(None, C.byref(cfg), C.byref(rate), None, None, None) == bad
    assert lib.uu3d_stream_timed_emit(None, C.byref(cfg), C.byref(rate), None, None, None, None) == bad
    assert lib.uu3d_stream_rate_reset(None, C.byref(cfg), C.byref(rate), None, None, None) == bad


def test_source_has_no_atomics_and_shares_the_helpers():
    csrc = os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "csrc")
    code = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "uu3d_stream_rate.h")).read())
    assert "atomic" not in code.lower()
    assert '#include "uu3d_stream_rate.h"' in open(os.path.join(csrc, "uu3d_api.hip")).read()
    # the normalisation and the float64 mix are uu3d_resample_tracks' own device functions, not restated
    for helper in ("normalize_pair", "resample_mix", "resample_source_pair", "finite_pair"):
        assert re.search(r"__device__ __forceinline__ \w+ " + helper + r"\(", open(os.path.join(csrc, "uu3d_tracks.h")).read()), helper
        assert not re.search(r"__device__[^\n]*\b" + helper + r"\(", code), helper
    assert "resample_mix(" in code and "resample_source_pair(" in code and "finite_pair(" in code


def test_the_bracket_rule_is_stated_once_for_ints_and_arrays():
    """rates.keyframe_bracket against the scalar formula of the plans (restated here), on the rates the tests use against 50 both ways
    round, P in {1, 2, 5}, the first 2000 positions of each: once on Python ints, once on one int64 array, equal element for element."""
    from uplift_upsample_3dhpe_amd import rates

    def scalar(q, A, B, P):
        k0 = q * A // B // P * P
        off = q * A - k0 * B
        return k0, (k0 if off == 0 else k0 + P), off, P * B
    q = np.arange(2000, dtype=np.int64)
    for fps in (24, 25, 30, 60, (2997, 100), (30000, 1001)):
        for rho in (Fraction(50) / rates.frame_rate(fps), rates.frame_rate(fps) / Fraction(50)):
            A, B = rho.numerator, rho.denominator
            for P in (1, 2, 5):
                want = [scalar(int(i), A, B, P) for i in q]
                got = [rates.keyframe_bracket(int(i) * A, B, P) for i in q]
                assert got == want and all(type(v) is int for g in got for v in g)
                k0, k1, off, den = rates.keyframe_bracket(q * A, B, P)
                assert k0.dtype == k1.dtype == off.dtype == np.int64 and den == P * B
                assert np.array_equal(np.stack([k0, k1, off, np.full_like(q, den)], 1), np.array(want, np.int64))
