"""No GPU: the host planning of stream.StreamSession(fps=F, interpolation="cubic") -- rate_plan's cubic form and the mirrors
push_plan_cubic / out_push_plan_cubic -- simulated push by push against a ring of D places, against brute force in Fractions and against
evaluation.keyframe_plan_cubic_at; the linear plan is what it was; the refusals; the C ABI of the two new launches."""
import ctypes as C
import inspect
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import util

PAIRS = [(10, 50), (30, 60), (25, 30), (30, 24), (29.97, 50), (24, 24)]                  # test_stream_out_fps_cpu's
CASES = [(name, ms) for name in ("h36m_81", "h36m_351") for ms in util.load_config(name).MASK_STRIDE]
FPS_ONLY = [("h36m_81", 4, 25), ("h36m_81", 4, 24), ("h36m_351", 5, 30), ("h36m_351", 10, 60), ("h36m_81", 4, 29.97)]     # test_stream_fps_gpu's
SIMULATED = [("h36m_81", 4, 24, None), ("h36m_81", 4, 30, None), ("h36m_81", 4, 29.97, None), ("h36m_351", 5, 30, None)] + \
            [(name, ms, fps, out) for name, ms in (("h36m_81", 4), ("h36m_351", 5)) for fps, out in ((10, 50), (30, 60), (30, 24))]


@pytest.mark.parametrize("cfgname,ms", CASES)
def test_the_linear_plan_is_the_plan_without_the_keyword(cfgname, ms):
    from uplift_upsample_3dhpe_amd import rates
    cfg = util.load_config(cfgname)
    for fps, out_fps in PAIRS + [(f, None) for n, m, f in FPS_ONLY if (n, m) == (cfgname, ms)] + [(f, None) for f in (10, 24, 25, 30)]:
        lo = rates.rate_plan(cfg, fps, None, ms, out_fps=out_fps).min_lookahead
        for la in (None, lo, lo + 4, 300):
            assert rates.rate_plan(cfg, fps, la, ms, out_fps=out_fps, interpolation="linear") == rates.rate_plan(cfg, fps, la, ms, out_fps=out_fps)
            assert rates.rate_plan(cfg, fps, la, ms, 50, out_fps, "linear") == rates.rate_plan(cfg, fps, la, ms, 50, out_fps)
        if lo > 0:                                                        # ... and the refusal in the words it had
            with pytest.raises(ValueError, match=rf"between two model keyframes .* at least {lo} source frames"):
                rates.rate_plan(cfg, fps, lo - 1, ms, out_fps=out_fps, interpolation="linear")


def _period(fps, out_fps, P, B):
    """Source frames in one period: B P without an output rate, else the smallest time that is a whole number of source frames, output
    frames and keyframes."""
    from uplift_upsample_3dhpe_amd import rates
    if out_fps is None:
        return B * P
    steps = (1 / rates.frame_rate(fps), 1 / rates.frame_rate(out_fps), Fraction(P, 50))
    t = Fraction(math.lcm(*(s.numerator for s in steps)), math.gcd(*(s.denominator for s in steps)))
    assert all((t / s).denominator == 1 for s in steps)
    return int(t * rates.frame_rate(fps))


def _simulate(plan, fps, out_fps):
    """Pushes j = 0 .. over two periods plus the lookahead under ``plan`` (whose D, lookahead and a_m the caller may have replaced): the
    sub-ticks of push_plan emit keyframes into a ring of plan.D places, tracked by what each place holds, and every keyframe that every
    returned pose reads (the up to four of the cubic mirrors) must have been emitted and still be in its place.
    -> (reads as (j, position, before, k0, k1, after, weight), the reads that failed as (j, keyframe))."""
    from uplift_upsample_3dhpe_amd import rates
    P = plan.pred_stride
    n = 2 * _period(fps, out_fps, P, plan.B) + plan.lookahead + 7
    ring, emitted, reads, failed = {}, set(), [], []
    for j in range(n):
        for k, _, _, _ in rates.push_plan(j, plan)["model"]:
            c = k - plan.a_m
            if c >= 0 and c % P == 0:                                     # the sub-tick of model frame k emits keyframe c
                emitted.add(c)
                ring[(c // P) % plan.D] = c
        if out_fps is None:
            pp = rates.push_plan_cubic(j, plan)
            frames = [] if pp["q"] is None else [(Fraction(pp["q"] * plan.A, plan.B), pp["before"], pp["k0"], pp["k1"], pp["after"], pp["weight"])]
        else:
            frames = [(Fraction(i * plan.pos_num, plan.pos_den),) + tuple(rest) for i, *rest in rates.out_push_plan_cubic(j, plan)]
        for frame in frames:
            reads.append((j,) + frame)
            for k in sorted({k for k in frame[1:5] if k is not None}):
                if k not in emitted or ring.get((k // P) % plan.D) != k:
                    failed.append((j, k))
    return reads, failed


@pytest.mark.parametrize("cfgname,ms,fps,out_fps", SIMULATED)
@pytest.mark.parametrize("extra", [0, 3])
def test_every_read_of_the_cubic_plan_is_emitted_and_kept_and_both_bounds_are_minimal(cfgname, ms, fps, out_fps, extra):
    from uplift_upsample_3dhpe_amd import rates
    cfg = util.load_config(cfgname)
    lo = rates.rate_plan(cfg, fps, None, ms, out_fps=out_fps, interpolation="cubic").min_lookahead
    plan = rates.rate_plan(cfg, fps, lo + extra, ms, out_fps=out_fps, interpolation="cubic")
    linear = rates.rate_plan(cfg, fps, max(lo + extra, rates.rate_plan(cfg, fps, None, ms, out_fps=out_fps).min_lookahead), ms, out_fps=out_fps)
    P = plan.pred_stride
    assert plan.min_lookahead == lo and plan.lookahead == lo + extra and 0 <= plan.a_m <= rates.max_lookahead(cfg)
    assert (plan.A, plan.B, plan.n_max, plan.pred_stride) + tuple(plan[8:]) == (linear.A, linear.B, linear.n_max, linear.pred_stride) + tuple(linear[8:])
    assert plan._fields == linear._fields
    reads, failed = _simulate(plan, fps, out_fps)
    assert not failed, failed[:5]
    # the reads are the rule's, by brute force in Fractions: the bracket, the two outer keyframes, the one-sided first segment
    mixed = first_segment = 0
    for j, u, before, k0, k1, after, w in reads:
        assert k0 == math.floor(u / P) * P
        if u == k0:
            assert (before, k1, after, w) == (None, k0, None, 0.0)
        else:
            mixed += 1
            first_segment += k0 == 0
            assert (before, k1, after) == (k0 - P if k0 >= P else None, k0 + P, k0 + 2 * P)
            off = (u - k0) * (plan.B if out_fps is None else plan.pos_den)
            assert off.denominator == 1 and w == float(np.float64(int(off)) / np.float64(P * (plan.B if out_fps is None else plan.pos_den)))
    # (a slot's first segment is read iff a returned pose lies strictly inside (0, P): not at 24 fps on P = 2, where frame 1 sits at 25/12)
    step = Fraction(plan.A, plan.B) if out_fps is None else Fraction(plan.pos_num, plan.pos_den)
    assert mixed > 0 and (first_segment > 0) == (step < P) and mixed < len(reads)
    # one place fewer loses a keyframe that is read; one source frame of lookahead fewer -- even with the keyframes emitted as early as
    # they can be, a_m = 0, and a ring that forgets nothing -- reads one that has not been emitted
    assert plan.D >= 2 and _simulate(plan._replace(D=plan.D - 1), fps, out_fps)[1]
    if lo > 0:
        late = _simulate(plan._replace(lookahead=lo - 1, a_m=0, D=4096), fps, out_fps)[1] if extra == 0 else [None]
        assert late
        with pytest.raises(ValueError, match=rf"cubic.*at least {lo} source frames"):
            rates.rate_plan(cfg, fps, lo - 1, ms, out_fps=out_fps, interpolation="cubic")
    # the cubic never asks for less than the line
    assert lo >= rates.rate_plan(cfg, fps, None, ms, out_fps=out_fps).min_lookahead and plan.D >= linear.D


@pytest.mark.parametrize("cfgname,ms,fps,out_fps", SIMULATED)
def test_the_mirrors_are_the_linear_ones_with_keyframe_plan_cubic_ats_outer_keyframes(cfgname, ms, fps, out_fps):
    from uplift_upsample_3dhpe_amd import evaluation, rates
    cfg = util.load_config(cfgname)
    plan = rates.rate_plan(cfg, fps, None, ms, out_fps=out_fps, interpolation="cubic")
    P, L = plan.pred_stride, plan.lookahead
    n = min(max(2 * _period(fps, out_fps, P, plan.B), 60), 400) + L + 7
    num, den, got = [], [], []
    for j in range(n):
        pp, pc = rates.push_plan(j, plan), rates.push_plan_cubic(j, plan)
        assert {k: pc[k] for k in pp} == pp and sorted(set(pc) - set(pp)) == ["after", "before"]
        if out_fps is None:
            if pp["q"] is None:
                assert pc["before"] is None and pc["after"] is None
                continue
            num.append(pp["q"] * plan.A); den.append(plan.B)
            got.append((pc["before"], pc["k0"], pc["k1"], pc["after"], pc["weight"]))
        else:
            frames, cubic = rates.out_push_plan(j, plan), rates.out_push_plan_cubic(j, plan)
            assert [(i, k0, k1, w) for i, _, k0, k1, _, w in cubic] == frames
            for i, before, k0, k1, after, w in cubic:
                num.append(i * plan.pos_num); den.append(plan.pos_den)
                got.append((before, k0, k1, after, w))
    assert len(got) > 20
    frames = np.arange(max(nu // de for nu, de in zip(num, den)) + 3 * P + 1)          # long enough that every `after` exists
    before, left, right, after, weight = evaluation.keyframe_plan_cubic_at(frames, P, (np.zeros(len(num), np.int64), np.array(num), np.array(den)))
    none = lambda v: -1 if v is None else v
    assert np.array_equal(before, [none(g[0]) for g in got]) and np.array_equal(after, [none(g[3]) for g in got])
    assert np.array_equal(left, [g[1] for g in got]) and np.array_equal(right, [g[2] for g in got])
    assert np.array_equal(weight.view(np.uint64), np.array([g[4] for g in got], np.float64).view(np.uint64))
    step = Fraction(plan.A, plan.B) if out_fps is None else Fraction(plan.pos_num, plan.pos_den)
    assert (after[left != right] >= 0).all() and ((before[left != right] < 0).sum() > 0) == (step < P)
    if out_fps is None:
        with pytest.raises(ValueError, match="no output rate"):
            rates.out_push_plan_cubic(L, plan)


def test_the_ring_limit_and_its_error_stay():
    from uplift_upsample_3dhpe_amd import rates
    cfg = util.load_config("h36m_81")
    with pytest.raises(ValueError, match=r"keyframes per slot; at most 4096"):
        rates.rate_plan(cfg, 30, 20000, 4, interpolation="cubic")


def test_refusals_and_signatures():
    from uplift_upsample_3dhpe_amd import rates, stream
    cfg = util.load_config("h36m_81")
    stub = type("M", (), {"arch": type("A", (), {"compiled_dims": True})(), "device": "cpu", "has_strided_input": True})()
    with pytest.raises(ValueError, match=r'interpolation="cubic" needs fps'):           # refused before anything touches a device
        stream.StreamSession(stub, cfg, slots=2, interpolation="cubic")
    for kw in ({}, {"fps": 30, "lookahead": 9}):
        with pytest.raises(ValueError, match=r"interpolation must be one of 'linear', 'cubic', got 'spline'"):
            stream.StreamSession(stub, cfg, slots=2, interpolation="spline", **kw)
    with pytest.raises(ValueError, match=r"interpolation must be one of"):
        rates.rate_plan(cfg, 30, None, interpolation="spline")
    lo = rates.rate_plan(cfg, 30, None, 4, interpolation="cubic").min_lookahead
    with pytest.raises(ValueError, match=rf"cubic.*at least {lo} source frames"):
        stream.StreamSession(stub, cfg, slots=2, mask_stride=4, lookahead=lo - 1, fps=30, interpolation="cubic")
    assert inspect.signature(stream.StreamSession).parameters["interpolation"].default == "linear"
    assert inspect.signature(stream.replay_tracks).parameters["interpolation"].default == "linear"
    assert inspect.signature(rates.rate_plan).parameters["interpolation"].default == "linear"
    assert "interpolation" not in stream.LIVE_OPTIONS and stream.push_plan_cubic is rates.push_plan_cubic
    assert stream.out_push_plan_cubic is rates.out_push_plan_cubic
    bench = open(os.path.join(util.ROOT, "tools", "stream_bench.py")).read()
    assert '"--interpolation"' in bench


SYMBOLS = ("uu3d_stream_timed_emit_cubic", "uu3d_stream_timed_emit_multi_cubic")


def test_symbols_declared_exported_and_refusing():
    import __graft_entry__ as ge
    ge.build()
    from uplift_upsample_3dhpe_amd import _capi
    lib = _capi.load_library()
    header = open(os.path.join(util.ROOT, "include", "uu3d.h")).read()
    assert "LIVE C1 MOTION" in header
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", header), s
        assert s in _capi.EXPORTED_SYMBOLS and hasattr(lib, s), s
    assert lib.uu3d_stream_timed_emit_cubic.argtypes == lib.uu3d_stream_timed_emit.argtypes
    assert lib.uu3d_stream_timed_emit_multi_cubic.argtypes == lib.uu3d_stream_timed_emit_multi.argtypes
    # arguments are refused before anything is launched (no device needed), with the status of the linear siblings
    cfg, rate, outp = _capi.Uu3dStreamConfig(3, 5, 5, 5, 0, 1, 1, 6), _capi.Uu3dStreamRate(5, 3, 5, 4), _capi.Uu3dStreamOut(5, 1, 1, 1, 5)
    assert lib.uu3d_stream_timed_emit_cubic(None, C.byref(cfg), C.byref(rate), None, None, None, None) == \
        lib.uu3d_stream_timed_emit(None, C.byref(cfg), C.byref(rate), None, None, None, None) == _capi.UU3D_ERR_INVALID_ARGUMENT
    assert lib.uu3d_stream_timed_emit_multi_cubic(None, C.byref(cfg), C.byref(rate), C.byref(outp), None, None, None, None) == \
        lib.uu3d_stream_timed_emit_multi(None, C.byref(cfg), C.byref(rate), C.byref(outp), None, None, None, None) == _capi.UU3D_ERR_INVALID_ARGUMENT


def test_the_cubic_emits_share_hermite_mix_and_the_siblings_shape():
    csrc = os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "csrc")
    code = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "uu3d_stream_rate.h")).read())
    tracks = open(os.path.join(csrc, "uu3d_tracks.h")).read()
    assert re.search(r"__device__ __forceinline__ float hermite_mix\(", tracks) and tracks.count("#pragma clang fp contract(off)") >= 1
    assert not re.search(r"__device__[^\n]*\bhermite_mix\(", code) and "fp contract" not in code and "h01" not in code      # called, not restated
    reader = code[code.index("keyframe_read_cubic("):code.index("stream_timed_emit_cubic_kernel(")]
    assert reader.count("hermite_mix(") == 1 and reader.count("% key_ring") == 4 and "has0 ?" in reader
    single = code[code.index("stream_timed_emit_cubic_kernel("):code.index("stream_timed_emit_multi_cubic_kernel(")]
    multi = code[code.index("stream_timed_emit_multi_cubic_kernel("):code.index("stream_rate_reset_kernel(")]
    for body in (single, multi):
        assert body.count("keyframe_read_cubic(") == 1 and "keyframe_read(" not in body and "float4" in body and "atomic" not in body.lower()
    assert "__syncthreads()" in multi and "INT32_MAX" in multi and "fresh_out" in single and "out_held" in single
