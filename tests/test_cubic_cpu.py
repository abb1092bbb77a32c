"""CPU: C1 motion between keyframes -- ``predict_tracks(interpolation="cubic")`` -- as far as it needs no device.
  1. evaluation.keyframe_plan_cubic / keyframe_plan_cubic_at against the plan restated as a loop over one track's frames (tests/cubic_util)
  2. evaluation.interpolate_cubic_host, the rule in numpy: whose bits it keeps, what it reproduces, how far it beats the line
  3. the refusals: an unknown interpolation, keyframes that are not equally spaced
  4. uu3d_assemble_tracks_cubic: declared, exported, refusing what uu3d_assemble_tracks refuses; its doubles are never fused"""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import cubic_util as cu
from tests import util

CSRC = os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "csrc")


# ---- 1. the plans -----------------------------------------------------------------------------------------------------------------------
def test_track_table_has_the_keyframe_counts_it_is_meant_to_have():
    assert cu.TRACK_LENS == [1, 5, 6, 10, 11, 16, 26, 17]
    assert [len(range(0, n, cu.STRIDE)) for n in cu.TRACK_LENS] == [1, 1, 2, 2, 3, 4, 6, 4]


def test_keyframe_plan_cubic_equals_the_loop():
    from uplift_upsample_3dhpe_amd import evaluation
    f = cu.frame_indices()
    want = cu.loop_plan()
    got = evaluation.keyframe_plan_cubic(f, cu.STRIDE)
    assert len(got) == 5
    for g, w in zip(got, want):
        assert cu.same_bits(g, w)
    left, right, weight, _ = evaluation.keyframe_plan(f, cu.STRIDE)
    assert np.array_equal(got[1], left) and np.array_equal(got[2], right) and cu.same_bits(got[4], weight)
    before, after = got[0], got[3]
    assert (before[left == right] == -1).all() and (after[left == right] == -1).all()
    assert (before >= 0).sum() > 20 and (after >= 0).sum() > 20 and ((before < 0) & (left != right)).sum() > 20
    # the same through ``rows``: only keyframes are forwarded, and that is all the plan needs
    rows, W = cu.key_rows()
    through = evaluation.keyframe_plan_cubic(f, cu.STRIDE, rows=rows)
    for g, w in zip(through, cu.to_rows(want, rows)):
        assert cu.same_bits(g, w)
    linear = evaluation.keyframe_plan(f, cu.STRIDE, rows=rows)
    assert np.array_equal(through[1], linear[0]) and np.array_equal(through[2], linear[1]) and cu.same_bits(through[4], linear[2])
    assert max(int(a.max()) for a in through[:4]) == W - 1


@pytest.mark.parametrize("name", sorted(cu.STEPS))
def test_keyframe_plan_cubic_at_equals_the_loop(name):
    from uplift_upsample_3dhpe_amd import evaluation
    f = cu.frame_indices()
    positions = cu.positions_at(cu.STEPS[name])
    want = cu.loop_plan(positions=positions)
    got = evaluation.keyframe_plan_cubic_at(f, cu.STRIDE, positions)
    for g, w in zip(got, want):
        assert cu.same_bits(g, w)
    left, right, weight = evaluation.keyframe_plan_at(f, cu.STRIDE, positions)
    assert np.array_equal(got[1], left) and np.array_equal(got[2], right) and cu.same_bits(got[4], weight)
    assert (got[0][left == right] == -1).all() and (got[3][left == right] == -1).all()
    assert (got[0] >= 0).any() and (got[3] >= 0).any()
    if cu.STEPS[name].denominator > 1:
        assert (np.modf(weight * cu.STRIDE)[0] != 0).any()          # positions between two frames are there
    rows, _ = cu.key_rows()
    through = evaluation.keyframe_plan_cubic_at(f, cu.STRIDE, positions, rows=rows)
    for g, w in zip(through, cu.to_rows(want, rows)):
        assert cu.same_bits(g, w)


def test_a_row_that_was_not_forwarded_is_refused_as_today():
    from uplift_upsample_3dhpe_amd import evaluation
    f = cu.frame_indices()
    rows, _ = cu.key_rows()
    first = int(np.cumsum(cu.TRACK_LENS)[5])                          # track 6: 26 frames, keyframes at its places 0, 5, ..., 25
    for missing in (first, first + 10, first + 25):
        r = rows.copy()
        r[missing] = -1
        with pytest.raises(ValueError, match="not forwarded"):
            evaluation.keyframe_plan_cubic(f, cu.STRIDE, rows=r)
        with pytest.raises(ValueError, match="not forwarded"):
            evaluation.keyframe_plan_cubic_at(f, cu.STRIDE, cu.positions_at(cu.STEPS["fps30"]), rows=r)
    # frames 6 .. 9 of track 6: the line reads its keyframes 5 and 10, the cubic 0 and 15 as well
    pos = (np.full(4, 6), np.arange(6, 10), np.ones(4, np.int64))
    for missing in (first, first + 15):
        r = rows.copy()
        r[missing] = -1
        evaluation.keyframe_plan_at(f, cu.STRIDE, pos, rows=r)
        with pytest.raises(ValueError, match="not forwarded"):
            evaluation.keyframe_plan_cubic_at(f, cu.STRIDE, pos, rows=r)


# ---- 2. the rule in numpy ------------------------------------------------------------------------------------------------------------
def _random_predictions(W, J=17, seed=0):
    return np.random.default_rng(seed).normal(size=(W, J, 3)).astype(np.float32)


def test_keyframes_and_tail_frames_carry_the_inputs_bits():
    from uplift_upsample_3dhpe_amd import evaluation
    rows, W = cu.key_rows()
    pred = _random_predictions(W)
    for plan in (evaluation.keyframe_plan_cubic(cu.frame_indices(), cu.STRIDE, rows=rows),
                 evaluation.keyframe_plan_cubic_at(cu.frame_indices(), cu.STRIDE, cu.positions_at(cu.STEPS["fps30"]), rows=rows)):
        out = evaluation.interpolate_cubic_host(pred, plan)
        assert out.dtype == np.float32 and out.shape == (len(plan[1]), 17, 3)
        own = plan[1] == plan[2]
        assert own.sum() > 20 and (~own).sum() > 20 and cu.same_bits(out[own], pred[plan[1][own]])
        assert np.isfinite(out).all() and not cu.same_bits(out[~own], pred[plan[1][~own]])
    with pytest.raises(ValueError):
        evaluation.interpolate_cubic_host(pred.astype(np.float64), plan)


def test_stride_1_is_the_linear_rule_bit_for_bit():
    from uplift_upsample_3dhpe_amd import evaluation
    f = cu.frame_indices()
    pred = _random_predictions(len(f), seed=1)
    want, _ = evaluation.interpolate_between_keyframes(pred, f, 1)
    plan = evaluation.keyframe_plan_cubic(f, 1)
    assert (plan[0] == -1).all() and (plan[3] == -1).all() and np.array_equal(plan[1], plan[2])
    assert cu.same_bits(evaluation.interpolate_cubic_host(pred, plan), want) and cu.same_bits(want, pred)


def test_a_quadratic_in_time_is_reproduced_where_all_four_keyframes_exist():
    """x(t) = a t^2 + b t + c per coordinate, t in seconds at 50 Hz, 41 frames, all values in [1.25, 1.85]: one binade, so a float32 ulp
    is 2^-23 everywhere.  The keyframes are x rounded to float32 (half an ulp each); the four Catmull-Rom weights sum to at most 1.25
    in magnitude and the result is rounded once more: 1.25 / 2 + 1 / 2 < 2 ulps.  The line through two keyframes h = stride / 50 s
    apart misses x by a w (1 - w) h^2, at its worst frames (w = 0.4, 0.6) 0.24 a h^2 -- about a stride^2 / 4 in frames."""
    from uplift_upsample_3dhpe_amd import evaluation
    rng = np.random.default_rng(2)
    n, J = 41, 17
    a, b, c = rng.uniform(0.1, 0.3, size=(J, 3)), rng.uniform(0.05, 0.2, size=(J, 3)), rng.uniform(1.25, 1.5, size=(J, 3))
    t = (np.arange(n) / 50.0)[:, None, None]
    truth = ((a * t * t + b * t) + c).astype(np.float32)
    assert truth.min() >= 1.25 and truth.max() < 2.0
    f = np.arange(n)
    plan = evaluation.keyframe_plan_cubic(f, cu.STRIDE)
    full = (plan[0] >= 0) & (plan[3] >= 0)
    assert full.sum() == 4 * 6                                         # the segments 5..10 to 30..35
    cubic = evaluation.interpolate_cubic_host(truth, plan)
    linear, _ = evaluation.interpolate_between_keyframes(truth, f, cu.STRIDE)
    ulp = 2.0 ** -23
    err = np.abs(cubic.astype(np.float64) - truth)[full].max()
    print(f"cubic: worst error {err / ulp:.2f} ulps")
    assert err <= 2 * ulp
    h = cu.STRIDE / 50.0
    miss = np.abs(linear.astype(np.float64) - truth)[full].max(axis=0) / (0.24 * a * h * h)
    print(f"linear: worst error over 0.24 a h^2 in [{miss.min():.4f}, {miss.max():.4f}]")
    assert np.abs(miss - 1.0).max() < 0.01 and (0.24 * a * h * h).min() > 1000 * ulp


def test_on_a_sinusoid_the_cubic_beats_the_line():
    """sin(2 pi t + 0.3) at 1 Hz, sampled at 50 Hz, stride 5, frames whose four keyframes exist: the cubic's worst error is below half
    of the line's (a float64 restatement measures a ratio near 0.1)."""
    from uplift_upsample_3dhpe_amd import evaluation
    n = 101
    x = np.sin(2.0 * np.pi * np.arange(n) / 50.0 + 0.3).astype(np.float32).reshape(n, 1, 1)
    f = np.arange(n)
    plan = evaluation.keyframe_plan_cubic(f, cu.STRIDE)
    full = (plan[0] >= 0) & (plan[3] >= 0)
    cubic = np.abs(evaluation.interpolate_cubic_host(x, plan) - x)[full].max()
    linear = np.abs(evaluation.interpolate_between_keyframes(x, f, cu.STRIDE)[0] - x)[full].max()
    print(f"1 Hz, stride 5: linear {linear:.4f}, cubic {cubic:.4f}, ratio {cubic / linear:.3f}")
    assert full.sum() == 4 * 18 and cubic < 0.5 * linear


def test_rows_outside_the_predictions_give_nan():
    from uplift_upsample_3dhpe_amd import evaluation
    rows, W = cu.key_rows()
    pred = _random_predictions(W, J=2)
    plan = [a.copy() for a in evaluation.keyframe_plan_cubic(cu.frame_indices(), cu.STRIDE, rows=rows)]
    want = evaluation.interpolate_cubic_host(pred, plan)
    mixed = np.flatnonzero((plan[0] >= 0) & (plan[3] >= 0))
    plan[1][3], plan[2][7], plan[0][mixed[0]], plan[3][mixed[1]] = W, -1, W, -2
    bad = [3, 7, int(mixed[0]), int(mixed[1])]
    out = evaluation.interpolate_cubic_host(pred, plan)
    assert np.isnan(out[bad]).all() and cu.same_bits(np.delete(out, bad, 0), np.delete(want, bad, 0))


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------------
def test_an_unknown_interpolation_is_refused_before_anything_runs():
    from uplift_upsample_3dhpe_amd import options, predict
    cfg = util.load_config("h36m_81")
    tracks = [np.zeros((9, 17, 2), np.float32)]
    for bad in ("spline", "Cubic", None, 3):
        with pytest.raises(ValueError, match="interpolation"):
            predict.predict_tracks(None, cfg, tracks, interpolation=bad)
        with pytest.raises(ValueError, match="interpolation"):
            predict.predict_detections(None, cfg, [np.zeros((9, 2, 17, 2), np.float32)], interpolation=bad)
    assert inspect.signature(predict.predict_tracks).parameters["interpolation"].default == "linear"
    assert inspect.signature(options.stage_options).parameters["interpolation"].default == "linear"
    none = dict(keypoints=None, camera=None, min_root_joints=6, smooth=None, bones=None, repair_joints=None, fps=None, out_fps=None)
    assert options.stage_options(cfg, 1, "track", True, **none).interpolation == "linear"
    assert options.stage_options(cfg, 1, "track", True, interpolation="cubic", **none).interpolation == "cubic"
    assert options.INTERPOLATIONS == ("linear", "cubic") and predict.check_interpolation is options.check_interpolation


def test_unequally_spaced_keyframes_are_refused_by_the_plan():
    from uplift_upsample_3dhpe_amd import evaluation
    f = np.array([0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15])      # frame 6 is not there: keyframes at places 0, 5, 9, 14
    evaluation.keyframe_plan(f, cu.STRIDE)
    with pytest.raises(ValueError, match="equally spaced"):
        evaluation.keyframe_plan_cubic(f, cu.STRIDE)
    with pytest.raises(ValueError, match="equally spaced"):
        evaluation.keyframe_plan_cubic_at(f, cu.STRIDE, (np.zeros(1, np.int64), np.array([5]), np.array([2])))
    # two keyframes only: nothing to compare a spacing with
    evaluation.keyframe_plan_cubic(np.array([0, 1, 2, 3, 4, 5, 7, 8, 9]), cu.STRIDE)


# ---- 4. the C ABI and the kernel's arithmetic -------------------------------------------------------------------------------------------
def test_c_abi_declared_exported_and_refusing_as_the_linear_entry():
    import __graft_entry__ as ge
    ge.build()
    from uplift_upsample_3dhpe_amd import _capi, predict, tracks
    lib = _capi.load_library()
    header = open(os.path.join(util.ROOT, "include", "uu3d.h")).read()
    s = "uu3d_assemble_tracks_cubic"
    assert s in _capi.EXPORTED_SYMBOLS and hasattr(lib, s) and re.search(r"\b" + s + r"\s*\(", header)
    assert predict.assemble_tracks_cubic is tracks.assemble_tracks_cubic
    p = C.c_void_p(256)                                               # (an aligned address that is never dereferenced: the calls refuse first)

    def both(plain=p, flipped=None, order=None, windows=4, frames=3, J=17, root=6, out=p):
        a = lib.uu3d_assemble_tracks(plain, flipped, windows, order, p, p, p, frames, J, root, out, None)
        b = lib.uu3d_assemble_tracks_cubic(plain, flipped, windows, order, p, p, p, p, p, frames, J, root, out, None)
        assert a == b
        return b
    BAD = _capi.UU3D_ERR_INVALID_ARGUMENT
    assert both(plain=None) == BAD and both(windows=-1) == BAD and both(windows=0) == BAD and both(frames=-1) == BAD and both(frames=0) == BAD
    assert both(J=-1) == BAD and both(J=0) == BAD and both(root=17) == BAD and both(flipped=p) == BAD and both(out=None) == BAD
    assert both(out=C.c_void_p(264)) == BAD
    for k in range(4, 9):                                             # each of the five plan arrays
        args = [p, None, 4, None, p, p, p, p, p, 3, 17, 6, p, None]
        args[k] = None
        assert lib.uu3d_assemble_tracks_cubic(*args) == BAD


def test_kernel_rounds_every_double_operation_and_stores_16_bytes():
    import importlib.util
    spec = importlib.util.spec_from_file_location("uu3d_build_cubic", os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as d:
        src, out = os.path.join(d, "k.hip"), os.path.join(d, "k.s")
        open(src, "w").write('#include "uu3d_tracks.h"\n')
        subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", *b.DEVICE_FLAGS, "-I", CSRC, "-S", "--cuda-device-only", "-o", out, src],
                       check=True, stderr=subprocess.DEVNULL)
        asm = open(out).read()
    bodies = [m.group(0) for m in re.finditer(r"^(_ZN4uu3d\w+):.*?s_endpgm", asm, re.S | re.M) if "assemble_tracks_cubic_kernel" in m.group(1)]
    assert len(bodies) == 1
    body = bodies[0]
    assert "v_fma_f64" not in body and "v_mul_f64" in body and "v_add_f64" in body
    assert "global_store_dwordx4" in body and "global_atomic" not in body and "flat_atomic" not in body
    text = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "uu3d_tracks.h")).read())
    assert "atomic" not in text.lower()
