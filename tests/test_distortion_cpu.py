"""CPU: lens distortion (include/uu3d.h, LENS DISTORTION; camera.py) -- ``predict.Camera``, the rule in numpy
(``predict.undistort_points_host``), the forward model (``predict.distort_points_host``), the options and their refusals.
  1. round trip: for four coefficient sets, fx = fy = 1145, cx = 960, cy = 540, a 41 x 41 grid of ideal pixels over 1920 x 1080:
     undistort(float32(distort(p))) is within 1e-3 px of p and no point comes back NaN.  The bound: float32's ulp at 1920 is 1.2e-4 px; one
     rounding goes in and one comes out, through a map whose slope stays below 2 on these sets; the iteration itself adds about 3e-6 px.
  2. no preimage: k1 = -0.5 alone, an observation at normalised radius 0.7 -- r (1 - 0.5 r^2) never exceeds 0.544 -- is (NaN, NaN); at
     radius 0.3 it is accepted
  3. NaN / Inf in, NaN out; the vectorised mirror equals the rule written as plain Python floats, bit for bit
  4. a ``Camera`` without distortion gives ``stage_options`` what the tuple gives; every new refusal; the recorded refusals reproduce
  5. the C ABI: declared, bound, and every guard in front of the launch"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import util

SETS = [(-0.2, 0.25, -0.0007, -0.001, -0.01), (0.1, -0.2, 0.001, -0.002, 0.05), (-0.28, 0.09, 0.0005, -0.0003, -0.012), (-0.35, 0.15, 0.0, 0.0, 0.0)]
FX, FY, CX, CY = 1145.0, 1145.0, 960.0, 540.0
NO_PREIMAGE = (-0.5, 0.0, 0.0, 0.0, 0.0)


def _grid():
    return np.stack(np.meshgrid(np.linspace(0.0, 1920.0, 41), np.linspace(0.0, 1080.0, 41)), axis=-1).reshape(-1, 1, 2)


# ---- 1. round trip ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coefficients", SETS)
def test_round_trip_within_a_thousandth_of_a_pixel(coefficients):
    from uplift_upsample_3dhpe_amd import predict
    cam = predict.Camera(FX, FY, CX, CY, distortion=coefficients)
    ideal = _grid()
    seen = predict.distort_points_host(ideal, cam)
    assert seen.dtype == np.float64 and seen.shape == ideal.shape
    back = predict.undistort_points_host(seen.astype(np.float32), cam)
    assert back.dtype == np.float32 and back.shape == ideal.shape
    assert not np.isnan(back).any()
    err = np.abs(back.astype(np.float64) - ideal).max()
    moved = np.abs(seen - ideal).max()
    print(f"{coefficients}: the lens moves a point by up to {moved:.2f} px; worst round-trip error {err:.3g} px")
    assert err <= 1e-3
    assert moved > 10.0                                                  # (the sets distort: the round trip is not the identity's)


# ---- 2. no preimage ---------------------------------------------------------------------------------------------------------------------
def test_an_observation_without_a_preimage_is_nan():
    from uplift_upsample_3dhpe_amd import predict
    cam = predict.Camera(FX, FY, CX, CY, distortion=NO_PREIMAGE)
    r = np.linspace(0.0, 3.0, 3001)
    assert (r * (1.0 - 0.5 * r * r)).max() < 0.5444                     # the forward model's largest radius: 0.7 has no preimage
    at = lambda radius: np.array([[[CX + FX * radius * 0.6, CY + FY * radius * 0.8]]], np.float32)     # (a 3-4-5 direction)
    assert np.isnan(predict.undistort_points_host(at(0.7), cam)).all()
    got = predict.undistort_points_host(at(0.3), cam)
    assert np.isfinite(got).all()
    again = predict.distort_points_host(got, cam)                       # the accepted point projects onto the observation
    assert np.abs(again - at(0.3)).max() <= 1e-3 + 2.5e-4               # tol, and float32's rounding of the result through a slope < 2
    # a more generous tol changes no bit of an accepted point
    loose = predict.Camera(FX, FY, CX, CY, distortion=NO_PREIMAGE, tol=5.0)
    assert np.array_equal(predict.undistort_points_host(at(0.3), loose), got)


# ---- 3. pass-through, the mirror against plain floats ------------------------------------------------------------------------------------
def _scalar_rule(u, v, cam):
    """The rule on Python floats (IEEE double, every operation rounded once), statement for statement."""
    fx, fy, cx, cy = cam.intrinsics
    k1, k2, p1, p2, k3 = cam.distortion.tolist()
    u, v = float(np.float32(u)), float(np.float32(v))
    if not (math.isfinite(u) and math.isfinite(v)):
        return None
    x0 = (u - cx) / fx
    y0 = (v - cy) / fy
    x, y = x0, y0
    try:
        for _ in range(20):
            r2 = x * x + y * y
            ic = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
            dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
            x = (x0 - dx) * ic
            y = (y0 - dy) * ic
    except (ZeroDivisionError, OverflowError):
        return None
    r2 = x * x + y * y
    rad = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    xd = x * rad + dx
    yd = y * rad + dy
    if not (math.isfinite(x) and math.isfinite(y) and abs(xd - x0) * fx <= cam.tol and abs(yd - y0) * fy <= cam.tol):
        return None
    return np.float32(fx * x + cx), np.float32(fy * y + cy)


def test_nan_and_inf_pass_through_and_the_mirror_is_the_rule():
    from uplift_upsample_3dhpe_amd import predict
    cams = [predict.Camera(1145.0, 1143.5, 960.25, 540.75, distortion=SETS[2]), predict.Camera(600.0, 610.0, 320.0, 240.0, distortion=NO_PREIMAGE, tol=1e-4)]
    rng = np.random.default_rng(5)
    kp = np.concatenate([rng.uniform(-200.0, 2100.0, size=(40, 5, 2)), rng.uniform(-100.0, 800.0, size=(23, 5, 2))]).astype(np.float32)
    kp[0, 0], kp[1, 1, 0], kp[2, 2, 1], kp[41, 3] = np.nan, np.inf, -np.inf, np.nan
    kp[3, 0], kp[50, 0] = (960.25, 540.75), (320.0, 240.0)              # exactly (cx, cy)
    got = predict.undistort_points_host(kp, cams, lens=[40, 23])
    assert np.isnan(got[0, 0]).all() and np.isnan(got[1, 1]).all() and np.isnan(got[2, 2]).all() and np.isnan(got[41, 3]).all()
    assert np.array_equal(got[3, 0], kp[3, 0]) and np.array_equal(got[50, 0], kp[50, 0])
    lost = 0
    for r in range(len(kp)):
        for j in range(kp.shape[1]):
            want = _scalar_rule(kp[r, j, 0], kp[r, j, 1], cams[0 if r < 40 else 1])
            if want is None:
                lost += 1
                assert np.isnan(got[r, j]).all(), (r, j)
            else:
                assert np.array_equal(got[r, j].view(np.uint32), np.array(want, np.float32).view(np.uint32)), (r, j)
    assert 10 < lost < kp.shape[0] * kp.shape[1] // 2                    # both outcomes are common (the k1 = -0.5 camera refuses its border)
    assert np.array_equal(got[np.isnan(got)].view(np.uint32), np.full(int(np.isnan(got).sum()), 0x7fc00000, np.uint32))      # THE quiet NaN
    # a list of tracks in, a list out: the same bits
    listed = predict.undistort_points_host([kp[:40], kp[40:]], cams)
    assert np.array_equal(np.concatenate(listed).view(np.uint32), got.view(np.uint32))
    # zero coefficients: the rule's result for a pinhole, the point itself up to float32's rounding of (u - cx) / fx * fx + cx
    flat = predict.undistort_points_host(kp[4:40], predict.Camera(1145.0, 1143.5, 960.25, 540.75))
    assert np.abs(flat.astype(np.float64) - kp[4:40]).max() <= 2.5e-4


# ---- 4. options and refusals ------------------------------------------------------------------------------------------------------------
def _options(camera, per="track", count=3, **more):
    from uplift_upsample_3dhpe_amd.options import stage_options
    kw = dict(keypoints=None, camera=camera, min_root_joints=6 if per == "track" else None, smooth=None, bones=None, repair_joints=None, fps=None,
              out_fps=None)
    kw.update(more)
    return stage_options(util.load_config("h36m_81"), count, per, True, **kw)


def test_a_camera_without_distortion_is_the_tuple():
    from uplift_upsample_3dhpe_amd import predict, stream
    assert stream.Camera is predict.Camera and stream.undistort_points_host is predict.undistort_points_host
    t = (1145.0, 1143.5, 512.25, 515.75)
    for per in ("track", "slot"):
        want = _options(t, per)
        for cam in (predict.Camera(*t), predict.Camera(*t, distortion=None, tol=0.5), predict.Camera(*t, distortion=(0, 0, 0, 0, 0)),
                    [predict.Camera(*t)] * 3):
            got = _options(cam, per)
            assert got.lens is None and np.array_equal(got.cameras, want.cameras) and got.cameras.dtype == want.cameras.dtype
            assert got[1:8] == want[1:8]
        assert want.lens is None and _options(None, per).lens is None
        with_lens = _options(predict.Camera(*t, distortion=SETS[0], tol=0.01), per)
        assert np.array_equal(with_lens.cameras, want.cameras)
        assert with_lens.lens.shape == (3, 10) and with_lens.lens.dtype == np.float64
        assert np.array_equal(with_lens.lens, np.tile(np.array(t + SETS[0] + (0.01,)), (3, 1)))
        each = [predict.Camera(t[0] + i, t[1], t[2], t[3] - i, distortion=SETS[i]) for i in range(3)]
        per_track = _options(each, per)
        assert np.array_equal(per_track.lens[:, :4], per_track.cameras) and np.array_equal(per_track.lens[:, 4:9], np.array(SETS[:3]))
    assert predict.Camera.ITERATIONS == 20 and predict.Camera(*t).tol == 1e-3


def test_new_refusals():
    from uplift_upsample_3dhpe_amd import predict
    t = (1145.0, 1143.5, 512.25, 515.75)
    bad = [dict(distortion=(0.1, 0.0, 0.0, float("nan"), 0.0)), dict(distortion=(0.1, float("inf"), 0.0, 0.0, 0.0)), dict(distortion=(0.1, 0.2, 0.0, 0.0)),
           dict(distortion=(0.1,) * 8), dict(distortion=0.1), dict(distortion="barrel"), dict(distortion=SETS[0], tol=0.0), dict(distortion=SETS[0], tol=-1.0),
           dict(distortion=SETS[0], tol=float("nan")), dict(distortion=SETS[0], tol=float("inf")), dict(tol=None), dict(tol="tight")]
    for kw in bad:
        with pytest.raises(ValueError):
            predict.Camera(*t, **kw)
    # the intrinsics: in check_cameras' own words
    with pytest.raises(ValueError, match=re.escape("camera must be finite (fx, fy, cx, cy) with fx > 0 and fy > 0")):
        predict.Camera(0.0, 1.0, 2.0, 3.0, distortion=SETS[0])
    with pytest.raises(ValueError, match=re.escape("camera must be finite (fx, fy, cx, cy) with fx > 0 and fy > 0")):
        predict.Camera(1.0, float("nan"), 2.0, 3.0)
    lens, plain = predict.Camera(*t, distortion=SETS[0]), predict.Camera(*t)
    for per in ("track", "slot"):
        with pytest.raises(ValueError, match="not a mix"):
            _options([lens, t, lens], per)
        with pytest.raises(ValueError, match="not a mix"):
            _options([t, plain, t], per)
        with pytest.raises(ValueError, match="all have distortion or all have none"):
            _options([lens, plain, lens], per)
        for cams in ([lens] * 2, [plain] * 2):                           # a wrong count: check_cameras' words
            with pytest.raises(ValueError, match=re.escape(f"camera must be one (fx, fy, cx, cy) or one per {per} (3), got shape (2, 4)")):
                _options(cams, per)
    # what is refused today with a camera stays refused with a Camera
    with pytest.raises(ValueError, match=re.escape("min_root_joints must be an int >= 2")):
        _options(lens, min_root_joints=1)
    # the functions of the rule take Cameras only
    kp = np.zeros((4, 3, 2), np.float32)
    for cam in (t, [lens], [lens, t], None):
        with pytest.raises(ValueError):
            predict.undistort_points_host(kp, cam, lens=[2, 2])
    with pytest.raises(ValueError):
        predict.undistort_points_host(kp, [lens, lens], lens=[2, 3])
    with pytest.raises(ValueError):
        predict.undistort_points_host(np.zeros((4, 3)), lens)
    with pytest.raises(ValueError):
        predict.distort_points_host(kp, t)


def test_the_recorded_refusals_reproduce():
    from tests import test_track_modules_cpu as recorded
    recorded.test_stage_options_refuse_in_the_callers_words()
    recorded.test_stage_options_record()


def test_live_refusals_keep_their_words():
    """``StreamSession._init_plan`` with a ``Camera``: together with ``out_fps``, and more than one with ``detections``, as with tuples."""
    from uplift_upsample_3dhpe_amd import predict, stream
    cfg = util.load_config("h36m_81")
    cam = predict.Camera(1145.0, 1143.5, 512.25, 515.75, distortion=SETS[0])
    s = object.__new__(stream.StreamSession)
    with pytest.raises(ValueError, match="camera together with out_fps is not supported yet"):
        s._init_plan(None, cfg, 3, None, 4, None, 40, True, False, 10, 50, 50, camera=cam)
    with pytest.raises(ValueError, match=re.escape("detections takes ONE camera (fx, fy, cx, cy), not one per slot")):
        s._init_plan(None, cfg, 3, None, 4, None, 5, True, False, None, 50, None, detections=4, camera=[cam] * 3)


# ---- 5. the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_and_guarded():
    from uplift_upsample_3dhpe_amd import _capi
    lib = _capi.load_library()
    header = open(os.path.join(util.ROOT, "include", "uu3d.h")).read()
    s = "uu3d_undistort_points"
    assert s in _capi.EXPORTED_SYMBOLS and hasattr(lib, s) and re.search(r"\b" + s + r"\s*\(", header)
    assert "uu3d_undistort.h" in open(os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "csrc", "uu3d_api.hip")).read()
    buf = (C.c_double * 64)()                                           # 8-byte aligned host memory: every call below returns before a launch
    a = C.addressof(buf)
    p = lambda off=0: C.c_void_p(a + off)
    call = lib.uu3d_undistort_points
    assert call(p(), p(256), 0, 17, None, 1, p(128), None) == _capi.UU3D_OK                          # no rows: nothing to do
    bad = _capi.UU3D_ERR_INVALID_ARGUMENT
    assert call(p(), p(256), -1, 17, None, 1, p(128), None) == bad
    assert call(p(), p(256), 2, 0, None, 1, p(128), None) == bad
    assert call(p(), p(256), 2, 17, None, 0, p(128), None) == bad
    assert call(None, p(256), 2, 17, None, 1, p(128), None) == bad
    assert call(p(), None, 2, 17, None, 1, p(128), None) == bad
    assert call(p(), p(256), 2, 17, None, 1, None, None) == bad
    assert call(p(), p(), 2, 17, None, 1, p(128), None) == bad                                       # in place
    assert call(p(4), p(256), 2, 17, None, 1, p(128), None) == bad                                   # 8-byte loads and stores
    assert call(p(), p(260), 2, 17, None, 1, p(128), None) == bad
    assert call(p(), p(256), 2, 17, None, 1, p(132), None) == bad
    assert call(p(), p(256), 2, 17, p(2), 1, p(128), None) == bad
    assert call(p(), p(256), 2 ** 62, 17, None, 1, p(128), None) == bad


def test_kernel_has_the_shape_the_header_states():
    """One 8-byte load of the point and one 8-byte store per lane, float64 arithmetic, no LDS, no atomics, no scratch.  (The rounding of
    every operation is checked on the bits, against the mirror, in tests/test_distortion_gpu.py: an IEEE float64 division expands into
    fused steps of its own, so the absence of a fused multiply-add cannot be read off the instruction names here.)"""
    import importlib.util
    import subprocess
    import tempfile
    csrc = os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "csrc")
    spec = importlib.util.spec_from_file_location("uu3d_build_undistort", os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as d:
        src, out = os.path.join(d, "k.hip"), os.path.join(d, "k.s")
        open(src, "w").write('#include "uu3d_undistort.h"\n')
        subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", *b.DEVICE_FLAGS, "-I", csrc, "-S", "--cuda-device-only", "-o", out, src],
                       check=True, stderr=subprocess.DEVNULL)
        asm = open(out).read()
    bodies = [m.group(0) for m in re.finditer(r"^(_ZN4uu3d\w+):.*?s_endpgm", asm, re.S | re.M) if "undistort_points_kernel" in m.group(1)]
    assert len(bodies) == 1
    ops = re.findall(r"^\s+([a-z_0-9]+)", bodies[0], re.M)
    assert ops.count("global_load_dwordx2") == 1 and [o for o in ops if "store" in o] == ["global_store_dwordx2"]
    assert "v_mul_f64" in ops and "v_add_f64" in ops and "v_div_fixup_f64" in ops
    assert not [o for o in ops if "atomic" in o or o.startswith(("ds_", "scratch_", "buffer_"))]
    text = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "uu3d_undistort.h")).read())
    assert "atomic" not in text.lower() and "__shared__" not in text and "fp contract(off)" in text and "__launch_bounds__(256)" in text
