"""CPU: several views (include/uu3d.h, SEVERAL VIEWS; views.py) -- the two rules in numpy (``predict.fuse_views_host``,
``predict.solve_view_roots_host``), the refusals of ``predict.predict_views`` and the C ABI.
  1. one view: the joint solve is the monocular rule (``solve_roots_host``) taken to world axes by the statements of
     ``camera_to_world_host``, in another algebra.  Both read float32 poses, so the comparison at 1e-9 needs cameras whose rotation maps
     float32 poses onto float32 poses exactly -- the 24 rotations of the cube, here 12 of them, at any position: then both solves see the
     same numbers and differ only in rounding (worst seen: 9.6e-14 m).  For a tilted camera the world pose is ROUNDED to float32 by
     uu3d_camera_to_world before the joint solve reads it, half an ulp of a 1 m pose is 3e-8 m per coordinate, and the normal matrix
     (condition number about 1e2) passes at most 1e2 times that into the root: the bound is 1e-5 there (worst seen: 7.5e-8 m).  The root
     is compared in float64 -- ``camera_to_world_host`` itself returns float32, whose rounding of a 4 m root is 2e-7 m.
  2. scale error: poses scaled by 1.1, three inward-looking cameras: the fused root's error lies below the smallest monocular one
     (seen: a mean of 0.0125 m with two views and 0.0121 m with three against 0.43 / 0.42 / 0.44 m).
  3. fusion: the exact cases.
  4. the seeded scenes of tests/test_views_gpu.py leave at least half of all frames solved, and their edge cases come out as stated.
  5. refusals: before any device is touched.
  6. the C ABI: exported, declared, guarded; the kernels have the shape the header states."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import util
from tests import views_util as VU

CUBE = [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (0.5, 0.5, 0.5, 0.5), (0.5, -0.5, 0.5, 0.5), (0.5, 0.5, -0.5, 0.5),
        (0.5, 0.5, 0.5, -0.5), (0.5, -0.5, -0.5, 0.5), (0.5, -0.5, 0.5, -0.5), (0.5, 0.5, -0.5, -0.5), (0.5, -0.5, -0.5, -0.5)]


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _camera_scene(R, J, seed):
    """A person 3 to 5 m in front of a camera, in CAMERA space -> (poses (R, J, 3) f32 root-relative, kp2d (R, J, 2) f32, roots (R, 3))."""
    rng = np.random.default_rng(seed)
    roots = np.stack([rng.normal(0.0, 0.5, R), rng.normal(0.0, 0.5, R), rng.uniform(3.0, 5.0, R)], axis=1)
    poses = rng.normal(0.0, 0.3, (R, J, 3)).astype(np.float32)
    poses[:, 0] = 0.0
    X = roots[:, None] + poses.astype(np.float64)
    fx, fy, cx, cy = VU.FX
    kp = np.stack([fx * X[..., 0] / X[..., 2] + cx, fy * X[..., 1] / X[..., 2] + cy], axis=-1).astype(np.float32)
    return poses, kp, roots


# ---- 1. one view ------------------------------------------------------------------------------------------------------------------------
def test_one_view_is_the_monocular_rule_in_world_axes():
    from uplift_upsample_3dhpe_amd import camera, predict
    R, J = 40, 17
    worst = {"cube": 0.0, "tilted": 0.0}
    tilted = [(0.81, -0.53, 0.2, 0.15), (-0.14, 0.15, 0.76, -0.62), (0.05, 0.7, -0.7, 0.1)]
    for kind, quats in (("cube", CUBE), ("tilted", tilted)):
        for i, q in enumerate(quats):
            cam = predict.Camera(*VU.FX, orientation=q, translation=(1.8 - i, 4.9 + 0.37 * i, 1.6))
            poses, kp, truth = _camera_scene(R, J, 7 + i)
            flags = np.ones((R, J), np.uint8)
            flags[3, 5:9], kp[4, 2] = 0, np.nan
            mono, ok = predict.solve_roots_host(poses, kp, cam.intrinsics, flags)
            assert ok.all() and np.abs(mono - truth).max() < 1e-4      # (the pose is exact here: only the pixels' float32 rounding is left)
            want = np.stack(camera._rotate_f64(cam.orientation, mono[:, 0], mono[:, 1], mono[:, 2]), axis=1) + cam.translation
            world, _ = predict.camera_to_world_host(poses, None, None, cam)
            if kind == "cube":                                           # the rotation is exact: a signed permutation of the float32 pose
                assert _same(np.sort(np.abs(world), axis=2), np.sort(np.abs(poses), axis=2))
            fused, count, sees = predict.fuse_views_host(world[None], kp[None], flags[None])
            assert _same(fused, world) and (count == 1).all() and sees.all()
            got, solved = predict.solve_view_roots_host(fused, kp[None], [cam], flags[None])
            assert solved.all()
            worst[kind] = max(worst[kind], float(np.abs(got - want).max()))
    print(f"one view against the monocular rule in world axes: exact rotations {worst['cube']:.3e} m, tilted cameras {worst['tilted']:.3e} m")
    assert worst["cube"] <= 1e-9
    assert worst["tilted"] <= 1e-5


# ---- 2. scale error ---------------------------------------------------------------------------------------------------------------------
def test_the_fused_root_beats_every_monocular_root_under_a_scale_error():
    from uplift_upsample_3dhpe_amd import camera, predict
    R, J = 30, 17
    rng = np.random.default_rng(5)
    cams = VU.ring_cameras(3, 9)
    roots = rng.normal(0.0, 0.3, (R, 3)) + np.array([0.0, 0.0, 0.9])
    pose = rng.normal(0.0, 0.3, (R, J, 3))
    pose[:, 0] = 0.0
    mono_err, worlds, kps = [], [], []
    for c in cams:
        Xc = predict.world_to_camera_host(roots[:, None] + pose, c)
        kp = VU.project(roots[:, None] + pose, c)[0].astype(np.float32)
        scaled = (1.1 * (Xc - Xc[:, :1])).astype(np.float32)            # the model's answer with a 10 % scale error, in camera space
        mono, ok = predict.solve_roots_host(scaled, kp, c.intrinsics)
        assert ok.all()
        in_world = np.stack(camera._rotate_f64(c.orientation, mono[:, 0], mono[:, 1], mono[:, 2]), axis=1) + c.translation
        mono_err.append(float(np.linalg.norm(in_world - roots, axis=1).mean()))
        worlds.append(predict.camera_to_world_host(scaled, None, None, c)[0])
        kps.append(kp)
    fused_err = {}
    for V in (2, 3):
        w, k = np.stack(worlds[:V]), np.stack(kps[:V])
        fused, count, _ = predict.fuse_views_host(w, k)
        got, solved = predict.solve_view_roots_host(fused, k, cams[:V])
        assert solved.all() and (count == V).all()
        fused_err[V] = float(np.linalg.norm(got - roots, axis=1).mean())
    print(f"root error under a 1.1 scale error: monocular {['%.3f' % e for e in mono_err]} m, two views {fused_err[2]:.4f} m, three views {fused_err[3]:.4f} m")
    assert fused_err[2] < min(mono_err[:2]) and fused_err[3] < min(mono_err)
    assert min(mono_err) > 0.2 and max(fused_err.values()) < 0.05        # (the depth ambiguity is what went away, not a rounding)


# ---- 3. fusion ---------------------------------------------------------------------------------------------------------------------------
def test_fusion_exact_cases():
    from uplift_upsample_3dhpe_amd import predict
    rng = np.random.default_rng(3)
    V, R, J, m = 3, 6, 17, 6
    poses = rng.normal(0.0, 0.5, (V, R, J, 3)).astype(np.float32)
    poses[:, :, 0] = 0.0
    poses[1, :, 0] = -0.0                                                # a view that hands over -0.0 at the root joint
    kp = rng.uniform(100.0, 900.0, (V, R, J, 2)).astype(np.float32)
    flags = np.ones((V, R, J), np.uint8)
    flags[0, 1, m - 1:] = 0                                              # frame 1: view 0 has one used joint too few
    kp[2, 2, :J - m + 1] = np.inf                                        # frame 2: view 2 likewise, through non-finite coordinates
    flags[:, 3] = 0                                                      # frame 3: nobody sees it
    poses[1, 4, 7, 2] = np.nan                                           # frame 4: NaN in
    flags[1:, 5] = 0                                                     # frame 5: view 0 alone
    fused, count, sees = predict.fuse_views_host(poses, kp, flags, m)
    assert fused.dtype == np.float32 and count.dtype == np.uint8 and sees.dtype == np.uint8 and sees.shape == (V, R)
    assert count.tolist() == [3, 2, 2, 0, 3, 1]
    assert sees.T.tolist() == [[1, 1, 1], [0, 1, 1], [1, 1, 0], [0, 0, 0], [1, 1, 1], [1, 0, 0]]
    assert _same(fused[:, 0], np.zeros((R, 3), np.float32))              # +0.0, bit for bit
    p64 = poses.astype(np.float64)
    assert _same(fused[0], (((p64[0, 0] + p64[1, 0]) + p64[2, 0]) / 3.0).astype(np.float32))
    assert _same(fused[1], ((p64[1, 1] + p64[2, 1]) / 2.0).astype(np.float32))
    assert _same(fused[2], ((p64[0, 2] + p64[1, 2]) / 2.0).astype(np.float32))
    assert _same(fused[3], (((p64[0, 3] + p64[1, 3]) + p64[2, 3]) / 3.0).astype(np.float32))      # nobody: the mean over ALL views
    assert np.isnan(fused[4, 7, 2]) and np.isfinite(np.delete(fused[4].ravel(), 7 * 3 + 2)).all()
    assert _same(fused[5], poses[0, 5])
    cams = VU.ring_cameras(V, 1)
    roots, solved = predict.solve_view_roots_host(fused, kp, cams, flags, m)
    assert not solved[3] and not roots[3].any()                          # nobody sees it: not solved
    # identical views return each view's bits when V is a power of two
    for V2 in (1, 2, 4, 8):
        same = np.repeat(poses[:1], V2, axis=0)
        got, count, _ = predict.fuse_views_host(same, np.repeat(kp[:1], V2, axis=0), None, m)
        assert _same(got, poses[0]) and (count == V2).all()
    with pytest.raises(ValueError):
        predict.fuse_views_host(poses, kp[:2], flags, m)
    with pytest.raises(ValueError):
        predict.fuse_views_host(np.zeros((9, 2, J, 3), np.float32), np.zeros((9, 2, J, 2), np.float32))
    with pytest.raises(ValueError):
        predict.solve_view_roots_host(fused, kp, cams[:2], flags, m)
    with pytest.raises(ValueError):
        predict.solve_view_roots_host(fused, kp, cams, flags, 1)


# ---- 4. the scenes of the GPU test -----------------------------------------------------------------------------------------------------
def test_the_gpu_scenes_are_mostly_solved_and_their_edge_cases_are_what_they_say():
    for case in VU.SHAPES + [(70, 17, 2, True), (257, 5, 3, True)]:
        R, J, V = case[:3]
        (cams, poses, kp, flags, truth), fused, count, sees, roots, solved = VU.host_rules(R, J, V, twin=len(case) == 4)
        assert solved.mean() >= 0.5, case
        err = np.linalg.norm(roots - truth, axis=1)[solved]
        # a solved frame is a sensible root: the views' poses carry 1 cm of noise on a 0.3 m skeleton, which one view turns into 3 % of its
        # 4.5 m of depth and more with five joints (the ambiguity this stage removes), two views into centimetres
        assert err.max() < (0.5 if V == 1 else 0.1), (case, float(err.max()))
        if R < 40:
            assert solved.all() and (count == V).all()
            continue
        assert not sees[0, VU.LOW] and count[VU.LOW] == V - 1 and bool(solved[VU.LOW]) == (V > 1), case
        assert count[VU.NOBODY] == 0 and not solved[VU.NOBODY] and not roots[VU.NOBODY].any(), case
        assert count[VU.BEHIND] == V and not solved[VU.BEHIND], case     # camera 0 sees the joint behind itself
        assert count[VU.ONE_PIXEL] == 1 and sees[0, VU.ONE_PIXEL] and not solved[VU.ONE_PIXEL], case
        assert np.isnan(fused).any() and (flags == 0).any() and np.isnan(kp).any()
        if len(case) == 4:
            assert cams[0] is cams[1]


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def test_predict_views_refuses_before_any_device_is_touched():
    from uplift_upsample_3dhpe_amd import predict
    cfg = util.load_config("h36m_81")
    cams = VU.ring_cameras(3, 2)
    track = lambda n: np.zeros((n, 17, 2), np.float32)
    views = [[track(20), track(31)] for _ in range(3)]
    call = lambda v, c, **kw: predict.predict_views(None, cfg, v, c, **kw)     # (model=None: anything that reached a device would raise another error)
    with pytest.raises(ValueError, match="1 to 8 lists"):
        call([], [])
    with pytest.raises(ValueError, match="1 to 8 lists"):
        call([[track(5)]] * 9, VU.ring_cameras(8, 2) + cams[:1])
    with pytest.raises(ValueError, match="needs extrinsics"):
        call(views, [cams[0], cams[1].without(extrinsics=True), cams[2]])
    with pytest.raises(ValueError, match="not plain"):
        call(views, [cams[0], VU.FX, cams[2]])
    with pytest.raises(ValueError, match="not plain"):
        call(views, cams[0])
    with pytest.raises(ValueError, match=re.escape("one Camera per view (3), got 2")):
        call(views, cams[:2])
    with pytest.raises(ValueError, match="same number of frames T_i in every view"):
        call([views[0], [track(20), track(30)], views[2]], cams)
    with pytest.raises(ValueError, match="same persons"):
        call([views[0], views[1][:1], views[2]], cams)
    with pytest.raises(ValueError, match="keyframes_only: the fusion needs one returned frame per given frame"):
        call(views, cams, keyframes_only=True)
    with pytest.raises(ValueError, match="out_fps: the fusion needs one returned frame per given frame"):
        call(views, cams, fps=25, out_fps=50)
    with pytest.raises(ValueError, match="a list of 3 lists"):
        call(views, cams, valid=[np.ones(20), np.ones(31)])
    with pytest.raises(ValueError, match="min_root_joints must be an int >= 2"):
        call(views, cams, min_root_joints=1)
    with pytest.raises(ValueError, match="interpolation must be one of"):
        call(views, cams, interpolation="spline")
    rows = predict.view_rows(cams)
    assert rows.shape == (3, 16) and rows.dtype == np.float64
    for c, r in zip(cams, rows):
        axes = r[4:13].reshape(3, 3)
        assert np.array_equal(r[:4], c.intrinsics) and np.array_equal(r[13:], c.translation) and np.abs(axes @ axes.T - np.eye(3)).max() < 1e-15
        assert np.abs(predict.world_to_camera_host(c.translation + axes[2], c) - [0.0, 0.0, 1.0]).max() < 1e-15      # r3 is the optical axis


# ---- 6. the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_guarded():
    from uplift_upsample_3dhpe_amd import _capi
    lib = _capi.load_library()
    header = open(os.path.join(util.ROOT, "include", "uu3d.h")).read()
    for s in ("uu3d_fuse_views", "uu3d_solve_view_roots"):
        assert s in _capi.EXPORTED_SYMBOLS and hasattr(lib, s) and re.search(r"\b" + s + r"\s*\(", header)
    assert "SEVERAL VIEWS" in header
    api = open(os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "csrc", "uu3d_api.hip")).read()
    assert '#include "uu3d_views.h"' in api and '#include "uu3d_views_api.inc"' in api
    buf = (C.c_double * 256)()                                          # 8-byte aligned host memory: every call below returns before a launch
    a = C.addressof(buf)
    p = lambda off=0: C.c_void_p(a + off)
    ok, bad, unsupported = _capi.UU3D_OK, _capi.UU3D_ERR_INVALID_ARGUMENT, _capi.UU3D_ERR_UNSUPPORTED
    fuse = lib.uu3d_fuse_views
    #    poses, kp2d, flags, views, rows, J, min_joints, fused, view_count, sees, stream
    assert fuse(p(), p(512), None, 2, 0, 17, 6, p(1024), p(1536), p(1600), None) == ok                    # no rows: nothing to do
    assert fuse(p(), p(512), None, 9, 2, 17, 6, p(1024), p(1536), p(1600), None) == unsupported
    assert fuse(p(), p(512), None, 2, 2, 65, 6, p(1024), p(1536), p(1600), None) == unsupported
    assert fuse(p(), p(512), None, 0, 2, 17, 6, p(1024), p(1536), p(1600), None) == bad
    assert fuse(p(), p(512), None, 2, -1, 17, 6, p(1024), p(1536), p(1600), None) == bad
    assert fuse(p(), p(512), None, 2, 2, 0, 6, p(1024), p(1536), p(1600), None) == bad
    assert fuse(p(), p(512), None, 2, 2, 17, 1, p(1024), p(1536), p(1600), None) == bad
    assert fuse(p(), p(512), None, 2, 2 ** 62, 17, 6, p(1024), p(1536), p(1600), None) == bad
    assert fuse(None, p(512), None, 2, 2, 17, 6, p(1024), p(1536), p(1600), None) == bad
    assert fuse(p(), None, None, 2, 2, 17, 6, p(1024), p(1536), p(1600), None) == bad
    assert fuse(p(), p(512), None, 2, 2, 17, 6, None, p(1536), p(1600), None) == bad
    assert fuse(p(), p(512), None, 2, 2, 17, 6, p(1024), None, p(1600), None) == bad
    assert fuse(p(), p(512), None, 2, 2, 17, 6, p(1024), p(1536), None, None) == bad
    assert fuse(p(), p(512), None, 2, 2, 17, 6, p(), p(1536), p(1600), None) == bad                       # in place
    assert fuse(p(2), p(512), None, 2, 2, 17, 6, p(1024), p(1536), p(1600), None) == bad                  # 4-byte aligned floats
    assert fuse(p(), p(516), None, 2, 2, 17, 6, p(1024), p(1536), p(1600), None) == bad                   # 8-byte loads of the pixels
    assert fuse(p(), p(512), None, 2, 2, 17, 6, p(1026), p(1536), p(1600), None) == bad
    solve = lib.uu3d_solve_view_roots
    #    fused, kp2d, flags, views, rows, J, cameras, min_joints, roots, solved, stream
    assert solve(p(), p(512), None, 2, 0, 17, p(1024), 6, p(1536), p(1800), None) == ok
    assert solve(p(), p(512), None, 9, 2, 17, p(1024), 6, p(1536), p(1800), None) == unsupported
    assert solve(p(), p(512), None, 2, 2, 65, p(1024), 6, p(1536), p(1800), None) == unsupported
    assert solve(p(), p(512), None, 0, 2, 17, p(1024), 6, p(1536), p(1800), None) == bad
    assert solve(p(), p(512), None, 2, -1, 17, p(1024), 6, p(1536), p(1800), None) == bad
    assert solve(p(), p(512), None, 2, 2, 17, p(1024), 1, p(1536), p(1800), None) == bad
    assert solve(None, p(512), None, 2, 2, 17, p(1024), 6, p(1536), p(1800), None) == bad
    assert solve(p(), None, None, 2, 2, 17, p(1024), 6, p(1536), p(1800), None) == bad
    assert solve(p(), p(512), None, 2, 2, 17, None, 6, p(1536), p(1800), None) == bad
    assert solve(p(), p(512), None, 2, 2, 17, p(1024), 6, None, p(1800), None) == bad
    assert solve(p(), p(512), None, 2, 2, 17, p(1024), 6, p(1536), None, None) == bad
    assert solve(p(), p(516), None, 2, 2, 17, p(1024), 6, p(1536), p(1800), None) == bad
    assert solve(p(), p(512), None, 2, 2, 17, p(1028), 6, p(1536), p(1800), None) == bad                  # 8-byte aligned doubles
    assert solve(p(), p(512), None, 2, 2, 17, p(1024), 6, p(1540), p(1800), None) == bad


def _compile(b, csrc, text, d, name):
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src, out = os.path.join(d, name + ".hip"), os.path.join(d, name + ".s")
    open(src, "w").write(text)
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", *b.DEVICE_FLAGS, "-I", csrc, "-S", "--cuda-device-only", "-o", out, src],
                   check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def _ops(asm, kernel):
    bodies = [m.group(0) for m in re.finditer(r"^(_ZN?[\w]+):.*?^\.Lfunc_end", asm, re.S | re.M) if kernel in m.group(1)]
    assert len(bodies) == 1, kernel
    return re.findall(r"^\s+([a-z_0-9]+)", bodies[0], re.M)


def test_kernels_have_the_shape_the_header_states():
    """Built for gfx950 on their own (the construction of tests/test_world_cpu.py): float64 arithmetic, a 12-byte store per lane of the
    fusion, no LDS, no atomics, no scratch -- and no fused float64 multiply-add of the kernels' own.  Both rules divide, and an IEEE
    float64 division expands on this target into a fixed sequence with fused steps of its own (v_div_scale, v_rcp, v_fma ..., v_div_fmas,
    v_div_fixup).  So the fused instructions are COUNTED: a kernel that holds nothing but one division, built beside them, says how many
    one division brings, and each kernel must hold exactly that many per v_div_fixup_f64 and not one more."""
    import importlib.util
    import tempfile
    csrc = os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "csrc")
    spec = importlib.util.spec_from_file_location("uu3d_build_views", os.path.join(util.ROOT, "uplift-upsample-3dhpe_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    if not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    one_division = ('#include <hip/hip_runtime.h>\n'
                    'extern "C" __global__ void one_division_kernel(const double* a, const double* b, double* c)\n'
                    '{\n#pragma clang fp contract(off)\n    c[threadIdx.x] = a[threadIdx.x] / b[threadIdx.x];\n}\n')
    with tempfile.TemporaryDirectory() as d:
        asm = _compile(b, csrc, '#include "uu3d_views.h"\n', d, "k")
        ref = _compile(b, csrc, one_division, d, "r")
    fused_op = lambda o: "f64" in o and ("fma" in o or "mad" in o)
    bodies = [m.group(0) for m in re.finditer(r"^(one_division_kernel):.*?^\.Lfunc_end", ref, re.S | re.M)]
    assert len(bodies) == 1
    ref_ops = re.findall(r"^\s+([a-z_0-9]+)", bodies[0], re.M)
    per_division = len([o for o in ref_ops if fused_op(o)])
    assert ref_ops.count("v_div_fixup_f64") == 1 and per_division >= 1
    for kernel in ("fuse_views_kernel", "solve_view_roots_kernel"):
        ops = _ops(asm, kernel)
        divisions = ops.count("v_div_fixup_f64")
        print(f"{kernel}: {divisions} divisions, {len([o for o in ops if fused_op(o)])} fused float64 instructions, {per_division} per division")
        assert divisions >= 1 and "v_add_f64" in ops
        assert len([o for o in ops if fused_op(o)]) == per_division * divisions, kernel
        assert not [o for o in ops if "atomic" in o or o.startswith(("ds_", "scratch_", "buffer_"))], kernel
    fuse = _ops(asm, "fuse_views_kernel")
    assert fuse.count("global_store_dwordx3") == 1 and "global_load_dwordx3" in fuse
    assert "v_mul_f64" in _ops(asm, "solve_view_roots_kernel")
    text = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "uu3d_views.h")).read())
    assert "atomic" not in text.lower() and "__shared__" not in text and text.count("fp contract(off)") == 2 and text.count("__launch_bounds__(256)") == 2
