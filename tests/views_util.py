"""Seeded multi-view scenes for tests/test_views_cpu.py and tests/test_views_gpu.py (include/uu3d.h, SEVERAL VIEWS): V cameras on a ring
around the origin, looking inwards, one person near the origin, every view's own noisy world pose and the 2D keypoints of the true
skeleton, with the edge cases of the two rules placed at fixed frames."""
import numpy as np

FX = (1145.0, 1143.5, 512.25, 515.75)
SHAPES = [(R, J, V) for R in (1, 70, 257) for J in (5, 17) for V in (1, 2, 3, 8)]
# frames of the edge cases (scenes of at least 40 frames have them): a view below min_root_joints, a frame nobody sees, a joint behind a
# camera, a single seeing view whose used joints share one pixel
LOW, NOBODY, BEHIND, ONE_PIXEL = 5, 11, 17, 23


def min_joints(J):
    return 3 if J < 8 else 6


def ring_cameras(V, seed, twin=False, distortion=None):
    """V cameras 4 to 4.5 m from the origin at 1.2 to 1.8 m height, looking at a point near the origin, rolled a little.  ``twin``: camera
    1 is camera 0 once more.  ``distortion``: None or {view: coefficients}."""
    from uplift_upsample_3dhpe_amd import predict
    rng = np.random.default_rng(seed)
    cams = []
    for v in range(V):
        ang = 2.0 * np.pi * (v + 0.3 * rng.uniform()) / max(V, 3)
        pos = np.array([np.cos(ang), np.sin(ang), 0.0]) * rng.uniform(4.0, 4.5) + np.array([0.0, 0.0, rng.uniform(1.2, 1.8)])
        z = np.array([0.0, 0.0, 0.9]) + rng.normal(0.0, 0.1, 3) - pos    # forward: towards the person
        z /= np.linalg.norm(z)
        x = np.cross(z, np.array([0.0, 0.0, 1.0]) + rng.normal(0.0, 0.05, 3))      # right (image y points down: world up is -y)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        Rcw = np.stack([x, y, z])                                        # X_cam = Rcw (X_world - pos)
        q, t = predict.extrinsics_from_opencv(Rcw, -Rcw @ pos)
        cams.append(predict.Camera(*FX, distortion=None if distortion is None else distortion.get(v), orientation=q, translation=t))
    if twin and V > 1:
        cams[1] = cams[0]
    return cams


def project(points, cam):
    """World points (..., 3) float64 -> the pinhole pixels of ``cam`` (..., 2) float64 and the depth (...)."""
    from uplift_upsample_3dhpe_amd import predict
    c = predict.world_to_camera_host(points, cam)
    fx, fy, cx, cy = cam.intrinsics
    with np.errstate(all="ignore"):
        return np.stack([fx * c[..., 0] / c[..., 2] + cx, fy * c[..., 1] / c[..., 2] + cy], axis=-1), c[..., 2]


def scene(R, J, V, seed=None, twin=False):
    """-> (cameras, poses (V, R, J, 3) f32 world axes, kp2d (V, R, J, 2) f32, flags (V, R, J) u8, true roots (R, 3) f64)."""
    seed = 1000 * R + 10 * J + V if seed is None else seed
    rng = np.random.default_rng(seed)
    cams = ring_cameras(V, seed + 1, twin)
    roots = rng.normal(0.0, 0.3, (R, 3)) + np.array([0.0, 0.0, 0.9])
    truth = rng.normal(0.0, 0.3, (R, J, 3))
    truth[:, 0] = 0.0
    poses = (truth[None] + rng.normal(0.0, 0.01, (V, R, J, 3))).astype(np.float32)
    poses[:, :, 0] = 0.0
    kp = np.stack([project(roots[:, None] + truth, c)[0] for c in cams]).astype(np.float32)
    flags = np.ones((V, R, J), np.uint8)
    if R >= 40:
        lost = rng.uniform(size=(V, R, J)) < 0.04                        # scattered: lost joints as NaN, as cleared flags, NaN poses
        kp[lost] = np.nan
        flags[rng.uniform(size=(V, R, J)) < 0.04] = 0
        poses[V - 1, 31, J // 2, 1] = np.nan
        poses[0, 33] = np.nan
        for f in (LOW, NOBODY, BEHIND, ONE_PIXEL):
            kp[:, f] = np.stack([project(roots[f, None] + truth[f], c)[0] for c in cams]).astype(np.float32)
            flags[:, f] = 1
        flags[0, LOW, min_joints(J) - 1:] = 0                            # view 0 keeps one joint too few
        flags[:, NOBODY] = 0
        flags[V // 2:, NOBODY, :2] = 1
        kp[0, NOBODY] = np.nan
        away = np.asarray(cams[0].translation) - roots[BEHIND]            # 1.5 times the way to camera 0: behind it
        poses[:, BEHIND, J - 1] = (1.5 * away).astype(np.float32)
        flags[1:, ONE_PIXEL] = 0
        kp[0, ONE_PIXEL] = kp[0, ONE_PIXEL, 1]
    return cams, poses, kp, flags, roots


def host_rules(R, J, V, twin=False):
    """The two mirrors on ``scene(R, J, V)`` -> (the scene, fused, view_count, sees, roots f64, solved)."""
    from uplift_upsample_3dhpe_amd import predict
    s = scene(R, J, V, twin=twin)
    cams, poses, kp, flags, _ = s
    fused, count, sees = predict.fuse_views_host(poses, kp, flags, min_joints(J))
    roots, solved = predict.solve_view_roots_host(fused, kp, cams, flags, min_joints(J))
    return s, fused, count, sees, roots, solved
