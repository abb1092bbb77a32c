"""Seeded scenes for tests/test_view_calibrate_cpu.py and tests/test_view_calibrate_gpu.py (include/uu3d.h, WHERE THE CAMERAS STAND), on
the ring cameras and the projection of tests/views_util.py: one or two persons who walk on a curve and turn while their limbs move, the
TRUE world joints kept, every view's lift in that camera's OWN axes -- the true root-relative skeleton scaled by ``scale`` plus
``lift_noise`` metres of noise --, pixels with ``px_noise`` pixels of noise, and every camera's true pose against camera 0."""
import functools

import numpy as np

from tests import views_util as VU

ROOT = 0


def _qmul(a, b):
    w0, x0, y0, z0 = a
    w1, x1, y1, z1 = b
    return np.array([w0 * w1 - x0 * x1 - y0 * y1 - z0 * z1, w0 * x1 + x0 * w1 + y0 * z1 - z0 * y1,
                     w0 * y1 - x0 * z1 + y0 * w1 + z0 * x1, w0 * z1 + x0 * y1 - y0 * x1 + z0 * w1], np.float64)


def true_poses(cams):
    """Every camera's pose against camera 0 -> (q (V, 4) with w >= 0, c (V, 3)): X_0 = qrot(q_v, X_v) + c_v."""
    from uplift_upsample_3dhpe_amd import predict
    q0 = np.asarray(cams[0].orientation, np.float64)
    qs, cs = [], []
    for c in cams:
        q = _qmul(q0 * np.array([1.0, -1.0, -1.0, -1.0]), np.asarray(c.orientation, np.float64))
        qs.append(-q if q[0] < 0 else q)
        cs.append(predict.world_to_camera_host(np.asarray(c.translation, np.float64), cams[0]))
    return np.stack(qs), np.stack(cs)


def walkers(persons, T, J, rng):
    """-> the world joints (persons * T, J, 3) float64 and the root-relative skeletons in world axes, the persons back to back."""
    joints, rel = [], []
    for i in range(persons):
        t = np.arange(T) / 50.0
        body = rng.normal(0.0, 0.25, (J, 3))
        body[ROOT] = 0.0
        swing = 0.08 * np.sin(2.0 * np.pi * (1.1 + 0.2 * i) * t)[:, None, None] * rng.normal(0.0, 1.0, (J, 3))
        turn = 0.9 * t + 0.6 * np.sin(0.7 * t) + 2.0 * i
        c, s = np.cos(turn), np.sin(turn)
        shape = body[None] + swing
        shape[:, ROOT] = 0.0
        r = np.stack([c[:, None] * shape[..., 0] - s[:, None] * shape[..., 1], s[:, None] * shape[..., 0] + c[:, None] * shape[..., 1], shape[..., 2]], -1)
        root = np.stack([0.9 * np.cos(0.8 * t + 2.5 * i) + 0.3 * i, 0.7 * np.sin(1.1 * t + 1.0 * i) - 0.2 * i, 0.9 + 0.05 * np.sin(3.0 * t)], -1)
        rel.append(r)
        joints.append(root[:, None] + r)
    return np.concatenate(joints), np.concatenate(rel)


def scene(V, persons, T, J=17, scale=1.0, lift_noise=0.0, px_noise=0.0, seed=None):
    """-> dict: cams (the true cameras, with extrinsics), bare (the same without), poses (V, R, J, 3) f32 in each camera's own axes, kp
    (V, R, J, 2) f32, truth (R, J, 3) f64 world joints, q (V, 4) and c (V, 3): the true poses against camera 0."""
    from uplift_upsample_3dhpe_amd import predict
    seed = 9000 * V + 900 * persons + T + J if seed is None else seed
    rng = np.random.default_rng(seed)
    cams = VU.ring_cameras(V, seed + 1)
    truth, rel = walkers(persons, T, J, rng)
    lifts = np.stack([predict.world_to_camera_host(rel + np.asarray(c.translation), c) for c in cams])      # rotated only
    poses = (scale * lifts + (rng.normal(0.0, lift_noise, lifts.shape) if lift_noise else 0.0)).astype(np.float32)
    poses[:, :, ROOT] = 0.0
    clean = np.stack([VU.project(truth, c)[0] for c in cams])
    kp = (clean + (rng.normal(0.0, px_noise, clean.shape) if px_noise else 0.0)).astype(np.float32)
    q, c = true_poses(cams)
    return dict(cams=cams, bare=[k.without(extrinsics=True) for k in cams], poses=poses, kp=kp, truth=truth, q=q, c=c, V=V, R=truth.shape[0], J=J,
                scale=scale)


EXACT = [(2, 1, 257), (3, 2, 129), (8, 1, 257)]                          # V, persons, frames per person
NOISY = [(3, 1, 257, 1.0), (3, 1, 257, 1.1), (3, 2, 129, 1.1)]           # ... and the scale of the lifts


@functools.lru_cache(maxsize=None)
def host_rules(V, persons, T, scale=1.0, noisy=False, J=17):
    """The mirror on ``scene``, computed once and shared; nobody writes to what this returns -> (the scene, pose (V, 8), terms (V,))."""
    from uplift_upsample_3dhpe_amd import predict
    s = scene(V, persons, T, J, scale, 0.01 if noisy else 0.0, 0.5 if noisy else 0.0)
    pose, terms = predict.calibrate_views_host(s["poses"], s["kp"], s["bare"])
    for a in (s["poses"], s["kp"], s["truth"], s["q"], s["c"], pose, terms):
        a.setflags(write=False)
    return s, pose, terms


def angle_deg(q, p):
    """The angle between two unit quaternions' rotations, in degrees, up to sign."""
    d = min(1.0, abs(float(np.dot(q, p))))
    return float(np.degrees(2.0 * np.arccos(d)))


def random_inputs(V, R, J, seed, with_flags, lost=0.05):
    """Random lifts, keypoints with NaN and Inf sprinkled in and flags for the launches alone; when R allows it, view V - 1 sees no row at
    all (a view with zero terms) and no view sees a row of the second chunk (a chunk with zero terms).
    -> (poses (V, R, J, 3) f32, kp (V, R, J, 2) f32, flags (V, R, J) u8 or None, intrinsics (V, 4) f64)."""
    rng = np.random.default_rng(seed)
    poses = rng.normal(0.0, 0.3, (V, R, J, 3)).astype(np.float32)
    poses[:, :, ROOT] = 0.0
    kp = (rng.normal(0.0, 150.0, (V, R, J, 2)) + 512.0).astype(np.float32)
    bad = rng.uniform(size=(V, R, J))
    kp[bad < lost] = np.nan
    kp[(bad >= lost) & (bad < 1.5 * lost), 0] = np.inf
    flags = (rng.uniform(size=(V, R, J)) > lost).astype(np.uint8) if with_flags else None
    if V >= 3 and R >= 255:
        kp[V - 1, :, : J - 2] = np.nan                                   # two joints left: below every min_root_joints
    if R > 4096:
        kp[0, 4096:8192] = np.nan
    intr = np.array([[1145.0 + 3.0 * v, 1143.5 - 2.0 * v, 512.25 + v, 515.75 - v] for v in range(V)], np.float64)
    return poses, kp, flags, intr
