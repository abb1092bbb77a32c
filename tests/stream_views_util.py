"""Seeded live multi-view scripts for tests/test_stream_views_cpu.py and tests/test_stream_views_gpu.py (include/uu3d.h, LIVE SEVERAL VIEWS):
the ring cameras of tests/views_util.py, N persons near the origin, every slot's camera-space pose and the pixels of the true skeleton per
push, view-major (slot v * N + i is person i in camera v), with the edge cases of the rule placed at fixed pushes."""
import numpy as np

from tests import views_util

J, M = 17, 6                                                             # joints, min_root_joints
BLIND = 6                                                                # the push at which every view of every person goes blind


def ticks_of(lookahead):
    """Pushes of a script: the blind push is read at BLIND + a, everybody is reset behind it, and the first fresh tick after that reads a
    blind frame again (state 0); the last two ticks read seen frames once more.  W = a + 1 <= 3 places: the ring wraps several times."""
    return BLIND + 3 * lookahead + 4


def person_tracks(V, N, ticks, seed):
    """-> (cameras, camera-space poses (ticks, V N, J, 3) f32, pixels (ticks, V N, J, 2) f32): N persons who walk a little, seen by V ring
    cameras; every view's pose is the true skeleton in that camera's axes plus its own noise."""
    from uplift_upsample_3dhpe_amd import predict
    rng = np.random.default_rng(seed)
    cams = views_util.ring_cameras(V, seed + 1)
    poses = np.zeros((ticks, V * N, J, 3), np.float32)
    kp = np.zeros((ticks, V * N, J, 2), np.float32)
    for i in range(N):
        start = rng.normal(0.0, 0.3, 3) + np.array([0.0, 0.0, 0.9])
        roots = start + np.cumsum(rng.normal(0.0, 0.01, (ticks, 3)), axis=0)
        truth = rng.normal(0.0, 0.3, (J, 3)) + rng.normal(0.0, 0.01, (ticks, J, 3))
        truth[:, 0] = 0.0
        for v, cam in enumerate(cams):
            t = np.asarray(cam.translation)
            rel = predict.world_to_camera_host(truth + t, cam) + rng.normal(0.0, 0.01, (ticks, J, 3))       # (rotated only)
            rel[:, 0] = 0.0
            poses[:, v * N + i] = rel.astype(np.float32)
            kp[:, v * N + i] = views_util.project(roots[:, None] + truth, cam)[0].astype(np.float32)
    return cams, poses, kp


def script(V, N, lookahead, seed=None):
    """The pushes of a stage-alone run -> (cameras, list of dicts per push: "kp" (T, J, 2), "flags" (T, J) u8, "active" (T,) bool, "poses"
    (T, J, 3) camera space, "reset": None, a list of slots or "all" -- applied BEHIND the push).  The slots' fresh flags follow from
    the counters (``fresh_of``).  Edge cases, all on person 0 unless said:
      push 2        view 0's joints share one pixel and every other view is flagged off: one seeing view of rank 2 (the rank guard)
      push 3        view 0 keeps one joint too few (below min_root_joints)
      push 4        view V - 1 is inactive (V == 1: the person does not take part at all)
      push 5        behind it, slot (view 0, person N - 1) is reset alone: its counter restarts, its views are out of phase from here on
      push BLIND    every view of every person pushes NaN: read at BLIND + a -- view_count 0, state 2 --, everybody is reset behind that
                    tick, and the next a + 1 pushes are blind again: the first fresh tick of the new tracks has view_count 0, state 0."""
    a = int(lookahead)
    ticks = ticks_of(a)
    seed = 100 * V + 10 * N + a if seed is None else seed
    cams, poses, kp = person_tracks(V, N, ticks, seed)
    T = V * N
    pushes = []
    for k in range(ticks):
        p = {"kp": kp[k].copy(), "flags": np.ones((T, J), np.uint8), "active": np.ones(T, bool), "poses": poses[k].copy(), "reset": None}
        if k == 2:
            p["kp"][0] = p["kp"][0, 1]
            for v in range(1, V):
                p["flags"][v * N] = 0
        if k == 3:
            p["flags"][0, M - 1:] = 0
        if k == 4:
            p["active"][(V - 1) * N] = False
        if k == 5:
            p["reset"] = [N - 1]
        if k == BLIND or BLIND + a < k <= BLIND + 2 * a + 1:
            p["kp"][:] = np.nan
        if k == BLIND + a:
            p["reset"] = "all"
        pushes.append(p)
    return cams, pushes


def fresh_of(count, active, lookahead, k, V, N):
    """The slots' fresh flags of push k from their counters AFTER the push: an active slot whose frame count - 1 - lookahead exists; slot
    (view V - 1, person N - 1) of a rig is fresh on even pushes only."""
    fresh = active & (count - 1 - int(lookahead) >= 0)
    if V > 1 and k % 2 == 1:
        fresh[V * N - 1] = False
    return fresh


def world_rows(cams, N):
    """The (V N, 7) rows of uu3d_camera_to_world, view-major."""
    return np.ascontiguousarray(np.stack([c.pose_row() for c in cams for _ in range(N)]))


def to_world(poses, rows):
    """camera.camera_to_world_rows_host on poses alone: (T, J, 3) camera space -> world axes, float32."""
    from uplift_upsample_3dhpe_amd import camera
    return camera.camera_to_world_rows_host(poses, None, None, rows)[0]


def same(a, b):
    """Bit for bit, NaN positions included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
