"""Seeded scenes for tests/test_triangulate_cpu.py and tests/test_triangulate_gpu.py (include/uu3d.h, WHERE RAYS MEET), on the ring cameras
and the projection of tests/views_util.py: one person near the origin, the TRUE world joints kept, every view's own monocular lift scaled
by ``scale`` (the error all views share) plus 1 cm of noise, pixels with 0.5 px of noise, 4 % scattered NaN joints and cleared flags, and
the edge cases of the rule at fixed frames of scenes with at least 40 frames."""
import functools

import numpy as np

from tests import views_util as VU

SHAPES = VU.SHAPES                                                       # R in {1, 70, 257}, J in {5, 17}, V in {1, 2, 3, 8}
TWINS = [(70, 17, 2, True), (257, 5, 3, True)]                           # camera 1 is camera 0 once more
ROOT = 0
NOISE_PX, OUTLIER_PX, LOST = 0.5, 40.0, 0.04
# the frames of the edge cases and the joint they are planted at (joint 0 is the root joint; every other joint of these frames is clean)
TWIN, BEHIND, OUTLIER3, OUTLIER2, ONE, LOW, NO_ROOT = 3, 7, 13, 19, 23, 29, 35
AT = 2


def scene(R, J, V, twin=False, scale=1.1, seed=None):
    """-> dict: cams, truth (R, J, 3) f64 world joints, poses (V, R, J, 3) f32 world axes and root-relative, kp (V, R, J, 2) f32, flags
    (V, R, J) u8, edges: whether the edge cases are planted."""
    seed = 7000 * R + 70 * J + V + (3 if twin else 0) if seed is None else seed
    rng = np.random.default_rng(seed)
    cams = VU.ring_cameras(V, seed + 1, twin)
    roots = rng.normal(0.0, 0.3, (R, 3)) + np.array([0.0, 0.0, 0.9])
    rel = rng.normal(0.0, 0.3, (R, J, 3))
    rel[:, ROOT] = 0.0
    truth = roots[:, None] + rel
    poses = (scale * rel[None] + rng.normal(0.0, 0.01, (V, R, J, 3))).astype(np.float32)
    poses[:, :, ROOT] = 0.0
    clean = np.stack([VU.project(truth, c)[0] for c in cams])
    kp = (clean + rng.normal(0.0, NOISE_PX, clean.shape)).astype(np.float32)
    flags = np.ones((V, R, J), np.uint8)
    edges = R >= 40
    if edges:
        kp[rng.uniform(size=(V, R, J)) < LOST] = np.nan
        flags[rng.uniform(size=(V, R, J)) < LOST] = 0
        for f in (TWIN, BEHIND, OUTLIER3, OUTLIER2, ONE, LOW, NO_ROOT):   # these frames: every joint seen by every view, apart from what follows
            kp[:, f] = (clean[:, f] + rng.normal(0.0, NOISE_PX, clean[:, f].shape)).astype(np.float32)
            flags[:, f] = 1
        flags[2:, TWIN, AT] = 0                                          # views 0 and 1 alone: with twin cameras, two rays that are one ray
        away = np.asarray(cams[0].translation) - truth[BEHIND, AT]        # 1.5 times the way to camera 0: all lines meet behind it
        kp[:, BEHIND, AT] = np.stack([VU.project(truth[BEHIND, AT] + 1.5 * away, c)[0] for c in cams]).astype(np.float32)
        flags[3:, OUTLIER3, AT] = 0                                      # three candidates, view 1 is 40 px off across the epipolar lines
        kp[min(1, V - 1), OUTLIER3, AT, 1] += OUTLIER_PX
        flags[2:, OUTLIER2, AT] = 0                                      # two candidates, one of them 40 px off: nothing is left to trust
        kp[min(1, V - 1), OUTLIER2, AT, 1] += OUTLIER_PX
        flags[1:, ONE, AT] = 0                                           # one candidate
        poses[:, ONE, AT, 1] = np.nan                                    # ... whose fused lift is NaN, and stays NaN
        flags[0, LOW, VU.min_joints(J) - 1:] = 0                         # view 0 keeps one joint too few: it does not SEE the frame
        flags[:, NO_ROOT, ROOT] = 0                                      # the root joint is lost: the frame stays lifted as a whole
    return dict(cams=cams, truth=truth, poses=poses, kp=kp, flags=flags, edges=edges, R=R, J=J, V=V, twin=twin)


@functools.lru_cache(maxsize=None)
def host_rules(R, J, V, twin=False, with_flags=True, min_views=2, max_residual=8.0, scale=1.1):
    """The mirrors on ``scene(R, J, V)``, computed once and shared; nobody writes to what this returns
    -> (the scene, fused, sees, X, count, placed, joint_views)."""
    from uplift_upsample_3dhpe_amd import predict
    s = scene(R, J, V, twin, scale)
    flags = s["flags"] if with_flags else None
    fused, _, sees = predict.fuse_views_host(s["poses"], s["kp"], flags, VU.min_joints(J))
    X, count = predict.triangulate_joints_host(s["kp"], s["cams"], sees, flags, max_residual, min_views)
    placed, joint_views = predict.place_joints_host(fused, X, count, ROOT)
    for a in (fused, sees, X, count, placed, joint_views, s["kp"], s["poses"], s["flags"], s["truth"]):
        a.setflags(write=False)
    return s, fused, sees, X, count, placed, joint_views
