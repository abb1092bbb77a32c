"""Seeded scenes for tests/test_view_match_cpu.py and tests/test_view_match_gpu.py (include/uu3d.h, WHO IS WHO), built on
``tests/views_util.ring_cameras`` and ``project``: P true persons with known spacing walk near the origin, V cameras on a ring see them,
and each view holds a shuffled subset of the persons -- so the true partition of the tracks is known.  Lost joints appear as NaN and as
cleared flags.  The persons stand ``SPACING`` apart on a circle and on steps of ``STEP`` height: ring cameras at one height look along
nearly horizontal rays, whose common normal is nearly vertical, so two different persons at one height would be told apart only by their
skeletons -- the steps make the distance between a wrong pair's lines a matter of the scene, not of chance."""
import numpy as np

from tests import views_util as VU

SPACING, STEP, NOISE_PX = 1.2, 0.6, 0.5


def persons_world(P, T, K, seed):
    """P persons -> (P, T, K, 3) float64 world joints: a random skeleton of about 0.5 m around a body centre that walks slowly."""
    rng = np.random.default_rng(seed)
    out = np.empty((P, T, K, 3), np.float64)
    t = np.arange(T)[:, None, None]
    for i in range(P):
        ang = 2.0 * np.pi * i / max(P, 3) + 0.4
        centre = np.array([np.cos(ang), np.sin(ang), 0.0]) * SPACING / (2.0 * np.sin(np.pi / max(P, 3))) + np.array([0.0, 0.0, 0.9 + STEP * i])
        body = rng.normal(0.0, 0.25, (K, 3))
        out[i] = centre + body + t * np.array([0.004, -0.003, 0.0]) * (1 + i) + rng.normal(0.0, 0.004, (T, K, 3))
    return out


def scene(counts, P, T, K, seed, twin=False, lost=0.04, noise=NOISE_PX, distortion=None):
    """``counts``: tracks per view (each <= P) -> (cameras, views, truth, valid): ``views[v]`` a list of counts[v] (T, K, 2) float32
    tracks, a shuffled subset of the persons; ``truth[v]``: the true person of each of them; ``valid[v]``: per track (T, K) uint8 flags.
    Lost joints: ``lost`` of all as NaN, as many as cleared flags.  ``distortion``: None or {view: coefficients}; such a view's pixels are
    those its lens would have produced."""
    from uplift_upsample_3dhpe_amd import predict
    rng = np.random.default_rng(seed)
    V = len(counts)
    cams = VU.ring_cameras(V, seed + 1, twin, distortion)
    world = persons_world(P, T, K, seed + 2)
    views, truth, valid = [], [], []
    for v, n in enumerate(counts):
        who = [int(i) for i in rng.permutation(P)[:n]]
        tracks, flags = [], []
        for i in who:
            px = VU.project(world[i], cams[v])[0] + rng.normal(0.0, noise, (T, K, 2))
            if cams[v].has_distortion:
                px = predict.distort_points_host(px, cams[v])
            px = px.astype(np.float32)
            if T * K >= 40:
                px[rng.uniform(size=(T, K)) < lost] = np.nan
            f = np.ones((T, K), np.uint8)
            if T * K >= 40:
                f[rng.uniform(size=(T, K)) < lost] = 0
            tracks.append(px)
            flags.append(f)
        views.append(tracks)
        truth.append(who)
        valid.append(flags)
    return cams, views, truth, valid


def same_partition(person, truth):
    """Whether the per-view lists ``person`` (what the match returned) group the tracks exactly as ``truth`` does."""
    got = [k for per_view in person for k in per_view]
    want = [k for per_view in truth for k in per_view]
    if len(got) != len(want):
        return False
    pairs = set(zip(got, want))
    return len({g for g, _ in pairs}) == len(pairs) == len({w for _, w in pairs})


def stacked(views, valid=None):
    """The view-major arrays of the launches -> (kp (M, T, K, 2) f32, view_of (M,) i32, flags (M, T, K) u8 or None)."""
    kp = np.stack([t for tracks in views for t in tracks]).astype(np.float32)
    view_of = np.repeat(np.arange(len(views), dtype=np.int32), [len(v) for v in views])
    flags = None if valid is None else np.stack([f for per_view in valid for f in per_view]).astype(np.uint8)
    return np.ascontiguousarray(kp), view_of, flags


def vanishing_tracks(cams, T, K, seed):
    """Two tracks whose rays are parallel: in cameras 0 and 1 the pixels of the vanishing points of K world directions (jittered per frame
    by the same direction in both cameras), so every pair of rays has cc far below ``VIEW_PARALLEL`` pp qq and no term counts."""
    rng = np.random.default_rng(seed)
    towards = -(np.asarray(cams[0].translation) + np.asarray(cams[1].translation))        # into the scene: in front of both cameras
    towards /= np.linalg.norm(towards)
    D = towards + rng.normal(0.0, 0.05, (T, K, 3))
    return [VU.project(np.asarray(c.translation) + D, c)[0].astype(np.float32) for c in cams[:2]]
