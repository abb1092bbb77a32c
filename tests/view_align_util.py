"""Seeded scenes for tests/test_view_align_cpu.py and tests/test_view_align_gpu.py (include/uu3d.h, ONE CLOCK), built on
``tests/views_util.ring_cameras`` and ``project``: P persons stand on the steps of ``tests/view_match_util`` and SWAY -- every body centre
moves by ``SWAY`` m * sin(2 pi t / period + phase) per axis, periods of 35 to 90 frames --, V cameras on a ring film them, and every view
is cut from the common timeline at its own offset and length: view v's frame f is the common frame f + offsets[v] - min(offsets).  The
linear walk of ``view_match_util`` would not do: one frame of lag moves a joint less than the pixel noise there.  Lost joints appear as
NaN and as cleared flags."""
import numpy as np

from tests import views_util as VU
from tests.view_match_util import NOISE_PX, SPACING, STEP

SWAY = 0.3


def persons_world(P, T, K, seed):
    """P persons -> (P, T, K, 3) float64 world joints on a common timeline of T frames."""
    rng = np.random.default_rng(seed)
    out = np.empty((P, T, K, 3), np.float64)
    t = np.arange(T)[:, None]
    for i in range(P):
        ang = 2.0 * np.pi * i / max(P, 3) + 0.4
        centre = np.array([np.cos(ang), np.sin(ang), 0.0]) * SPACING / (2.0 * np.sin(np.pi / max(P, 3))) + np.array([0.0, 0.0, 0.9 + STEP * i])
        body = rng.normal(0.0, 0.25, (K, 3))
        period, phase = rng.uniform(35.0, 90.0, 3), rng.uniform(0.0, 2.0 * np.pi, 3)
        sway = SWAY * np.sin(2.0 * np.pi * t / period + phase)           # (T, 3)
        out[i] = centre + body + sway[:, None, :] + rng.normal(0.0, 0.004, (T, K, 3))
    return out


def scene(offsets, lengths, P, K, seed, counts=None, lost=0.04, noise=NOISE_PX, distortion=None, twin=False, still=False):
    """``offsets`` / ``lengths``: per view -> (cameras, views, truth, valid): ``views[v]`` a list of (lengths[v], K, 2) float32 tracks, all
    P persons in order, or with ``counts`` a shuffled subset of counts[v] of them; ``truth[v]`` the true person of each; ``valid[v]`` per
    track (T_v, K) uint8 flags.  ``still``: nobody moves, nothing is noisy and no joint is lost -- every frame of a track is the same frame."""
    from uplift_upsample_3dhpe_amd import predict
    rng = np.random.default_rng(seed)
    V = len(offsets)
    cams = VU.ring_cameras(V, seed + 1, twin, distortion)
    base = min(offsets)
    Tc = max(n + o - base for n, o in zip(lengths, offsets))
    world = persons_world(P, Tc, K, seed + 2)
    if still:
        world[:] = world[:, :1]
        noise, lost = 0.0, 0.0
    views, truth, valid = [], [], []
    for v in range(V):
        who = list(range(P)) if counts is None else [int(i) for i in rng.permutation(P)[:counts[v]]]
        start, T = offsets[v] - base, lengths[v]
        tracks, flags = [], []
        for i in who:
            px = VU.project(world[i, start:start + T], cams[v])[0] + rng.normal(0.0, noise, (T, K, 2))
            if cams[v].has_distortion:
                px = predict.distort_points_host(px, cams[v])
            px = px.astype(np.float32)
            f = np.ones((T, K), np.uint8)
            if T * K >= 40 and lost > 0:
                px[rng.uniform(size=(T, K)) < lost] = np.nan
                f[rng.uniform(size=(T, K)) < lost] = 0
            tracks.append(px)
            flags.append(f)
        views.append(tracks)
        truth.append(who)
        valid.append(flags)
    return cams, views, truth, valid


def stacked(views, valid=None):
    """The view-major arrays of the launches -> (kp (rows, K, 2) f32, view_of (M,) i32, frames (M,) i64, flags (rows, K) u8 or None)."""
    flat = [t for tracks in views for t in tracks]
    kp = np.ascontiguousarray(np.concatenate(flat).astype(np.float32))
    view_of = np.repeat(np.arange(len(views), dtype=np.int32), [len(v) for v in views])
    frames = np.array([len(t) for t in flat], np.int64)
    flags = None if valid is None else np.ascontiguousarray(np.concatenate([f for per_view in valid for f in per_view]).astype(np.uint8))
    return kp, view_of, frames, flags


def score_ratio(sums, terms, view_of, V, L, min_terms, same_index, true_offsets):
    """Per later view: the smallest score among the WRONG lags over the score at the true lag, from ``view_offsets_host`` on the tables
    with one lag left at a time -- how decisive the minimum is."""
    from uplift_upsample_3dhpe_amd import predict
    ratios = []
    for w in range(1, V):
        true = true_offsets[w] - true_offsets[0]
        keep = np.zeros_like(terms)
        keep[:, :, true + L] = terms[:, :, true + L]
        at_true = predict.view_offsets_host(sums, keep, view_of, V, L, min_terms, same_index)[2][w]
        wrong = terms.copy()
        wrong[:, :, true + L] = 0
        off, state, score = predict.view_offsets_host(sums, wrong, view_of, V, L, min_terms, same_index)
        assert state[w] == 1 and off[w] != true
        ratios.append(float(score[w] / at_true))
    return ratios
