"""Seeded scenes for tests/test_lift_match_cpu.py and tests/test_lift_match_gpu.py (include/uu3d.h, WHO IS WHO WITHOUT A WORLD), on the
ring cameras of tests/views_util.py and the walkers of tests/view_calibrate_util.py: every view holds a shuffled subset of the persons'
tracks, each track's lifts in that camera's OWN axes, so the true partition of the tracks is known.  ``shared_body`` is the hard scene:
all persons have ONE body and differ only in how they turn and in the phase of their limbs."""
import functools

import numpy as np

from tests import view_calibrate_util as CU
from tests import views_util as VU

ROOT = CU.ROOT


def shared_walkers(persons, T, J, rng):
    """``view_calibrate_util.walkers`` with ONE body and ONE set of limb directions for all persons: person i differs in the course of its
    turning, the phase of its limbs and its path -> the world joints (persons * T, J, 3) float64 and the root-relative skeletons in world
    axes, the persons back to back."""
    t = np.arange(T) / 50.0
    body = rng.normal(0.0, 0.25, (J, 3))
    body[ROOT] = 0.0
    limbs = rng.normal(0.0, 1.0, (J, 3))
    joints, rel = [], []
    for i in range(persons):
        swing = 0.08 * np.sin(2.0 * np.pi * 1.1 * t + 2.1 * i)[:, None, None] * limbs
        turn = (0.9 + 0.8 * i) * t + 0.6 * np.sin(0.7 * t + 1.3 * i) + 2.0 * i
        c, s = np.cos(turn), np.sin(turn)
        shape = body[None] + swing
        shape[:, ROOT] = 0.0
        r = np.stack([c[:, None] * shape[..., 0] - s[:, None] * shape[..., 1], s[:, None] * shape[..., 0] + c[:, None] * shape[..., 1], shape[..., 2]], -1)
        root = np.stack([0.9 * np.cos(0.8 * t + 2.5 * i) + 0.3 * i, 0.7 * np.sin(1.1 * t + 1.0 * i) - 0.2 * i, 0.9 + 0.05 * np.sin(3.0 * t)], -1)
        rel.append(r)
        joints.append(root[:, None] + r)
    return np.concatenate(joints), np.concatenate(rel)


def tracks_of(poses, kp, persons, T, who):
    """The view-major buffers of ``view_calibrate_util.scene`` cut into tracks: ``poses`` (V, persons * T, J, 3), ``kp`` (V, persons * T, J,
    2); ``who[v]``: the persons view v holds, in the order of its tracks -> (poses (M, T, J, 3) f32, kp (M, T, J, 2) f32, view_of (M,)
    i32, truth (M,): the true person of every track)."""
    J = poses.shape[2]
    lifts = poses.reshape(len(who), persons, T, J, 3)
    pixels = kp.reshape(len(who), persons, T, J, 2)
    view_of = np.repeat(np.arange(len(who), dtype=np.int32), [len(w) for w in who])
    truth = np.array([i for w in who for i in w], np.int64)
    return (np.ascontiguousarray(np.stack([lifts[v, i] for v, w in enumerate(who) for i in w])),
            np.ascontiguousarray(np.stack([pixels[v, i] for v, w in enumerate(who) for i in w])), view_of, truth)


def same_partition(person, truth):
    """Whether ``person`` (M,) groups the tracks exactly as ``truth`` (M,) does."""
    pairs = set(zip([int(k) for k in person], [int(k) for k in truth]))
    return len({g for g, _ in pairs}) == len(pairs) == len({w for _, w in pairs})


SHARED_WHO = [[2, 0, 1], [1, 2, 0], [0, 2]]                              # view 2 does not hold person 1; view 0 holds everybody


@functools.lru_cache(maxsize=None)
def shared_body(V=3, persons=3, T=129, J=17, scale=1.1, lift_noise=0.01, px_noise=0.5, seed=4711):
    """3 ring cameras, 3 persons with ONE body, 129 frames, lifts scaled by 1.1 with 1 cm of noise, pixels with 0.5 px of noise, the tracks
    shuffled per view, one camera missing one person.  Computed once and shared; nobody writes to what this returns
    -> dict: cams (the true cameras), bare (the same without extrinsics), poses (M, T, J, 3) f32, kp (M, T, J, 2) f32, view_of, truth,
    who, q and c (the true poses against camera 0), T, J, scale."""
    from uplift_upsample_3dhpe_amd import predict
    rng = np.random.default_rng(seed)
    cams = VU.ring_cameras(V, seed + 1)
    world, rel = shared_walkers(persons, T, J, rng)
    lifts = np.stack([predict.world_to_camera_host(rel + np.asarray(c.translation), c) for c in cams])      # rotated only
    poses = (scale * lifts + rng.normal(0.0, lift_noise, lifts.shape)).astype(np.float32)
    poses[:, :, ROOT] = 0.0
    clean = np.stack([VU.project(world, c)[0] for c in cams])
    kp = (clean + rng.normal(0.0, px_noise, clean.shape)).astype(np.float32)
    who = SHARED_WHO[:V]
    P, K, view_of, truth = tracks_of(poses, kp, persons, T, who)
    q, c = CU.true_poses(cams)
    for a in (P, K, view_of, truth, q, c):
        a.setflags(write=False)
    return dict(cams=cams, bare=[k.without(extrinsics=True) for k in cams], poses=P, kp=K, view_of=view_of, truth=truth, who=who, q=q, c=c, T=T, J=J,
                scale=scale, persons=persons)


def pair_rms(sums, terms, truth, view_of):
    """The root-mean-square joint distance of every pair of tracks of different views -> (the largest of the true pairs, the smallest of
    the wrong pairs), in the poses' units."""
    true, wrong = [], []
    for p in range(len(truth)):
        for q in range(p + 1, len(truth)):
            if view_of[p] != view_of[q] and terms[p, q] > 0:
                (true if truth[p] == truth[q] else wrong).append(float(np.sqrt(sums[p, q] / terms[p, q])))
    return max(true), min(wrong)


def random_inputs(view_of, T, J, seed, with_flags, lost=0.05):
    """Random lifts, keypoints with NaN and Inf sprinkled in and flags for the launch alone: ``view_calibrate_util.random_inputs`` with a
    track in the place of a view; with three or more tracks and T >= 255 nobody sees the last track
    -> (poses (M, T, J, 3) f32, kp (M, T, J, 2) f32, flags (M, T, J) u8 or None)."""
    poses, kp, flags, _ = CU.random_inputs(len(view_of), T, J, seed, with_flags, lost)
    return poses, kp, flags
