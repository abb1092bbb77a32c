"""The association stage of the track pipeline: per-frame person detections -> tracks and slots (include/uu3d.h, PER-FRAME DETECTIONS).
Wraps uu3d_associate_state_bytes and uu3d_associate_detections (``associate_detections``; the rule in numpy: ``AssociationHost`` /
``associate_host``, which is also the rule of a session's uu3d_stream_associate).

Per-frame detections: ``predict_detections(model, config, detections, counts, valid, slots=S)`` takes what a multi-person detector emits --
per frame a list of people in arbitrary order, (T_v, D, K, 2) per video -- associates people to tracks on the device
(uu3d_associate_detections; ``associate_detections``; the rule in numpy: ``associate_host`` / ``AssociationHost``: greedy, no motion model,
S, D, K <= 64) and calls ``predict_tracks`` on the tracks -> per video a list of (track_id, first_frame, poses).

Per-frame detections -- ``StreamSession(..., detections=D, max_age=, max_dist=, min_common=)``: the session takes what a multi-person
detector emits, ``push_detections(dets (D, K, 2), count, valid)`` -- per frame a list of people in ANY order, people entering, leaving and
being missed -- and matches people to slots on the device: ``slots`` is the capacity, a slot is born, fed and freed by the rule of
``predict.associate_host`` (include/uu3d.h, PER-FRAME DETECTIONS: greedy, no motion model).  The captured tick begins with
uu3d_stream_associate -- it scatters the detections into the session's frame, flag and ``active`` buffers and writes the ``born`` mask --,
then uu3d_stream_reset (and uu3d_stream_repair_reset) with that mask ON THE DEVICE, then the steps above unchanged: still ONE linear
captured graph, ``push_detections`` never waits, ``count`` may be a device tensor.  Implies ``missed_detections=True``: an alive slot
without a match gets a MISSING frame.  The contract: the session equals, bit for bit, a ``StreamSession(missed_detections=True)`` driven
by ``associate_host`` -- ``reset(born)``, then ``push(frames, active=alive, valid=matched)``.  Works with ``keypoints`` (the association
runs on the detector's joints, in front of the map) and ``repair_joints``; NOT together with ``fps`` / ``out_fps`` (ValueError: the host
mirror of the source counters cannot follow births that happen on the device yet)."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import ptr as _ptr
from .tracks import _host_array, _shape, _upload


MAX_ASSOCIATION = 64                                                  # the largest slots, detections per frame and joints (kAssocMax)
# conveniences, not tuned values: frames a track survives without a match, the largest normalised distance, the fewest common joints
ASSOCIATION_DEFAULTS = {"max_age": 10, "max_dist": 0.5, "min_common": 3}


class Association(object):
    """What ``associate_host`` (host arrays for ONE video) and ``associate_detections`` (lists with one device tensor per video) return --
        assignment (T, D) int32   the slot of each detection, -1: none (no candidate, or dropped)
        track_of   (T, D) int32   the track id of each detection, -1: none
        track_ids  (T, S) int32   the track in each slot after the frame, -1: a free slot
        born, alive (T, S) uint8  slots born at the frame; slots alive after it
        num_tracks, dropped       ids handed out (they are 0 .. num_tracks - 1) and detections dropped for want of a free slot: ints on
                                  the host; on the device ``counters`` (V, 2) int32 holds both per video
    and, from ``associate_host`` only, slot_det (T, S) int32: the detection that is the slot's frame of the tick (-1: none), and slot_full
    (T, S) bool: it has one and every joint flag of it is set."""

    def __init__(self, **fields):
        self.__dict__.update(fields)


def check_association(slots, detections, joints, max_age, max_dist, min_common):
    """The capacities (each in [1, 64]) and the three parameters of the rule: ValueError naming what is wrong."""
    for name, v in (("slots", slots), ("detections per frame", detections), ("joints", joints)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= MAX_ASSOCIATION:
            raise ValueError(f"{name} must be an int in [1, {MAX_ASSOCIATION}] (the association runs in one workgroup's LDS), got {v!r}")
    if isinstance(max_age, bool) or not isinstance(max_age, (int, np.integer)) or int(max_age) < 0:
        raise ValueError(f"max_age must be an int >= 0: frames a track survives without a match, got {max_age!r}")
    if isinstance(min_common, bool) or not isinstance(min_common, (int, np.integer)) or int(min_common) < 1:
        raise ValueError(f"min_common must be an int >= 1: joints a detection needs, and a pair needs in common, got {min_common!r}")
    if isinstance(max_dist, bool) or not isinstance(max_dist, (int, float, np.integer, np.floating)) or not float(max_dist) >= 0.0:
        raise ValueError(f"max_dist must be a number >= 0: the largest normalised distance of a match, got {max_dist!r}")


def _association_options(options):
    """max_age / max_dist / min_common out of keyword options, the defaults where one is not given -> (the three, the other options)."""
    rest = dict(options)
    return {k: rest.pop(k, v) for k, v in ASSOCIATION_DEFAULTS.items()}, rest


def _detection_flags(valid, T, D, K):
    """``valid`` of one video -> (frame flags (T, D) bool, joint flags (T, D, K) bool): None / "finite" = every flag set (the finite test
    always applies), (T, D) = one flag per detection, (T, D, K) = one per joint."""
    if valid is None or (isinstance(valid, str) and valid == "finite"):
        return np.ones((T, D), bool), np.ones((T, D, K), bool)
    v = _host_array(valid) != 0
    if v.shape == (T, D):
        return v, np.ones((T, D, K), bool)
    if v.shape == (T, D, K):
        return np.ones((T, D), bool), v
    raise ValueError(f"valid must be None, ({T}, {D}) or ({T}, {D}, {K}), got {v.shape}")


class AssociationHost(object):
    """The rule of PER-FRAME DETECTIONS (include/uu3d.h) in numpy, written to be read, one frame per ``step``: the state machine that
    uu3d_associate_detections and uu3d_stream_associate run, bit for bit.  State per slot: ``alive``, ``track`` (-1: free), ``age``
    (consecutive frames without a match), ``ref`` (K, 2) float32 with ``seen`` (K,): the last observed position of each joint since the
    slot's birth; ``next_id``, ``dropped``.  Greedy, no motion model, no Hungarian step: the simplest rule that can be stated exactly."""

    def __init__(self, slots, detections, joints, max_age=10, max_dist=0.5, min_common=3):
        check_association(slots, detections, joints, max_age, max_dist, min_common)
        self.S, self.D, self.K = int(slots), int(detections), int(joints)
        self.max_age, self.min_common = int(max_age), int(min_common)
        self.max_dist2 = np.float64(max_dist) * np.float64(max_dist)  # the right side of the test, computed once
        S, K = self.S, self.K
        self.alive, self.track, self.age = np.zeros(S, bool), np.full(S, -1, np.int64), np.zeros(S, np.int64)
        self.ref, self.seen = np.zeros((S, K, 2), np.float32), np.zeros((S, K), bool)
        self.next_id = self.dropped = 0

    def end(self, slots=None):
        """``uu3d_associate_reset``: the tracks in the given slots end (None: all of them, and the two counters start again)."""
        which = slice(None) if slots is None else np.asarray(slots, np.int64).reshape(-1)
        self.alive[which], self.track[which], self.age[which], self.seen[which] = False, -1, 0, False
        if slots is None:
            self.next_id = self.dropped = 0

    def step(self, det, count=None, frame_flag=None, joint_flag=None):
        """One frame: ``det`` (D, K, 2) float32, ``count`` given rows (None: D), ``frame_flag`` (D,) / ``joint_flag`` (D, K) bools or None
        -> (det_slot (D,) the assignment, slot_det (S,) the detection that is each slot's frame of this tick or -1, born (S,) bool)."""
        S, D, K, min_common = self.S, self.D, self.K, self.min_common
        alive, track, age, ref, seen = self.alive, self.track, self.age, self.ref, self.seen
        det = np.asarray(det, np.float32).reshape(D, K, 2)
        frame_flag = np.ones(D, bool) if frame_flag is None else np.asarray(frame_flag).reshape(D) != 0
        joint_flag = np.ones((D, K), bool) if joint_flag is None else np.asarray(joint_flag).reshape(D, K) != 0
        observed = joint_flag & np.isfinite(det).all(axis=2)
        cand = (np.arange(D) < (D if count is None else min(max(int(count), 0), D))) & frame_flag & (observed.sum(axis=1) >= min_common)
        # 1. the cost of every (alive slot, candidate) pair: the joint sum is an explicit left-to-right accumulation in float64 (np.sum
        #    adds pairwise), every product and sum rounded; unobserved joints never enter it
        cost, allowed = np.zeros((S, D), np.float64), np.zeros((S, D), bool)
        det64, ref64 = det.astype(np.float64), ref.astype(np.float64)
        d2, common = np.zeros((S, D), np.float64), np.zeros((S, D), np.int64)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            for j in range(K):
                both = seen[:, None, j] & observed[None, :, j]
                dx = det64[None, :, j, 0] - ref64[:, None, j, 0]
                dy = det64[None, :, j, 1] - ref64[:, None, j, 1]
                d2 = np.where(both, d2 + (dx * dx + dy * dy), d2)
                common += both
            for s in np.flatnonzero(alive & seen.any(axis=1)):
                box = ref[s][seen[s]]                                   # the bounding box of the slot's seen reference joints
                w = np.float64(box[:, 0].max()) - np.float64(box[:, 0].min())
                h = np.float64(box[:, 1].max()) - np.float64(box[:, 1].min())
                scale2 = w * w + h * h
                if scale2 == 0:
                    continue
                pairs = cand & (common[s] >= min_common)
                cost[s, pairs] = d2[s, pairs] / (common[s, pairs].astype(np.float64) * scale2)
                allowed[s] = pairs & (cost[s] <= self.max_dist2)
        # 2. greedy: the smallest allowed cost among unmatched slots and candidates; ties to the smaller s, then the smaller d
        slot_det, det_slot = np.full(S, -1, np.int64), np.full(D, -1, np.int64)
        while True:
            open_pairs = allowed & (slot_det < 0)[:, None] & (det_slot < 0)[None, :]
            if not open_pairs.any():
                break
            s, d = divmod(int(np.flatnonzero(open_pairs)[np.argmin(cost[open_pairs])]), D)      # (row-major: the first minimum)
            slot_det[s], det_slot[d] = d, s
        # 3. / 4. matched slots are young again; unmatched ones age and die
        born = np.zeros(S, bool)
        for s in np.flatnonzero(alive):
            if slot_det[s] >= 0:
                age[s] = 0
            else:
                age[s] += 1
                if age[s] > self.max_age:
                    alive[s], track[s], age[s], seen[s] = False, -1, 0, False
        # 5. births: unmatched candidates in ascending d take the lowest free slot (one that has just died included)
        for d in np.flatnonzero(cand & (det_slot < 0)):
            free = np.flatnonzero(~alive)
            if len(free) == 0:
                self.dropped += 1
                continue
            s = int(free[0])
            alive[s], born[s], track[s], age[s], seen[s] = True, True, self.next_id, 0, False
            slot_det[s], det_slot[d] = d, s
            self.next_id += 1
        # 3. / 5. the reference pose takes the bits of the joints observed in the slot's detection
        for s in np.flatnonzero(slot_det >= 0):
            o = observed[slot_det[s]]
            ref[s][o] = det[slot_det[s]][o]
            seen[s] |= o
        return det_slot, slot_det, born


def associate_host(dets, counts=None, valid=None, slots=None, max_age=10, max_dist=0.5, min_common=3):
    """``AssociationHost`` over ONE whole video: what uu3d_associate_detections computes, bit for bit.  ``dets`` (T, D, K, 2): per frame
    the people a detector listed, in any order; ``counts`` (T,) or None = D: how many rows of each frame are given; ``valid``: None,
    (T, D) or (T, D, K) flags; ``slots`` = S (None: D) -> an ``Association`` of host arrays."""
    dets = np.asarray(_host_array(dets), np.float32)
    if dets.ndim != 4 or dets.shape[3] != 2:
        raise ValueError(f"dets must be (T, D, K, 2), got {dets.shape}")
    T, D, K = (int(n) for n in dets.shape[:3])
    rule = AssociationHost(D if slots is None else slots, D, K, max_age, max_dist, min_common)
    S = rule.S
    counts = np.full(T, D, np.int64) if counts is None else np.asarray(_host_array(counts), np.int64).reshape(-1)
    if len(counts) != T:
        raise ValueError(f"counts must have one entry per frame: {T} frames, {len(counts)} entries")
    frame_flag, joint_flag = _detection_flags(valid, T, D, K)
    out = {k: np.full((T, n), -1, np.int32) for k, n in (("assignment", D), ("track_of", D), ("track_ids", S), ("slot_det", S))}
    out.update({k: np.zeros((T, S), np.uint8) for k in ("born", "alive")})
    out["slot_full"] = np.zeros((T, S), bool)
    for t in range(T):
        det_slot, slot_det, born = rule.step(dets[t], counts[t], frame_flag[t], joint_flag[t])
        out["assignment"][t], out["slot_det"][t], out["track_ids"][t] = det_slot, slot_det, rule.track
        out["track_of"][t] = np.where(det_slot >= 0, rule.track[np.maximum(det_slot, 0)], -1)
        out["born"][t], out["alive"][t] = born, rule.alive
        out["slot_full"][t] = (slot_det >= 0) & joint_flag[t][np.maximum(slot_det, 0)].all(axis=1)
    return Association(num_tracks=rule.next_id, dropped=rule.dropped, **out)


def association_tracks_host(dets, valid, result):
    """The tracks of one video out of ``associate_host``'s result, as ``predict_detections`` builds them on the device -> list of
    (track_id, first_frame, coordinates (n, K, 2) float32, joint flags (n, K) bool), by track id: a track runs from its birth frame to
    its last matched frame; a frame in between without a match is missing (zeros, no flag set)."""
    dets = np.asarray(_host_array(dets), np.float32)
    T, D, K = dets.shape[:3]
    _, joint_flag = _detection_flags(valid, T, D, K)
    tracks = []
    for tid in range(result.num_tracks):
        frames, which = np.nonzero(result.track_of == tid)
        first, n = int(frames[0]), int(frames[-1]) - int(frames[0]) + 1
        xy, flags = np.zeros((n, K, 2), np.float32), np.zeros((n, K), bool)
        xy[frames - first], flags[frames - first] = dets[frames, which], joint_flag[frames, which]
        tracks.append((tid, first, xy, flags))
    return tracks


def _device_detections(detections, counts, valid, device):
    """The videos' detections on the device, back to back -> (dets (F, D, K, 2) f32, counts (F,) i32 or None, flags u8 or None, whether
    the flags are per joint, frames per video)."""
    import torch
    vids = []
    for v in detections:
        v = v.to(device=device, dtype=torch.float32) if isinstance(v, torch.Tensor) else _upload(np.asarray(v), np.float32, device)
        if v.dim() != 4 or v.shape[3] != 2:
            raise ValueError(f"a video's detections must be (T, D, K, 2), got {tuple(v.shape)}")
        vids.append(v)
    if not vids:
        raise ValueError("no videos")
    D, K = int(vids[0].shape[1]), int(vids[0].shape[2])
    if any(tuple(v.shape[1:3]) != (D, K) for v in vids):
        raise ValueError("all videos must have the same detections per frame and joints")
    lens = np.array([int(v.shape[0]) for v in vids], np.int64)
    if (lens < 1).any():
        raise ValueError("every video needs at least one frame")
    dets = (torch.cat(vids, 0) if len(vids) > 1 else vids[0]).contiguous()
    d_counts = None
    if counts is not None:
        if len(counts) != len(vids) or any(_shape(c) != (int(n),) for c, n in zip(counts, lens)):
            raise ValueError("counts must be None or a list with one (T_v,) entry per video")
        parts = [c.to(device=device, dtype=torch.int32) if isinstance(c, torch.Tensor) else _upload(np.asarray(c), np.int32, device) for c in counts]
        d_counts = torch.cat(parts, 0).contiguous()
    flags, per_joint = None, False
    if valid is not None and not isinstance(valid, str):
        if not isinstance(valid, (list, tuple)) or len(valid) != len(vids):
            raise ValueError('valid must be None, "finite" or a list with one (T_v, D) or (T_v, D, K) entry per video')
        shapes = [_shape(f) for f in valid]
        per_joint = any(len(sh) == 3 for sh in shapes)
        for sh, n in zip(shapes, lens):
            if sh != (int(n), D) and sh != (int(n), D, K):
                raise ValueError(f"an entry of valid must be ({int(n)}, {D}) or ({int(n)}, {D}, {K}), got {sh}")
        parts = []
        for f in valid:
            f = ((f if f.is_cuda else f.contiguous().pin_memory().to(device, non_blocking=True)) != 0).to(torch.uint8) if isinstance(f, torch.Tensor) \
                else _upload(np.asarray(f) != 0, np.uint8, device)
            parts.append(f.reshape(f.shape[0], D, 1).expand(-1, -1, K) if per_joint and f.dim() == 2 else f)
        flags = torch.cat(parts, 0).contiguous()
    elif valid is not None and valid != "finite":
        raise ValueError('valid must be None, "finite" or a list with one (T_v, D) or (T_v, D, K) entry per video')
    return dets, d_counts, flags, per_joint, lens


def associate_detections(detections, counts=None, valid=None, slots=None, max_age=10, max_dist=0.5, min_common=3, device="cuda"):
    """``associate_host`` on the device for a list of videos (uu3d_associate_detections: one launch, one workgroup per video).
    ``detections``: list of (T_v, D, K, 2) arrays or tensors, on the host or the device; ``counts``: None or a list of (T_v,) ints;
    ``valid``: None, "finite" or a list of (T_v, D) / (T_v, D, K) flags -> an ``Association`` whose fields are lists with one device
    tensor per video, and ``counters`` (V, 2) int32 on the device: (tracks, dropped) per video.  Nothing waits for the device."""
    import torch
    lib = _capi.load_library()
    device = torch.device(device)
    shape = _shape(detections[0]) if len(detections) else (0, 1, 1, 2)
    if len(shape) == 4:
        check_association(shape[1] if slots is None else slots, int(shape[1]), int(shape[2]), max_age, max_dist, min_common)
    dets, d_counts, flags, per_joint, lens = _device_detections(detections, counts, valid, device)
    F, D, K = int(dets.shape[0]), int(dets.shape[1]), int(dets.shape[2])
    S, V = D if slots is None else int(slots), len(lens)
    params = _capi.Uu3dAssociateParams(S, D, K, int(max_age), int(min_common), 0, float(max_dist))
    start = _upload(np.concatenate([[0], np.cumsum(lens)]), np.int64, device)
    state = torch.zeros((V * int(lib.uu3d_associate_state_bytes(S, K)),), dtype=torch.uint8, device=device)
    i32 = lambda n: torch.empty((F, n), dtype=torch.int32, device=device)
    u8 = lambda n: torch.empty((F, n), dtype=torch.uint8, device=device)
    assignment, track_of, track_ids, born, alive = i32(D), i32(D), i32(S), u8(S), u8(S)
    counters = torch.empty((V, 2), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        _capi.check(lib, lib.uu3d_associate_detections(C.byref(params), _ptr(dets), _ptr(d_counts), _ptr(flags), int(per_joint), _ptr(start), V, F,
                                                       _ptr(state), _ptr(assignment), _ptr(track_of), _ptr(track_ids), _ptr(born), _ptr(alive),
                                                       _ptr(counters), C.c_void_p(stream)), None)
    split = lambda a: list(torch.split(a, [int(n) for n in lens], 0))
    r = Association(assignment=split(assignment), track_of=split(track_of), track_ids=split(track_ids), born=split(born), alive=split(alive),
                    counters=counters)
    r._flat = (dets, flags, per_joint, lens, track_of)
    return r
