"""The validity stage of the track pipeline: which frames and joints were observed, and the repair of joints the detector lost.  Wraps
uu3d_repair_joints (``repair_joints``; the rule in numpy: ``repair_joints_host``; its live form, uu3d_stream_repair_stage, in numpy:
``LiveRepairHost``) and prepares the ``valid_in`` flags of uu3d_normalize_tracks_valid / uu3d_resample_tracks (``_front_validity``).

Per-joint missed detections: ``predict_tracks(..., valid=..., repair_joints=G)`` fills a joint the detector lost for up to G frames by
linear interpolation between the nearest frames where it was seen (uu3d_repair_joints, in front of the two front kernels above; the rule
in numpy: ``repair_joints_host``) instead of giving up the whole frame.

Live per-joint missed detections -- ``StreamSession(..., repair_joints=G)``: ``push(valid=...)`` takes one flag per JOINT and a joint the
detector lost is filled by the rule of ``predict.repair_joints_host``.  The one rule above is unchanged: the pose of frame t - lookahead is
what ``predict_tracks(track[:t + 1], valid=flags[:t + 1], repair_joints=G)`` gives for it -- a closed gap interpolated, a trailing or leading
gap held for up to G frames.  The rule looks ahead, so a push may REVISE frames the session has filed, within bounds:
  near    coordinates change only for frames t - G .. t (a gap of at most G frames closes at t: held -> interpolated; a joint is seen for
          the first time at t: unfilled -> held from t).  Of those the ring keeps the multiples of s_in and the edge frame, at most
          K = G // s_in + 2 frames: the tick re-stages them (uu3d_stream_repair_stage), runs uu3d_frame_features over slots x K (x 2
          with flip) frames and files K rows (uu3d_stream_commit_repair).
  far     an older frame only ever goes from valid to missing (a gap longer than G closes at t: the frames held from its left end become
          unfillable): a byte of the validity state, no features.
The state this needs is bounded; ``LiveRepairHost`` is the state machine the device runs, in numpy.  G <= 32 (``MAX_LIVE_REPAIR``: K and
the buffers are fixed at construction).  Not together with ``fps`` / ``out_fps``: a revised source frame would re-make model frames that
were filed already (a later change).  ``repair_joints=None`` is the session above, bit for bit."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import ptr as _ptr
from .tracks import _shape, _upload


def check_valid(valid, given, joints=None):
    """``predict_tracks``' ``valid`` argument against the frames given per track (``given``; keyframes with ``keyframes_only``): None,
    "finite" or one (T_i,) array / tensor per track -- with ``joints`` = J (``predict_tracks``) an entry may also be (T_i, J), one flag per
    joint; without it (a session, ``replay_tracks``) only (T_i,) passes.  Shapes only: nothing touches a device."""
    if valid is None or (isinstance(valid, str) and valid == "finite"):
        return
    if isinstance(valid, str) or not isinstance(valid, (list, tuple)):
        raise ValueError('valid must be None, "finite" or a list with one (T_i,) array per track')
    if len(valid) != len(given):
        raise ValueError(f"valid must have one entry per track: {len(given)} tracks, {len(valid)} entries")
    for i, (v, n) in enumerate(zip(valid, given)):
        shape = _shape(v)
        if shape != (int(n),) and (joints is None or shape != (int(n), int(joints))):
            per_joint = "" if joints is None else f" or ({int(n)}, {int(joints)}): one per joint"
            raise ValueError(f"valid[{i}] must be ({int(n)},): one flag per given frame of track {i}{per_joint}, got {shape}")


def check_repair_joints(repair_joints, valid):
    """``predict_tracks``' ``repair_joints`` argument: None, or an int G >= 1 together with ``valid``."""
    if repair_joints is None:
        return
    if isinstance(repair_joints, bool) or not isinstance(repair_joints, (int, np.integer)) or int(repair_joints) < 1:
        raise ValueError(f"repair_joints must be None or an int >= 1: the longest run of frames a joint is filled over, got {repair_joints!r}")
    if valid is None:
        raise ValueError('repair_joints needs valid: "finite" or per-frame / per-joint flags say which joints were observed')


def _device_valid(valid, device):
    """The list form of ``valid`` -> one (sum of given frames,) uint8 device tensor; host arrays go up in one pinned, asynchronous copy.
    A (T_i, J) entry counts per frame here: all of its joints."""
    import torch

    def frames(v):
        v = np.asarray(v) != 0
        return v.all(axis=1) if v.ndim == 2 else v.reshape(-1)
    if not any(isinstance(v, torch.Tensor) for v in valid):
        return _upload(np.concatenate([frames(v) for v in valid]).view(np.uint8), np.uint8, device)
    parts = []
    for v in valid:
        if isinstance(v, torch.Tensor):
            v = v if v.is_cuda else v.contiguous().pin_memory().to(device, non_blocking=True)
            v = v != 0
            parts.append((v.all(dim=1) if v.dim() == 2 else v).to(device=device, dtype=torch.uint8))
        else:
            parts.append(_upload(frames(v).view(np.uint8), np.uint8, device))
    return torch.cat(parts, 0)


def _device_joint_flags(valid, J, device):
    """The list form of ``valid`` -> one (sum of given frames, J) uint8 device tensor, one flag per joint; a (T_i,) entry stands for all
    joints of its frames.  Host arrays go up in one pinned, asynchronous copy."""
    import torch

    def joints(v):
        v = np.asarray(v) != 0
        return v if v.ndim == 2 else np.repeat(v.reshape(-1, 1), J, axis=1)
    if not any(isinstance(v, torch.Tensor) for v in valid):
        return _upload(np.concatenate([joints(v) for v in valid], 0).view(np.uint8), np.uint8, device)
    parts = []
    for v in valid:
        if isinstance(v, torch.Tensor):
            v = v if v.is_cuda else v.contiguous().pin_memory().to(device, non_blocking=True)
            v = (v != 0).to(device=device, dtype=torch.uint8)
            parts.append(v if v.dim() == 2 else v.reshape(-1, 1).expand(-1, J))
        else:
            parts.append(_upload(joints(v).view(np.uint8), np.uint8, device))
    return torch.cat(parts, 0).contiguous()


def repair_joints_host(tracks, joint_flags, G):
    """The rule of ``predict_tracks(repair_joints=G)`` (include/uu3d.h, PER-JOINT MISSED DETECTIONS) in numpy, written to be read: what
    uu3d_repair_joints computes, bit for bit.  ``tracks``: list of (T_i, J, 2) arrays; ``joint_flags``: None (no flags given: the finite test
    alone) or a list with one (T_i,) or (T_i, J) array per track -> (repaired, frame_flags, state): per track (T_i, J, 2) float32,
    (T_i,) bool and (T_i, J) uint8 (1 observed, 2 filled, 0 neither).  Nothing crosses a track boundary."""
    G = int(G)
    if G < 1:
        raise ValueError("G must be >= 1")
    repaired, frame_flags, states = [], [], []
    for i, track in enumerate(tracks):
        src = np.asarray(track, np.float32)
        T, J = src.shape[:2]
        observed = np.isfinite(src).all(axis=2)
        if joint_flags is not None:
            f = np.asarray(joint_flags[i]) != 0
            observed &= f if f.ndim == 2 else f[:, None]
        out = np.zeros((T, J, 2), np.float32)
        state = np.zeros((T, J), np.uint8)
        for j in range(J):
            seen = np.flatnonzero(observed[:, j])
            for t in range(T):
                if observed[t, j]:
                    out[t, j], state[t, j] = src[t, j], 1
                    continue
                before, after = seen[seen < t], seen[seen > t]
                l = int(before[-1]) if len(before) else None
                r = int(after[0]) if len(after) else None
                if l is not None and r is not None:
                    if r - l - 1 <= G:
                        w = np.float64(t - l) / np.float64(r - l)
                        out[t, j] = (src[l, j].astype(np.float64) * (1.0 - w) + src[r, j].astype(np.float64) * w).astype(np.float32)
                        state[t, j] = 2
                elif r is not None:
                    if r - t <= G:
                        out[t, j], state[t, j] = src[r, j], 2
                elif l is not None:
                    if t - l <= G:
                        out[t, j], state[t, j] = src[l, j], 2
        repaired.append(out)
        states.append(state)
        frame_flags.append((state == 1).any(axis=1) & (state != 0).all(axis=1))
    return repaired, frame_flags, states


def repair_joints(src, lens, G, joint_flags=None):
    """uu3d_repair_joints on the current stream.  ``src`` (R, J, 2) float32 on the device, the given frames of all tracks back to back
    (only read); ``lens``: given frames per track; ``joint_flags`` (R, J) uint8 on the device or None -> (repaired (R, J, 2) float32,
    frame flags (R,) uint8, joint state (R, J) uint8), fresh device buffers."""
    import torch
    lib = _capi.load_library()
    dev = src.device
    lens = np.asarray(lens, np.int64)
    R, J = int(src.shape[0]), int(src.shape[1])
    if int(lens.sum()) != R:
        raise ValueError("lens must add up to the rows of src")
    track_start = _upload(np.concatenate([[0], np.cumsum(lens)]), np.int64, dev)
    out = torch.empty((R, J, 2), dtype=torch.float32, device=dev)
    frame_flags = torch.empty((R,), dtype=torch.uint8, device=dev)
    state = torch.empty((R, J), dtype=torch.uint8, device=dev)
    nbytes = int(lib.uu3d_repair_joints_scratch_bytes(R, J))
    if nbytes == 0:
        raise ValueError(f"{R} frames of {J} joints are out of uu3d_repair_joints' range")
    scratch = torch.empty((nbytes // 4,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(lib, lib.uu3d_repair_joints(_ptr(src), R, J, _ptr(joint_flags), _ptr(track_start), len(lens), min(int(G), 2 ** 31 - 1), _ptr(out),
                                                _ptr(frame_flags), _ptr(state), _ptr(scratch), nbytes, C.c_void_p(stream)), None)
    return out, frame_flags, state


def _source_joint_flags(valid, J, device):
    """``valid`` behind the keypoint map -> the (given frames, J) uint8 per-joint flags on the device, or None where the finite test alone
    says which joints were observed (None, "finite")."""
    return None if valid is None or isinstance(valid, str) else _device_joint_flags(valid, J, device)


def _front_validity(src, given, J, valid, repair, joint_flags=None):
    """What the front kernels take as source and ``valid_in``: as they are, or with ``repair`` = G the repaired source and the frame
    flags of uu3d_repair_joints -> (src, valid_in, joint state or None).  ``joint_flags``: ``_source_joint_flags`` where the caller has
    made them already."""
    if repair is None:
        return src, None if valid is None or isinstance(valid, str) else _device_valid(valid, src.device), None
    return repair_joints(src, given, repair, _source_joint_flags(valid, J, src.device) if joint_flags is None else joint_flags)


MAX_LIVE_REPAIR = 32                                                  # the largest repair_joints of a live session (kLiveRepairMaxGap)


def staged_frames(repair_joints, mask_stride):
    """K: frames a session with ``repair_joints`` re-stages per slot and tick -- the multiples of s_in among G + 1 consecutive frames and
    the edge frame."""
    return int(repair_joints) // int(mask_stride) + 2


class LiveRepairHost(object):
    """The incremental state machine of uu3d_stream_repair_stage for ONE slot, in numpy, written to be read: ``predict.repair_joints_host``
    on the growing track, one frame per ``step``, from a bounded state --
        raw, observed   the raw coordinates and observed flags of the newest G + 1 frames (frame f at place f % (G + 1));
        last, last_xy   per joint the last observation that has LEFT that window, as index (-1: the joint was not seen before the window)
                        and coordinates;
        held            per joint G bits: bit k = frame last + 1 + k has left the window as a valid frame in which the joint was held
                        from ``last`` -- the frames a gap longer than G turns missing when it closes.
    ``step(frame (J, 2) float32, flags (J,) bool)`` -> (staged, far): ``staged`` lists (frame index, repaired raw (J, 2) float32,
    frame_valid, state (J,) uint8) for the frames this tick re-stages -- with t the frame pushed, the multiples of ``s_in`` in
    [max(0, t - G), t], oldest first, then the edge frame (t // seq_stride * seq_stride) where it lies in that range and is no multiple
    of ``s_in``; with s_in = 1 every frame of the range --, ``far`` the older frames that this tick turns from valid to missing, ascending.
    The repaired frame is ``repair_joints_host``'s (zeros for a joint it cannot fill); the device stages zeros for a frame that is not valid."""

    def __init__(self, J, G, s_in=1, seq_stride=1):
        self.J, self.G, self.W, self.s_in, self.seq_stride = int(J), int(G), int(G) + 1, int(s_in), int(seq_stride)
        if not 1 <= self.G <= MAX_LIVE_REPAIR:
            raise ValueError(f"G must be in [1, {MAX_LIVE_REPAIR}]")
        self.frames = 0
        self.raw = np.zeros((self.W, self.J, 2), np.float32)
        self.observed = np.zeros((self.W, self.J), bool)
        self.last = np.full(self.J, -1, np.int64)
        self.last_xy = np.zeros((self.J, 2), np.float32)
        self.held = [0] * self.J

    def _joint(self, f, j, lo, newest):
        """Joint j of frame f under the rule, seen from the frames lo .. newest of the window and ``last`` -> (xy, state)."""
        G, W, src = self.G, self.W, self.raw
        if self.observed[f % W, j]:
            return src[f % W, j], 1
        before = [g for g in range(lo, f) if self.observed[g % W, j]]
        after = [g for g in range(f + 1, newest + 1) if self.observed[g % W, j]]
        l, a = (before[-1], src[before[-1] % W, j]) if before else (int(self.last[j]), self.last_xy[j])
        r = after[0] if after else None
        if l >= 0 and r is not None:
            if r - l - 1 <= G:
                w = np.float64(f - l) / np.float64(r - l)
                return (a.astype(np.float64) * (1.0 - w) + src[r % W, j].astype(np.float64) * w).astype(np.float32), 2
        elif r is not None:
            if r - f <= G:
                return src[r % W, j], 2
        elif l >= 0:
            if f - l <= G:
                return a, 2
        return np.zeros(2, np.float32), 0

    def _frame(self, f, lo, newest):
        """Frame f under the rule -> (repaired (J, 2) float32, frame_valid, state (J,) uint8)."""
        out, state = np.zeros((self.J, 2), np.float32), np.zeros(self.J, np.uint8)
        for j in range(self.J):
            out[j], state[j] = self._joint(f, j, lo, newest)
        valid = bool((state == 1).any() and (state != 0).all())
        return out, valid, state

    def step(self, frame, flags):
        G, W, J, t = self.G, self.W, self.J, self.frames
        frame = np.asarray(frame, np.float32).reshape(J, 2)
        seen_now = (np.asarray(flags).reshape(J) != 0) & np.isfinite(frame).all(axis=1)
        # 1. frame e leaves the window: what it is under the frames up to t - 1 stays, but for the far list
        e = t - G - 1
        if e >= 0:
            _, valid_e, _ = self._frame(e, e, t - 1)
            for j in range(J):
                if self.observed[e % W, j]:
                    self.last[j], self.last_xy[j], self.held[j] = e, self.raw[e % W, j], 0
                elif valid_e and self.last[j] >= 0 and e - self.last[j] <= G:
                    self.held[j] |= 1 << (e - int(self.last[j]) - 1)
        # 2. file the pushed frame (the place frame e had)
        self.raw[t % W], self.observed[t % W] = frame, seen_now
        # 3. a joint seen again after more than G frames: the frames it was held in turn missing
        lo = max(0, t - G)
        far = set()
        for j in range(J):
            if seen_now[j] and self.last[j] >= 0 and t - self.last[j] - 1 > G and not self.observed[[g % W for g in range(lo, t)], j].any():
                far |= {int(self.last[j]) + 1 + k for k in range(G) if self.held[j] >> k & 1}
                self.held[j] = 0
        for f in far:                                                 # no longer valid frames, for any joint's bits
            for j in range(J):
                if self.last[j] >= 0 and 0 <= f - self.last[j] - 1 < G:
                    self.held[j] &= ~(1 << (f - int(self.last[j]) - 1))
        # 4. the frames to re-stage
        cand = [f for f in range(lo, t + 1) if f % self.s_in == 0]
        edge = t // self.seq_stride * self.seq_stride
        if edge >= lo and edge % self.s_in != 0:
            cand.append(edge)
        self.frames = t + 1
        return [(f,) + self._frame(f, lo, t) for f in cand], sorted(far)

    def newest_state(self):
        """(J,) uint8: the state of the newest frame (``StreamSession.joint_state``)."""
        t = self.frames - 1
        return self._frame(t, max(0, t - self.G), t)[2]
