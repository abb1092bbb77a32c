"""The root stage of the track pipeline: every track placed in the camera's 3D space (include/uu3d.h, ABSOLUTE ROOT POSITION).  Wraps
uu3d_solve_roots (``solve_roots``; the rule in numpy: ``solve_roots_host``) and uu3d_root_trajectory_scratch_bytes / uu3d_root_trajectory
(``root_trajectory``; ``root_trajectory_host``); ``LiveRootHost`` is the rule of a session's uu3d_stream_root / uu3d_stream_root_drain in
numpy.

Absolute root position: every pose ``predict_tracks`` returns is root-relative.  ``predict_tracks(..., camera=(fx, fy, cx, cy))`` also returns, per frame, where
the skeleton stands in the camera's space: at every given frame the translation that projects the returned pose onto the frame's own 2D
keypoints (uu3d_solve_roots: linear least squares over the observed joints; ``solve_roots`` is the launch alone; the rule in numpy:
``solve_roots_host``), joined to a piecewise-linear trajectory that is read at the returned frames (uu3d_root_trajectory;
``root_trajectory_host``).  ``predict_detections(..., camera=...)`` places every person of a video in the same space.

Live absolute root -- ``StreamSession(..., camera=(fx, fy, cx, cy), min_root_joints=6)``: every push returns, beside the poses, where each
of them stands in the camera's 3D space -- ``push`` -> (poses, fresh, roots (slots, 3) float32, root_state (slots,) uint8), and
``poses[i] + roots[i]`` is slot i's skeleton in the camera's space (``predict.predict_tracks(camera=...)`` for a finished video).  The
intrinsics are in the units of the frames AS PUSHED (pixels with ``resolutions``), one tuple or one per slot.  Per slot the session keeps a
ring of its last lookahead + 1 raw frames in the model's joint layout (behind the ``keypoints`` map, before normalisation; frame t at place
t % (lookahead + 1)) with one USED byte per joint -- the joint's flag (none: every joint; ``missed_detections``: the frame's flag for all of
its joints; ``repair_joints``: the push's per-joint flag, mapped with ``keypoints``) and both raw coordinates finite -- and the last solved
root.  A joint that ``repair_joints`` fills is never used (an interpolation is not a measurement) and the ring holds the pushed coordinates,
never the repaired ones, so no push revises it.  Whenever a slot's pose is fresh, the frame it belongs to -- c = t - lookahead, with ``fps``
source frame q = j - lookahead -- is solved against that pose by ``predict.solve_roots_host``'s rule, unchanged (uu3d_stream_root: lane j of
one wave per slot files joint j, lane 0 solves).  Solved: the root, state 1, and the slot holds it.  Not solved: the held root, state 2; no
held root yet: zeros, state 0.  A push that is not fresh returns the previous root and state, like the pose; ``reset`` clears ring, held
root and state (also on the device, for a slot born at a ``push_detections`` tick).  The rule is CAUSAL: it holds the last solved root and
cannot interpolate towards a later solved frame as ``predict_tracks(camera=...)`` does, because the poses of later frames do not exist
yet.  ``LiveRootHost`` is the rule in numpy.  The launch is the LAST step of the one captured tick (behind uu3d_stream_emit); with ``fps``
it follows uu3d_stream_timed_emit, not captured.  ``captures`` stays 1 and ``push`` never waits.  With ``detections`` one tuple only: the
people of a video share one space.  Not together with ``out_fps`` (ValueError: those poses are not at source-frame times; a later
change).  No accuracy is claimed: the model's scale error goes 1:1 into the depth.  ``camera=None`` is the session above, bit for bit: no
further launch or buffer."""
import ctypes as C
from fractions import Fraction

import numpy as np

from . import _capi
from ._capi import ptr as _ptr
from .rates import frame_rates, given_positions, output_positions, root_plan
from .tracks import _host_array, _upload

MAX_ROOT_JOINTS = 64                                                  # kRootMaxJoints
DEFAULT_MIN_ROOT_JOINTS = 6


def check_cameras(camera, count, per="track"):
    """``camera``: one (fx, fy, cx, cy) or one per track (per video, for ``predict_detections``) -> (count, 4) float64, contiguous.
    Anything else, a non-finite entry, fx <= 0 or fy <= 0 is a ValueError."""
    try:
        c = np.asarray(camera, np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"camera must be one (fx, fy, cx, cy) or one per {per}, got {camera!r}") from None
    if c.shape == (4,):
        c = np.tile(c, (int(count), 1))
    if c.shape != (int(count), 4):
        raise ValueError(f"camera must be one (fx, fy, cx, cy) or one per {per} ({int(count)}), got shape {c.shape}")
    if not np.isfinite(c).all() or not (c[:, :2] > 0).all():
        raise ValueError("camera must be finite (fx, fy, cx, cy) with fx > 0 and fy > 0")
    return np.ascontiguousarray(c)


def check_min_root_joints(min_root_joints):
    if isinstance(min_root_joints, bool) or not isinstance(min_root_joints, (int, np.integer)) or int(min_root_joints) < 2:
        raise ValueError(f"min_root_joints must be an int >= 2: the fewest used joints a frame's root is solved from, got {min_root_joints!r}")
    return int(min_root_joints)


def _root_lens(lens, frames):
    """Frames per track of a root call (None: one track) -> int64 array that adds up to ``frames``."""
    lens = np.array([int(frames)], np.int64) if lens is None else np.asarray(lens, np.int64).reshape(-1)
    if (lens < 0).any() or int(lens.sum()) != int(frames):
        raise ValueError(f"lens must add up to the {int(frames)} frames given")
    return lens


def solve_roots_host(poses, kp2d, camera, flags=None, min_root_joints=DEFAULT_MIN_ROOT_JOINTS, lens=None):
    """The per-frame rule of ABSOLUTE ROOT POSITION (include/uu3d.h) in numpy, written to be read: what uu3d_solve_roots computes, bit for
    bit.  ``poses`` (G, J, 3): the 3D pose of every frame, root-relative or not; ``kp2d`` (G, J, 2): the 2D keypoints it was uplifted from,
    raw, in the model's joint layout; ``camera``: (fx, fy, cx, cy) in the units of ``kp2d``, one or -- with ``lens``, frames per track --
    one per track; ``flags``: None or (G, J), non-zero = the joint was observed (non-finite coordinates are never used)
    -> (roots (G, 3) float64, solved (G,) bool); the root of a frame that is not solved is zeros.
    Everything in float64, every product and sum rounded; the sums run over the used joints in ascending order as a plain loop (np.sum
    adds pairwise, np.dot in BLAS's order)."""
    P = np.asarray(_host_array(poses), np.float32)
    uv = np.asarray(_host_array(kp2d), np.float32)
    if P.ndim != 3 or P.shape[2] != 3 or uv.shape != P.shape[:2] + (2,):
        raise ValueError(f"poses must be (G, J, 3) and kp2d (G, J, 2), got {P.shape} and {uv.shape}")
    G, J = P.shape[:2]
    m = check_min_root_joints(min_root_joints)
    lens = _root_lens(lens, G)
    cam = np.repeat(check_cameras(camera, len(lens)), lens, axis=0)      # (G, 4): the camera of each frame's track
    fx, fy, cx, cy = cam[:, 0], cam[:, 1], cam[:, 2], cam[:, 3]
    used = np.isfinite(uv).all(axis=2)
    if flags is not None:
        f = np.asarray(_host_array(flags)) != 0
        if f.shape != (G, J):
            raise ValueError(f"flags must be ({G}, {J}), got {f.shape}")
        used &= f
    P64, uv64 = P.astype(np.float64), uv.astype(np.float64)
    n = np.zeros(G, np.int64)
    Sa, Sb, Sq, Sp, Sk, Sr = (np.zeros(G, np.float64) for _ in range(6))
    with np.errstate(all="ignore"):
        for j in range(J):
            X, Y, Z = P64[:, j, 0], P64[:, j, 1], P64[:, j, 2]
            a = (uv64[:, j, 0] - cx) / fx
            b = (uv64[:, j, 1] - cy) / fy
            p = a * Z - X
            q = b * Z - Y
            u = used[:, j]
            n += u
            Sa = np.where(u, Sa + a, Sa)
            Sb = np.where(u, Sb + b, Sb)
            Sq = np.where(u, Sq + (a * a + b * b), Sq)
            Sp = np.where(u, Sp + p, Sp)
            Sk = np.where(u, Sk + q, Sk)
            Sr = np.where(u, Sr + (a * p + b * q), Sr)
        nd = n.astype(np.float64)
        den = Sq - (Sa * Sa + Sb * Sb) / nd
        num = (Sa * Sp + Sb * Sk) / nd - Sr
        Tz = num / den
        Tx = (Sp + Sa * Tz) / nd
        Ty = (Sk + Sb * Tz) / nd
        solved = (n >= m) & (den > 0) & np.isfinite(Tx) & np.isfinite(Ty) & np.isfinite(Tz) & (Tz > 0)
        for j in range(J):                                            # every used joint in front of the camera
            solved &= ~used[:, j] | (P64[:, j, 2] + Tz > 0)
    roots = np.zeros((G, 3), np.float64)
    roots[solved] = np.stack([Tx, Ty, Tz], axis=1)[solved]
    return roots, solved


def root_trajectory_host(roots, solved, lens=None, positions=None):
    """The trajectory rule of ABSOLUTE ROOT POSITION in numpy, written to be read: what uu3d_root_trajectory computes, bit for bit.
    ``roots`` (G, 3) float64 and ``solved`` (G,) of ``solve_roots_host``, the given frames of all tracks back to back, ``lens`` of them
    per track (None: one track); ``positions``: (track, num, den) of ``given_positions`` -- returned frame i sits at given-frame position
    num / den of its track -- or None: every given frame itself -> (roots (R, 3) float32, root_state (R,) uint8: 1 solved here, 2
    interpolated or held, 0 the track has no solved frame).  Nothing crosses a track boundary."""
    roots = np.asarray(roots, np.float64).reshape(-1, 3)
    solved = np.asarray(solved).reshape(-1) != 0
    lens = _root_lens(lens, len(roots))
    start = np.concatenate([[0], np.cumsum(lens)])
    if positions is None:
        positions = given_positions(lens)
    base, _, _ = root_plan(lens, positions)                             # (the range checks of the device call)
    out = np.zeros((len(base), 3), np.float32)
    state = np.zeros(len(base), np.uint8)
    for i, (t, num, den) in enumerate(zip(*(np.asarray(a).tolist() for a in positions))):
        seen = np.flatnonzero(solved[start[t]:start[t + 1]])          # the track's solved frames, by their index in the track
        b = num // den
        before, after = seen[seen <= b], seen[seen > b]
        L = int(before[-1]) if len(before) else None
        R = int(after[0]) if len(after) else None
        if L == b and num == b * den:
            out[i], state[i] = roots[start[t] + L].astype(np.float32), 1
        elif L is not None and R is not None:
            w = np.float64(num - L * den) / np.float64((R - L) * den)
            out[i], state[i] = (roots[start[t] + L] * (1.0 - w) + roots[start[t] + R] * w).astype(np.float32), 2
        elif L is not None or R is not None:
            out[i], state[i] = roots[start[t] + (L if L is not None else R)].astype(np.float32), 2
    return out, state


def solve_roots(poses, kp2d, camera, flags=None, min_root_joints=DEFAULT_MIN_ROOT_JOINTS, lens=None):
    """uu3d_solve_roots on the current stream: ``solve_roots_host`` on device tensors, one launch, nothing copies to the host or waits.
    ``poses`` (G, J, 3) float32 and ``kp2d`` (G, J, 2) float32 on the device, contiguous (only read); ``camera``: (fx, fy, cx, cy), one or
    one per track with ``lens`` (frames per track); ``flags`` (G, J) uint8 / bool on the device or None
    -> (roots (G, 3) float64, solved (G,) bool), fresh device buffers.  ``poses + roots[:, None]`` stands in the camera's space.
    The live form is ``StreamSession(camera=...)``: every push returns the roots beside the poses, at any ``lookahead`` (the session keeps
    the raw frames an emitted pose belongs to); at ``lookahead=0`` a solved root of it is this call on the push's poses and frame."""
    import torch
    lib = _capi.load_library()
    dev = poses.device
    if poses.dim() != 3 or poses.shape[2] != 3 or poses.dtype != torch.float32 or not poses.is_contiguous() or not poses.is_cuda:
        raise ValueError(f"poses must be a contiguous (G, J, 3) float32 device tensor, got {tuple(poses.shape)}")
    G, J = int(poses.shape[0]), int(poses.shape[1])
    if tuple(kp2d.shape) != (G, J, 2) or kp2d.dtype != torch.float32 or not kp2d.is_contiguous() or kp2d.device != dev:
        raise ValueError(f"kp2d must be a contiguous ({G}, {J}, 2) float32 tensor on the poses' device, got {tuple(kp2d.shape)}")
    if flags is not None:
        if tuple(flags.shape) != (G, J) or flags.dtype not in (torch.uint8, torch.bool) or not flags.is_contiguous() or flags.device != dev:
            raise ValueError(f"flags must be a contiguous ({G}, {J}) uint8 or bool tensor on the poses' device")
        flags = flags.view(torch.uint8)
    m = check_min_root_joints(min_root_joints)
    lens = _root_lens(lens, G)
    cams = _upload(check_cameras(camera, len(lens)), np.float64, dev)
    row_track = None if len(lens) == 1 else _upload(np.repeat(np.arange(len(lens), dtype=np.int32), lens), np.int32, dev)
    roots = torch.empty((G, 3), dtype=torch.float64, device=dev)
    solved = torch.empty((G,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(lib, lib.uu3d_solve_roots(_ptr(poses), _ptr(kp2d), _ptr(flags), G, J, _ptr(row_track), len(lens), _ptr(cams), m, _ptr(roots),
                                              _ptr(solved), C.c_void_p(stream)), None)
    return roots, solved.view(torch.bool)


def root_trajectory(roots, solved, lens=None, positions=None):
    """uu3d_root_trajectory on the current stream: ``root_trajectory_host`` on the device tensors of ``solve_roots``; the plan
    (``root_plan``) is made on the host in exact integers and goes up pinned and asynchronously -> (roots (R, 3) float32, root_state (R,)
    uint8), fresh device buffers."""
    import torch
    lib = _capi.load_library()
    dev = roots.device
    G = int(roots.shape[0])
    if tuple(roots.shape) != (G, 3) or roots.dtype != torch.float64 or not roots.is_contiguous() or not roots.is_cuda or G < 1:
        raise ValueError(f"roots must be a contiguous (G, 3) float64 device tensor, got {tuple(roots.shape)}")
    if tuple(solved.shape) != (G,) or solved.dtype not in (torch.uint8, torch.bool) or not solved.is_contiguous() or solved.device != dev:
        raise ValueError(f"solved must be a contiguous ({G},) uint8 or bool tensor on the roots' device")
    lens = _root_lens(lens, G)
    base, wnum, wden = root_plan(lens, positions)
    R = len(base)
    if R < 1:
        raise ValueError("no returned frames")
    track_start = _upload(np.concatenate([[0], np.cumsum(lens)]), np.int64, dev)
    d_plan = _upload(np.stack([base, wnum, wden]), np.int64, dev)
    out = torch.empty((R, 3), dtype=torch.float32, device=dev)
    state = torch.empty((R,), dtype=torch.uint8, device=dev)
    nbytes = int(lib.uu3d_root_trajectory_scratch_bytes(G))
    if nbytes == 0:
        raise ValueError(f"{G} given frames are out of uu3d_root_trajectory's range")
    scratch = torch.empty((nbytes // 4,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(lib, lib.uu3d_root_trajectory(_ptr(roots), _ptr(solved.view(torch.uint8)), G, _ptr(track_start), len(lens), _ptr(d_plan[0]),
                                                  _ptr(d_plan[1]), _ptr(d_plan[2]), R, _ptr(out), _ptr(state), _ptr(scratch), nbytes,
                                                  C.c_void_p(stream)), None)
    return out, state


def poses_at_given_frames(poses, lens, given, key_stride=0, rates=None, out_fps=None, model_fps=50, reread=None):
    """What ``predict_tracks(camera=...)`` solves the roots against: the poses at the GIVEN frames' times, and where the returned frames lie
    among the given ones.  ``poses`` (sum(lens), J, 3): the returned poses, ``lens`` of them per track; ``given``: frames given per track
    -> (poses (sum(given), J, 3), the ``positions`` of ``root_trajectory`` -- None: every returned frame is a given frame).
      the plain call and ``fps`` alone    the returned poses themselves;
      ``key_stride`` = s_in (``keyframes_only``)    given keyframe g is returned frame g s_in: one index_select, positions i / s_in;
      ``out_fps`` (with the tracks' ``rates``)    ``reread(at)`` reads the same motion once more at the model positions ``at`` of the given
          frames -- a second uu3d_assemble_tracks over the same raw predictions and, with ``bones``, uu3d_fix_bones with the same lengths
          table; no further forward --, positions i fps / out_fps."""
    if key_stride:
        first = np.concatenate([[0], np.cumsum(lens)[:-1]])
        picks = np.concatenate([f + np.arange(n, dtype=np.int64) * int(key_stride) for f, n in zip(first, given)])
        return poses.index_select(0, _upload(picks, np.int64, poses.device)), given_positions(lens, [Fraction(1, int(key_stride))] * len(given))
    if out_fps is not None:
        _, at = output_positions(given, rates, rates, model_fps)
        return reread(at), given_positions(lens, [f / o for f, o in zip(rates, frame_rates(out_fps, len(given)))])
    return poses, None


class LiveRootHost(object):
    """The rule of uu3d_stream_root for ONE slot, in numpy, written to be read: the live form of ``predict.solve_roots_host``.  State --
        raw, used   the raw coordinates and USED flags of the newest lookahead + 1 frames (frame f at place f % (lookahead + 1));
        held        the last solved root, float64 (None: no frame was solved yet);
        root, state what the slot returned last.
    ``step(frame (J, 2) float32, used_flags, pose)``: one push of the slot while it is active.  ``frame``: the raw frame as pushed, in
    the model's joint layout; ``used_flags``: None (every joint), one flag for the whole frame, or (J,) flags -- a joint is USED iff its flag
    is set and both coordinates are finite; ``pose``: the (J, 3) pose the push returned when it is fresh, else None.
    -> (root (3,) float32, state): a fresh pose is solved against frame c = t - lookahead (t: the frame just filed) -- solved: the root
    rounded to float32, state 1, and the root is held; not solved (or c < 0): the held root, state 2, or zeros, state 0, when none
    exists.  ``pose=None`` returns what the last step returned.  A push at which the slot is inactive is no step.  The rule is causal: it
    holds the last solved root and never interpolates towards a later one (``predict.root_trajectory_host`` does; it sees the whole track)."""

    def __init__(self, J, lookahead, camera, min_root_joints=DEFAULT_MIN_ROOT_JOINTS):
        self.J, self.W = int(J), int(lookahead) + 1
        if not 1 <= self.J <= MAX_ROOT_JOINTS or self.W < 1:
            raise ValueError(f"J must be in [1, {MAX_ROOT_JOINTS}] and lookahead >= 0")
        self.camera = check_cameras(camera, 1, per="slot")[0]
        self.min_root_joints = check_min_root_joints(min_root_joints)
        self.reset()

    def reset(self):
        self.frames = self.drained = 0                                # (drained: drain ticks taken since the track ended)
        self.raw = np.zeros((self.W, self.J, 2), np.float32)
        self.used = np.zeros((self.W, self.J), bool)
        self.held = None
        self.root, self.state = np.zeros(3, np.float32), 0

    def step(self, frame, used_flags=None, pose=None):
        J, W, t = self.J, self.W, self.frames
        frame = np.asarray(frame, np.float32).reshape(J, 2)
        flags = np.ones(J, bool) if used_flags is None else np.broadcast_to(np.asarray(used_flags) != 0, (J,))
        # 1. file the pushed frame
        self.raw[t % W], self.used[t % W] = frame, flags & np.isfinite(frame).all(axis=1)
        self.frames = t + 1
        # 2. solve the frame the fresh pose belongs to
        return self._settle(t - (W - 1), pose)

    def drain(self, pose=None):
        """One drain tick of the slot (``StreamSession.finish``; uu3d_stream_root_drain): the track has ENDED, nothing is filed.  The k-th
        drain tick since the last step (k = 1 .. lookahead; a tick beyond that, or of a slot without frames, changes nothing) solves
        frame c = frames - 1 - lookahead + k -- one of the last lookahead + 1 frames filed, so it is in the ring -- against ``pose``, the
        (J, 3) pose of that tick when it is fresh, else None; held root and state by ``step``'s rule.  -> (root, state)."""
        if self.frames < 1 or self.drained >= self.W - 1:
            return self.root.copy(), self.state
        self.drained += 1
        return self._settle(self.frames - 1 - (self.W - 1) + self.drained, pose)

    def _settle(self, c, pose):
        """The root of a push or drain tick whose pose (None: not fresh) belongs to frame c -> (root, state)."""
        J, W = self.J, self.W
        if pose is None:                                              # not fresh: nothing is solved, nothing changes
            return self.root.copy(), self.state
        solved = False
        if c >= 0:
            roots, ok = solve_roots_host(np.asarray(pose, np.float32).reshape(1, J, 3), self.raw[c % W][None], self.camera,
                                         flags=self.used[c % W][None], min_root_joints=self.min_root_joints)
            solved = bool(ok[0])
        # 3. the root of this push: solved here, else the last solved one
        if solved:
            self.held, self.state = roots[0], 1
            self.root = roots[0].astype(np.float32)
        else:
            self.state = 2 if self.held is not None else 0
        return self.root.copy(), self.state


class LiveRoot(object):
    """uu3d_stream_root as an output-side stage of a ``StreamSession`` (the interface: ``smooth.LiveOneEuro``).  ``keypoints`` / ``flags``
    (or None): the session's buffers of the pushed frame and its validity flags, which the tick's solve files -- no part of a scene."""

    def __init__(self, slots, joints, lookahead, cameras, min_root_joints, keypoints, flags, device):
        import torch
        self._lib = _capi.load_library()
        size = int(self._lib.uu3d_stream_root_bytes(slots, joints, lookahead))
        if size == 0:
            raise ValueError(f"camera: slots = {slots}, joints = {joints}, lookahead = {lookahead} are out of uu3d_stream_root's range")
        self._shape, self.min_root_joints, self._keypoints, self._flags = (slots, joints, lookahead), min_root_joints, keypoints, flags
        self._cams = _upload(cameras, cameras.dtype, device)
        self._state = torch.zeros(size, dtype=torch.uint8, device=device)
        self.roots = torch.zeros((slots, 3), dtype=torch.float32, device=device)
        self.state = torch.zeros((slots,), dtype=torch.uint8, device=device)
        self.outputs = (("roots", "roots", self.roots), ("root_state", "root_state", self.state))

    def launch(self, active, frames, drain_state=None):
        read, solve = self.read, (_ptr(self._cams), self.min_root_joints, _ptr(self.roots), _ptr(self.state))
        if drain_state is not None:                                  # a drain tick files nothing and solves from the ring
            return (self._lib.uu3d_stream_root_drain, self._shape + (_ptr(self._state), _ptr(drain_state), _ptr(active), _ptr(read.fresh),
                                                                     _ptr(read.poses)) + solve)
        per_joint = int(self._flags is not None and self._flags.dim() == 2)
        return (self._lib.uu3d_stream_root, self._shape + (_ptr(self._state), _ptr(frames), _ptr(active), _ptr(read.fresh), _ptr(read.poses),
                                                           _ptr(self._keypoints), _ptr(self._flags), per_joint) + solve)

    def reset_launch(self):
        return (self._lib.uu3d_stream_root_reset, self._shape + (_ptr(self._state),))
