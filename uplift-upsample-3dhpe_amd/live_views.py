"""Live several views: ``StreamSession(model, config, slots=V * N, camera=[V Cameras with extrinsics], views=V)`` fuses the cameras of a
rig at every tick, on the device (include/uu3d.h, LIVE SEVERAL VIEWS) -- the live form of ``predict.predict_views``' fusion and root solve.

The slots are VIEW-MAJOR, the layout of ``predict_views``' flattened tracks: slot ``v * N + i`` is person i in camera v; ``camera`` is one
``Camera`` per VIEW and the session expands it to one row per slot.  Nothing changes on the input side: stage, features, commit, forward,
emit, uu3d_stream_root and uu3d_camera_to_world run on all V N slots as in a session with one ``Camera`` per slot.  One stage more,
``LiveViews`` (uu3d_stream_views), joins the launch table directly behind uu3d_camera_to_world; the two filters and the rotations follow it
and run on N person rows.  ``push`` -> (poses (N, J, 3), fresh (N,), roots (N, 3), root_state (N,), view_count (N,) uint8), on the device;
``view_count`` is the first of the buffers appended behind the four, in front of ``rotations``.  ``push`` still never waits, ``captures``
stays 1, the tick stays one linear captured graph.

THE RULE (``LiveViewsHost`` is it in numpy, the device equals it bit for bit).  A push is the clock: the frames all slots received at one
push are one instant, whatever the slots' counters say.
  taking part   view v takes part in person i's tick iff its slot is active and its pose is fresh at this tick.
  seeing        view v sees the person iff it takes part and at least ``min_root_joints`` joints are USED in its own frame
                c_v = frames[slot] - 1 - lookahead: the USED bytes of uu3d_stream_root's ring, which the stage reads and never writes.
  fresh         person i is fresh iff some view takes part.  Its pose is ``fuse_views_host``'s rule over the seeing views in ascending order,
                ``view_count`` their number; if no view sees, the mean over the views that take part, ``view_count`` 0.
  world root    ``solve_view_roots_host``'s rule over the seeing views -- the same statements, the 2^-40 rank guard, the in-front test --
                against the fused pose and each view's own ring frame.  Solved: the held root (float64, per person) takes it, state 1.  Not
                solved: state 2 when a held root exists, else 0 (``LiveRootHost``'s settling; causal, nothing is interpolated).
  not fresh     the pose row keeps its bits; the held root and the last state are returned, ``view_count`` 0.
  counter       the stage owns a per-person tick counter, which grows by one at every push at which any of the person's slots is active,
                and a per-person ``active``; the filters behind take them where they take a slot's counter and ``active``.
  reset         ``reset(slots)`` clears a person's held root, state and counter iff ALL V of its slots are chosen (None: everybody).
On a model whose prediction stride is above 1 a slot is fresh on every stride-th push of its own counter: views whose slots were reset at
different pushes are fresh at different ticks and never meet in one fusion.  Start (and reset) a person's V slots together.

Refused (ValueError, no device touched): ``views`` without ``camera``; another camera count than V; a camera without extrinsics; plain
tuples; V outside 1 .. 8; ``slots % V != 0``; ``detections``; ``out_fps``; ``bones`` (offline it runs on the fused pose, in front of the
solve: a later change); a list that mixes cameras with and without distortion (the session's front undistorts all slots or none).
``finish()`` on such a session: ValueError (a later change).  ``fps`` and ``interpolation="cubic"`` mean what they mean with ``camera=``: the
stage sits behind the timed emit and reads the ring under the same (source) counters.  Out of scope live: ``match``, ``align``,
``triangulate``, ``calibrate``, ``bones`` on the fused pose, ``finish``, per-frame detections across views.  No accuracy is claimed."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import ptr as _ptr
from .camera import Camera
from .roots import DEFAULT_MIN_ROOT_JOINTS, MAX_ROOT_JOINTS, check_min_root_joints
from .tracks import _upload
from .views import MAX_VIEWS, check_view_cameras, fuse_views_host, solve_view_roots_host, view_rows


def check_live_views(views, camera, slots, detections=None, out_fps=None, bones=None):
    """``StreamSession(views=V, camera=...)`` -> (V, the V ``Camera`` objects, the camera list expanded to one entry per slot, view-major).
    Every refusal of the module's docstring is a ValueError."""
    if isinstance(views, bool) or not isinstance(views, (int, np.integer)) or not 1 <= int(views) <= MAX_VIEWS:
        raise ValueError(f"views must be an int in [1, {MAX_VIEWS}], the cameras of the rig, got {views!r}")
    V, slots = int(views), int(slots)
    if camera is None:
        raise ValueError("views needs camera: one Camera with extrinsics per view (the views meet in the world frame)")
    if isinstance(camera, Camera):
        camera = [camera]
    cams = check_view_cameras(camera, V)
    if slots % V != 0:
        raise ValueError(f"slots must be a multiple of views: slot v * N + i is person i in camera v, got slots = {slots} and views = {V}")
    if detections is not None:
        raise ValueError("views together with detections is not supported: the association runs per camera and does not know which person "
                         "of one view is which of another (a later change)")
    if out_fps is not None:
        raise ValueError("views together with out_fps is not supported: camera together with out_fps is not (the returned poses are not at "
                         "source-frame times, so no pushed frame is theirs to be solved against)")
    if bones is not None:
        raise ValueError("views together with bones is not supported yet: offline the fix runs on the fused pose, in front of the root solve "
                         "(a later change)")
    return V, cams, [c for c in cams for _ in range(slots // V)]


class LiveViewsHost(object):
    """The rule of uu3d_stream_views (the module's docstring) for a whole rig, in numpy, written to be read.  It files the pushed frames
    itself, as ``LiveRootHost`` does per slot: raw coordinates and USED flags of the newest lookahead + 1 frames per slot.
    ``step(kp (V N, J, 2), used_flags, active (V N,) or None, fresh (V N,), view_poses (V N, J, 3))``: one push.  ``kp``: the frames as
    pushed, in the model's layout (undistorted); ``used_flags``: None, (V N,) or (V N, J); ``fresh`` / ``view_poses``: what the session
    without ``views`` returned at this push -- its fresh flags and its world poses
    -> (poses (N, J, 3) float32, fresh (N,) bool, roots (N, 3) float32, root_state (N,) uint8, view_count (N,) uint8); ``frames`` (N,) and
    ``active`` (N,) are the person counter and flag the stages behind take.  ``reset(slots=None)``: the chosen slots lose their ring and
    counter; a person ALL of whose slots are chosen loses held root, state and counter."""

    def __init__(self, views, persons, joints, lookahead, cameras, min_root_joints=DEFAULT_MIN_ROOT_JOINTS):
        self.V, self.N, self.J, self.W = int(views), int(persons), int(joints), int(lookahead) + 1
        if not 1 <= self.J <= MAX_ROOT_JOINTS or self.W < 1 or self.N < 1:
            raise ValueError(f"joints must be in [1, {MAX_ROOT_JOINTS}], lookahead >= 0 and persons >= 1")
        self.cameras = check_view_cameras(cameras, self.V)
        self.min_root_joints = check_min_root_joints(min_root_joints)
        T, N, J = self.V * self.N, self.N, self.J
        self.slot_frames = np.zeros(T, np.int64)
        self.raw, self.used = np.zeros((T, self.W, J, 2), np.float32), np.zeros((T, self.W, J), bool)
        self.held, self.state = np.zeros((N, 3), np.float64), np.zeros(N, np.uint8)
        self.frames, self.active = np.zeros(N, np.int64), np.zeros(N, bool)
        self.poses = np.zeros((N, J, 3), np.float32)

    def reset(self, slots=None):
        chosen = np.zeros(self.V * self.N, bool)
        chosen[slice(None) if slots is None else np.asarray(slots, np.int64).reshape(-1)] = True
        self.slot_frames[chosen] = 0
        self.raw[chosen], self.used[chosen] = 0, False
        everyone = chosen.reshape(self.V, self.N).all(axis=0)
        self.held[everyone], self.state[everyone], self.frames[everyone] = 0, 0, 0

    def step(self, kp, used_flags, active, fresh, view_poses):
        V, N, J, W = self.V, self.N, self.J, self.W
        T = V * N
        kp = np.asarray(kp, np.float32).reshape(T, J, 2)
        flags = np.ones((T, J), bool) if used_flags is None else np.broadcast_to((np.asarray(used_flags) != 0).reshape(T, -1), (T, J))
        active = np.ones(T, bool) if active is None else np.asarray(active).reshape(T) != 0
        fresh = np.asarray(fresh).reshape(T) != 0
        P = np.asarray(view_poses, np.float32).reshape(T, J, 3)
        # 1. file the pushed frames (uu3d_stream_root's filing, an earlier launch of the tick)
        for s in np.flatnonzero(active):
            t = int(self.slot_frames[s])
            self.raw[s, t % W], self.used[s, t % W] = kp[s], flags[s] & np.isfinite(kp[s]).all(axis=1)
            self.slot_frames[s] = t + 1
        out_fresh, count = np.zeros(N, bool), np.zeros(N, np.uint8)
        for i in range(N):
            slots = np.arange(V) * N + i
            part = active[slots] & fresh[slots] & (self.slot_frames[slots] >= 1)
            self.active[i] = active[slots].any()
            self.frames[i] += int(self.active[i])
            if not part.any():                                        # not fresh: nothing is fused, nothing is solved, nothing changes
                continue
            # 2. the views that take part, ascending; a view whose frame is not in the ring (c < 0) cannot see
            who = np.flatnonzero(part)
            c = self.slot_frames[slots[who]] - 1 - (W - 1)
            frame = np.full((len(who), 1, J, 2), np.nan, np.float32)
            used = np.zeros((len(who), 1, J), bool)
            for k, (s, ck) in enumerate(zip(slots[who], c)):
                if ck >= 0:
                    frame[k, 0], used[k, 0] = self.raw[s, ck % W], self.used[s, ck % W]
            # 3. the fusion and the root of SEVERAL VIEWS on this one instant
            fused, seen, _ = fuse_views_host(P[slots[who]][:, None], frame, used, self.min_root_joints)
            root, solved = solve_view_roots_host(fused, frame, [self.cameras[v] for v in who], used, self.min_root_joints)
            self.poses[i], count[i], out_fresh[i] = fused[0], seen[0], True
            # 4. settling: the root solved here, else the last solved one
            if solved[0]:
                self.held[i], self.state[i] = root[0], 1
            else:
                self.state[i] = 2 if self.state[i] != 0 else 0
        return self.poses.copy(), out_fresh, self.held.astype(np.float32), self.state.copy(), count


class LiveViews(object):
    """uu3d_stream_views as an output-side stage of a ``StreamSession`` (the interface: ``smooth.LiveOneEuro``), directly behind
    ``LiveWorld``.  ``slots`` = V N, view-major; ``root``: the ``LiveRoot`` of the same slots whose ring the stage reads (its lookahead
    and ``min_root_joints`` are the stage's); ``cameras``: the V ``Camera`` objects.  It reads the scene in front of it -- the slots'
    world poses and fresh flags -- and leaves the persons' scene: ``poses`` (N, J, 3), ``fresh`` (N,), ``roots`` (N, 3), ``state`` (N,)
    and ``view_count`` (N,); ``frames`` (N,) int32 and ``active`` (N,) uint8 are the person counter and flag the stages behind take.
    The chain ``LiveRoot`` -> ``LiveWorld`` -> ``LiveViews`` needs no model."""

    def __init__(self, slots, joints, views, root, cameras, device):
        import torch
        self._lib = _capi.load_library()
        self.views, self.persons, self.joints = int(views), int(slots) // int(views), int(joints)
        if self.persons * self.views != int(slots) or tuple(root._shape[:2]) != (int(slots), self.joints):
            raise ValueError(f"views: {slots} slots of {joints} joints must be {views} views of whole persons on the root stage's own slots")
        size = int(self._lib.uu3d_stream_views_bytes(self.views, self.persons))
        if size == 0:
            raise ValueError(f"views = {self.views}, persons = {self.persons} are out of uu3d_stream_views' range")
        self._root, self.lookahead, self.min_root_joints = root, int(root._shape[2]), root.min_root_joints
        self._cams = _upload(view_rows(check_view_cameras(cameras, self.views)), np.float64, device)
        N, J = self.persons, self.joints
        self._state = torch.zeros(size, dtype=torch.uint8, device=device)
        self.poses = torch.zeros((N, J, 3), dtype=torch.float32, device=device)
        self.roots = torch.zeros((N, 3), dtype=torch.float32, device=device)
        self.fresh, self.state, self.view_count, self.active = (torch.zeros((N,), dtype=torch.uint8, device=device) for _ in range(4))
        self.frames = torch.zeros((N,), dtype=torch.int32, device=device)
        self.outputs = (("poses", "fused_poses", self.poses), ("fresh", "fused_fresh", self.fresh), ("roots", "fused_roots", self.roots),
                        ("root_state", "fused_root_state", self.state), ("extras", "view_count", self.view_count))

    def launch(self, active, frames, drain_state=None):
        read = self.read
        return (self._lib.uu3d_stream_views, (self.views, self.persons, self.joints, self.lookahead, _ptr(self._state), _ptr(self._root._state),
                                              _ptr(frames), _ptr(active), _ptr(read.fresh), _ptr(read.poses), _ptr(self._cams), self.min_root_joints,
                                              _ptr(self.poses), _ptr(self.fresh), _ptr(self.roots), _ptr(self.state), _ptr(self.view_count),
                                              _ptr(self.frames), _ptr(self.active)))

    def reset_launch(self):
        return (self._lib.uu3d_stream_views_reset, (self.views, self.persons, _ptr(self._state)))


def person_mask(slots, views, count):
    """The slots ``reset`` was given (indices; None = all) of a view-major session of ``count`` slots -> None, or the (N,) uint8 host mask of
    the persons ALL of whose V slots are chosen: what the stages behind ``LiveViews`` reset."""
    if slots is None:
        return None
    chosen = np.zeros(int(count), bool)
    chosen[np.asarray(slots, np.int64).reshape(-1)] = True
    return np.ascontiguousarray(chosen.reshape(int(views), -1).all(axis=0).astype(np.uint8))


def replay_views(model, config, views, cameras, resolutions=None, mask_stride=None, flip=None, lookahead=0, graph=True, fps=None, model_fps=50,
                 interpolation="linear", **options):
    """Push finished view tracks tick by tick through a ``StreamSession(views=V)``, all slots active and in phase.  ``views``: a list of V
    lists of N tracks (T, J, 2), ``views[v][i]`` person i in camera v, every track of one length T (``predict_views``' layout);
    ``cameras``: V ``Camera`` objects with extrinsics; ``resolutions``: None, one (w, h) or one per view; ``options``: ``min_root_joints``,
    ``smooth``, ``rotations``, ``keypoints`` as ``StreamSession`` takes them
    -> per person (poses (T, J, 3) float32, fresh (T,) bool, roots (T, 3) float32, root_state (T,) uint8, view_count (T,) uint8) and, with
    ``rotations``, the quaternions (T, J, 4) behind them: lists of N host arrays.  One copy to the host, at the end."""
    import torch
    from .stream import StreamSession
    if not isinstance(views, (list, tuple)) or not 1 <= len(views) <= MAX_VIEWS or not all(isinstance(v, (list, tuple)) and len(v) == len(views[0]) >= 1 for v in views):
        raise ValueError(f"views must be a list of 1 to {MAX_VIEWS} lists of tracks, one list per camera, the same persons in each")
    V, N = len(views), len(views[0])
    flat = [np.asarray(t, np.float32) for tracks in views for t in tracks]
    ticks = int(flat[0].shape[0])
    if ticks < 1 or any(t.ndim != 3 or t.shape != flat[0].shape for t in flat):
        raise ValueError("replay_views takes tracks of one shape (T >= 1, J, 2): all slots are pushed in phase")
    if resolutions is not None and np.ndim(resolutions) == 2:
        resolutions = [r for r in resolutions for _ in range(N)]
    s = StreamSession(model, config, V * N, resolutions=resolutions, mask_stride=mask_stride, flip=flip, lookahead=lookahead, graph=graph, fps=fps,
                      model_fps=model_fps, interpolation=interpolation, camera=list(cameras), views=V, **options)
    kept = None
    try:
        for k in range(ticks):
            out = s.push(np.stack([t[k] for t in flat]))
            if kept is None:
                kept = [torch.zeros((ticks,) + tuple(o.shape), dtype=o.dtype, device=o.device) for o in out]
            for dst, src in zip(kept, out):
                dst[k].copy_(src)
        s.check_range()
    finally:
        s.close()
    return tuple([a[:, i] for i in range(N)] for a in (t.cpu().numpy() for t in kept))
