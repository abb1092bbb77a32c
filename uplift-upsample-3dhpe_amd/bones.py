"""The bone stage of the track pipeline: rigid skeletons, every bone at one length over a track (include/uu3d.h, CONSTANT BONE LENGTHS).
Wraps uu3d_bone_lengths (``bone_lengths``; the rule in numpy: ``bone_lengths_host``) and uu3d_fix_bones (``fix_bones``;
``fix_bones_host``); ``LiveBonesHost`` is the rule of a session's uu3d_stream_bones in numpy.

Constant bone lengths: the network predicts every frame's skeleton on its own, so nothing holds a person's bone lengths constant over a
track.  ``predict_tracks(..., bones="track")`` rebuilds every pose from the root outwards with each bone at the track's mean length;
``bones=lengths`` does it with lengths that are known -- calibrated once with ``bone_lengths`` on a recording -- which also takes the
model's scale error out of the depth ``camera`` solves (``Skeleton`` / ``SKELETONS``: the tree; uu3d_bone_lengths, uu3d_fix_bones;
``bone_lengths`` / ``fix_bones`` are the launches alone; the rule in numpy: ``bone_lengths_host`` / ``fix_bones_host``).

Live constant bone lengths -- ``StreamSession(..., bones=B)``: the network predicts every tick's skeleton on its own, so a person's bone
lengths breathe from tick to tick, and under ``camera`` the depth with them.  ``bones`` -- "track", a (J,) array of lengths by child joint,
one such array per slot, or a ``predict.Bones(lengths, skeleton)`` for another tree than ``predict.SKELETONS["h36m17"]`` -- puts ONE more
launch into the session's launch table, directly behind the emit (with ``fps`` behind uu3d_stream_timed_emit) and in front of the root
solve and the One-Euro launches: uu3d_stream_bones, one wave per slot, rebuilds the emitted pose from the root outwards with every bone at
the slot's length, its direction kept (the rule: ``predict.fix_bones_host``; include/uu3d.h, CONSTANT BONE LENGTHS).  It writes a buffer
of its own, which ``push`` returns and the root solve and the pose filter read; ``raw_poses`` stays the model's output and
``bone_lengths`` is the slots' (slots, J) float64 table on the device.  With "track" a slot's length is the mean over the FRESH poses it
has emitted so far: the mean is CAUSAL and therefore differs from ``predict_tracks(bones="track")``, which averages the whole track; early
in a track it still moves, and a subject whose lengths are known should pass them.  The output is a pure function of the raw pose and the
slot's lengths: a slot that is not fresh returns its previous rebuilt pose, bit for bit.  ``reset`` and a birth at a ``push_detections``
tick clear the sums and counts with everything else; ``finish`` runs the same step in every drain tick, the chosen slots as ``active``.
``LiveBonesHost`` is the rule in numpy, and the device equals it bit for bit.  ``captures`` stays 1 and ``push`` never waits.  Not
together with ``out_fps`` (ValueError: several rows per push).  No accuracy figure is claimed.  ``bones=None`` is the session above, bit
for bit: no further launch or buffer."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import ptr as _ptr
from .roots import _root_lens
from .tracks import _host_array, _upload


MAX_BONE_JOINTS = 64                                                  # kBonesMaxJoints


class Skeleton(object):
    """The tree of a joint layout: ``parents`` is a length-J integer sequence, ``parents[j]`` the joint that joint j hangs on and -1 for the
    ONE tree root; every other entry in [0, J), no cycles, J <= 64.  Anything else is a ValueError.  Derived --
        ``root``    the tree root;
        ``order``   all joints, every parent in front of its children: again and again the lowest joint whose parent is placed already;
        ``paths``   per joint j the non-root joints on the way from the root down to j, j included, root side first (the root's is empty);
        ``depth``   the longest path (at least 1: the second dimension of the device table).
    Immutable; the tables are made once and uploaded once per device (``device_tables``), as a ``KeypointMap``'s."""

    def __init__(self, parents):
        try:
            a = np.asarray(parents)
        except (TypeError, ValueError):
            raise ValueError(f"Skeleton takes a sequence of J parent indices, got {parents!r}") from None
        if a.ndim != 1 or a.dtype.kind not in "iu" or not 1 <= len(a) <= MAX_BONE_JOINTS:
            raise ValueError(f"Skeleton takes a sequence of 1 to {MAX_BONE_JOINTS} integer parent indices (J <= {MAX_BONE_JOINTS}), got "
                             f"{'shape ' + str(a.shape) + ' of ' + str(a.dtype) if a.ndim else repr(parents)}")
        p = [int(v) for v in a]
        J = len(p)
        roots = [j for j, v in enumerate(p) if v == -1]
        if len(roots) != 1:
            raise ValueError(f"Skeleton needs exactly one -1, the tree root, got {len(roots)}")
        for j, v in enumerate(p):
            if v != -1 and not 0 <= v < J:
                raise ValueError(f"Skeleton: the parent of joint {j} must be -1 or in [0, {J}), got {v}")
        paths = []
        for j in range(J):
            up, a_ = [], j
            while p[a_] != -1:
                up.append(a_)
                a_ = p[a_]
                if len(up) > J:
                    raise ValueError(f"Skeleton: joint {j} never reaches the root: the parents form a cycle")
            paths.append(tuple(reversed(up)))
        placed, order = {roots[0]}, [roots[0]]
        while len(order) < J:
            nxt = min(j for j in range(J) if j not in placed and p[j] in placed)
            placed.add(nxt)
            order.append(nxt)
        self.parents, self.joints, self.root = tuple(p), J, roots[0]
        self.order, self.paths = tuple(order), tuple(paths)
        self.depth = max(1, max(len(q) for q in paths))
        self._tables = {}

    def tables(self):
        """-> (parents (J,) int32, paths (J, depth) int32 with -1 behind a joint's last entry): what the device reads."""
        paths = np.full((self.joints, self.depth), -1, np.int32)
        for j, q in enumerate(self.paths):
            paths[j, :len(q)] = q
        return np.array(self.parents, np.int32), paths

    def device_tables(self, device):
        """The two tables on ``device``: uploaded at the first call, which waits for the copy once -- whatever stream uses them later finds
        them there --, and kept for the life of the skeleton."""
        import torch
        key = str(torch.device(device))
        if key not in self._tables:
            parents, paths = self.tables()
            both = _upload(np.concatenate([parents, paths.reshape(-1)]), np.int32, device)
            torch.cuda.current_stream(device).synchronize()
            self._tables[key] = (both[:self.joints], both[self.joints:].view(self.joints, self.depth))
        return self._tables[key]

    def __repr__(self):
        return f"Skeleton(joints={self.joints}, root={self.root})"


# The tree of H36MOrder17P (the layout of ``_h36m17_from``), the pelvis as root: right leg ankle -> knee -> hip -> pelvis, left leg
# likewise, spine torso -> pelvis, neck -> torso, head -> neck, head top -> head, arms wrist -> elbow -> shoulder -> neck.  It commutes
# with AUGM_FLIP_KEYPOINT_ORDER: parents[flip[j]] == flip[parents[j]].
SKELETONS = {
    "h36m17": Skeleton([1, 2, 6, 6, 3, 4, -1, 8, 6, 7, 9, 12, 13, 7, 7, 14, 15]),
}


def skeleton_of(skeleton, J=None):
    """A name of ``SKELETONS`` or a ``Skeleton`` -> the ``Skeleton``; ``J``: the joint count it must have (ValueError naming ``Skeleton``)."""
    if isinstance(skeleton, str):
        if skeleton not in SKELETONS:
            raise ValueError(f"skeleton must be a Skeleton or one of {sorted(SKELETONS)}, got {skeleton!r}")
        sk, what = SKELETONS[skeleton], repr(skeleton)
    elif isinstance(skeleton, Skeleton):
        sk, what = skeleton, repr(skeleton)
    else:
        raise ValueError(f"skeleton must be a Skeleton or one of {sorted(SKELETONS)}, got {skeleton!r}")
    if J is not None and sk.joints != int(J):
        raise ValueError(f"the skeleton {what} has {sk.joints} joints, the poses have {int(J)}: describe the layout's tree with "
                         f"predict.Skeleton(parents) and pass predict.Bones(lengths, skeleton=...)")
    return sk


class Bones(object):
    """``bones=`` with a tree of your own: ``lengths`` is "track" (measure every track, or slot, itself), a (J,) array of lengths in the
    poses' units, indexed by CHILD joint (the root's entry is ignored), or a list of such arrays, one per track or slot; ``skeleton``: a
    name of ``SKELETONS`` or a ``Skeleton``."""
    __slots__ = ("lengths", "skeleton")

    def __init__(self, lengths="track", skeleton="h36m17"):
        self.lengths, self.skeleton = lengths, skeleton_of(skeleton)

    def __repr__(self):
        return f"Bones(lengths={self.lengths!r}, skeleton={self.skeleton!r})"


def check_bones(bones, count, J, root=None, per="track"):
    """``bones`` of ``predict_tracks`` / ``StreamSession`` -> None (no fix) or (skeleton, lengths): lengths None for "track", else a
    (count, J) float64 array, the root's column 0.  ``J``: the joints of the poses; ``root``: the joint that is subtracted from the returned
    poses, or None when they are not root-relative -- the tree root must be that joint, so that it stays exactly 0."""
    if bones is None:
        return None
    b = bones if isinstance(bones, Bones) else Bones.__new__(Bones)
    if not isinstance(bones, Bones):
        b.lengths, b.skeleton = bones, "h36m17"
    sk = skeleton_of(b.skeleton, J)
    if root is not None and sk.root != int(root):
        raise ValueError(f"bones: the tree root of the skeleton is joint {sk.root}, but the poses are relative to joint {int(root)} "
                         f"(ROOT_KEYTPOINT): rebuilt from another root, that joint would not stay 0")
    if isinstance(b.lengths, str):
        if b.lengths != "track":
            raise ValueError(f'bones must be None, "track", a ({int(J)},) array of lengths, one such array per {per} or a predict.Bones, got {b.lengths!r}')
        return sk, None
    try:
        L = np.array([np.asarray(_host_array(v), np.float64) for v in b.lengths] if isinstance(b.lengths, (list, tuple)) and len(b.lengths)
                     and np.ndim(b.lengths[0]) else _host_array(b.lengths), np.float64)
    except (TypeError, ValueError):
        raise ValueError(f'bones must be None, "track", a ({int(J)},) array of lengths, one such array per {per} or a predict.Bones') from None
    if L.shape == (int(J),):
        L = np.tile(L, (int(count), 1))
    if L.shape != (int(count), int(J)):
        raise ValueError(f"bones: the lengths must be ({int(J)},) or one such array per {per} ({int(count)}), got shape {L.shape}")
    L = np.ascontiguousarray(L)
    L[:, sk.root] = 0.0
    return sk, L


def _bone_offsets(X, sk):
    """(G, J, 3) float32 poses -> (d (G, J, 3) float64: x[j] - x[parent of j], zeros for the root; len (G, J) float64)."""
    X64 = X.astype(np.float64)
    par = np.array(sk.parents, np.int64)
    d = X64 - X64[:, np.where(par >= 0, par, np.arange(sk.joints))]
    return X64, d, np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def _bone_poses(poses, skeleton):
    X = np.asarray(_host_array(poses), np.float32)
    if X.ndim != 3 or X.shape[2] != 3:
        raise ValueError(f"poses must be (G, J, 3), got {X.shape}")
    return X, skeleton_of(skeleton, X.shape[1])


def bone_lengths_host(poses, lens=None, skeleton="h36m17", return_counts=False):
    """The length rule of CONSTANT BONE LENGTHS (include/uu3d.h) in numpy, written to be read: what uu3d_bone_lengths computes, bit for
    bit.  ``poses`` (G, J, 3) float32: the rows of all tracks back to back; ``lens``: rows per track (None: one track)
    -> lengths (tracks, J) float64, indexed by CHILD joint: the mean of the bone's length over the track's frames where it is finite
    and > 0, summed in ascending frame order as a plain loop (np.sum adds pairwise); NaN where there is no such frame ("not corrected");
    0 for the tree root.  ``return_counts``: -> (lengths, counts (tracks, J) int64)."""
    X, sk = _bone_poses(poses, skeleton)
    lens = _root_lens(lens, len(X))
    is_bone = np.array(sk.parents) >= 0
    L, N = np.zeros((len(lens), sk.joints), np.float64), np.zeros((len(lens), sk.joints), np.int64)
    with np.errstate(all="ignore"):
        _, _, ln = _bone_offsets(X, sk)
        first = 0
        for t, n in enumerate(lens.tolist()):
            total, count = np.zeros(sk.joints, np.float64), np.zeros(sk.joints, np.int64)
            for i in range(first, first + n):
                ok = is_bone & np.isfinite(ln[i]) & (ln[i] > 0)
                total = np.where(ok, total + ln[i], total)
                count += ok
            L[t] = np.where(is_bone, np.where(count > 0, total / count.astype(np.float64), np.nan), 0.0)
            N[t] = count
            first += n
    return (L, N) if return_counts else L


def _bone_length_table(lengths, tracks, J):
    L = np.asarray(_host_array(lengths), np.float64)
    if L.shape == (J,):
        L = np.tile(L, (tracks, 1))
    if L.shape != (tracks, J):
        raise ValueError(f"lengths must be ({J},) or ({tracks}, {J}): one row per track, got {L.shape}")
    return np.ascontiguousarray(L)


def fix_bones_host(poses, lens, lengths, skeleton="h36m17"):
    """The fix of CONSTANT BONE LENGTHS in numpy, written to be read: what uu3d_fix_bones computes, bit for bit.  ``poses`` (G, J, 3)
    float32, ``lens`` as ``bone_lengths_host``; ``lengths`` (J,) or (tracks, J) float64 by child joint -> the rebuilt poses, float32.
    The root keeps its bits.  Every other joint j: acc = x[root] widened, then per joint a on ``skeleton.paths[j]``, root side first,
    ``acc = acc + d(a) * s(a)`` with ``s(a) = L[a] / len(a)`` where L[a] and len(a) are finite and > 0, else 1.0; the result is acc
    rounded once.  A product and a sum are two roundings (no fused multiply-add); the joints of a path are a plain loop."""
    X, sk = _bone_poses(poses, skeleton)
    lens = _root_lens(lens, len(X))
    L = np.repeat(_bone_length_table(lengths, len(lens), sk.joints), lens, axis=0)        # (G, J): the lengths of each row's track
    out = X.copy()
    with np.errstate(all="ignore"):
        X64, d, ln = _bone_offsets(X, sk)
        ok = np.isfinite(L) & (L > 0) & np.isfinite(ln) & (ln > 0)
        s = np.where(ok, L / np.where(ok, ln, 1.0), 1.0)
        for j in sk.order[1:]:
            acc = X64[:, sk.root].copy()
            for a in sk.paths[j]:
                acc = acc + d[:, a] * s[:, a, None]
            out[:, j] = acc.astype(np.float32)
    return out


def _bone_device_poses(poses, skeleton):
    import torch
    if not isinstance(poses, torch.Tensor) or poses.dim() != 3 or poses.shape[2] != 3 or poses.dtype != torch.float32 or not poses.is_contiguous() \
            or not poses.is_cuda:
        raise ValueError(f"poses must be a contiguous (G, J, 3) float32 device tensor, got {tuple(getattr(poses, 'shape', ()))}")
    return skeleton_of(skeleton, int(poses.shape[1]))


def bone_lengths(poses, lens=None, skeleton="h36m17", return_counts=False):
    """uu3d_bone_lengths on the current stream: ``bone_lengths_host`` on a device tensor, one launch, nothing copies to the host or waits
    (the per-track plan goes up pinned and asynchronously).  ``poses``: a contiguous (G, J, 3) float32 device tensor, only read
    -> lengths (tracks, J) float64 on the device (``return_counts``: and counts (tracks, J) int64).  Also the calibration helper: the
    lengths of one recording are what ``bones=`` takes for the next."""
    import torch
    sk = _bone_device_poses(poses, skeleton)
    lib = _capi.load_library()
    dev, G, J = poses.device, int(poses.shape[0]), sk.joints
    lens = _root_lens(lens, G)
    T = len(lens)
    L = torch.zeros((T, J), dtype=torch.float64, device=dev)
    N = torch.zeros((T, J), dtype=torch.int64, device=dev) if return_counts else None
    parents, _ = sk.device_tables(dev)
    plan = _upload(np.stack([np.concatenate([[0], np.cumsum(lens)[:-1]]), lens]), np.int64, dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        if G == 0:                                                    # (no rows: the library launches nothing; a track without rows is "not corrected")
            L.fill_(float("nan"))
            L[:, sk.root] = 0.0
        _capi.check(lib, lib.uu3d_bone_lengths(_ptr(poses), G, J, _ptr(parents), _ptr(plan[0]), _ptr(plan[1]), T, _ptr(L), _ptr(N),
                                               C.c_void_p(stream)), None)
    return (L, N) if return_counts else L


def fix_bones(poses, lens, lengths, skeleton="h36m17"):
    """uu3d_fix_bones on the current stream: ``fix_bones_host`` on a device tensor, one launch, nothing copies to the host or waits.
    ``poses``: a contiguous (G, J, 3) float32 device tensor, only read; ``lengths``: what ``bone_lengths`` returned -- a contiguous
    (tracks, J) float64 device tensor -- or a host array (J,) / (tracks, J) -> the rebuilt poses, a fresh device tensor."""
    import torch
    sk = _bone_device_poses(poses, skeleton)
    lib = _capi.load_library()
    dev, G, J = poses.device, int(poses.shape[0]), sk.joints
    lens = _root_lens(lens, G)
    T = len(lens)
    if isinstance(lengths, torch.Tensor) and lengths.is_cuda:
        if tuple(lengths.shape) != (T, J) or lengths.dtype != torch.float64 or not lengths.is_contiguous() or lengths.device != dev:
            raise ValueError(f"lengths must be a contiguous ({T}, {J}) float64 tensor on the poses' device, got {tuple(lengths.shape)} of {lengths.dtype}")
    else:
        lengths = _upload(_bone_length_table(lengths, T, J), np.float64, dev)
    out = torch.empty_like(poses)
    if G == 0:
        return out
    parents, paths = sk.device_tables(dev)
    row_track = None if T == 1 else _upload(np.repeat(np.arange(T, dtype=np.int32), lens), np.int32, dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(lib, lib.uu3d_fix_bones(_ptr(poses), _ptr(out), G, J, _ptr(parents), _ptr(paths), sk.depth, _ptr(row_track), T, _ptr(lengths),
                                            C.c_void_p(stream)), None)
    return out


class LiveBonesHost(object):
    """The rule of uu3d_stream_bones in numpy, written to be read: the live form of ``predict.bone_lengths_host`` / ``fix_bones_host``.
    State per slot and joint -- ``total`` (float64), the sum of the bone's lengths, and ``count``, how many were added.
    ``step(poses (slots, J, 3) float32, fresh (slots,), active (slots,) or None)`` -> the rebuilt poses (slots, J, 3) float32.
      ``lengths=None`` ("track"): an active slot whose pose is fresh first adds the finite, positive length of each of its bones to the
          sum and counts it; the slot's L is sum / count -- NaN ("not corrected") before the first one, 0 for the tree root.  The mean is
          CAUSAL: it equals ``predict.bone_lengths_host`` on the fresh poses seen so far, not the mean of the whole track.
      ``lengths`` (J,) or (slots, J): L is what was given, and there is no state.
      Then EVERY slot, fresh or not, returns ``predict.fix_bones_host`` of its row with its L: a pure function of the raw pose and the
      slot's lengths, so a slot that holds its previous raw pose returns its previous fixed pose bit for bit.
    ``drain(poses, fresh, chosen)``: one drain tick of ``StreamSession.finish`` -- ``step`` with the chosen slots as ``active``.
    ``lengths``: the (slots, J) float64 table after the last step.  ``reset(slots=None)``: the chosen slots' sums and counts are zero."""

    def __init__(self, slots, skeleton="h36m17", lengths=None):
        self.slots, self.skeleton = int(slots), skeleton_of(skeleton)
        J = self.skeleton.joints
        self.given = None if lengths is None else check_bones(Bones(lengths, self.skeleton), self.slots, J, per="slot")[1]
        self.total, self.count = np.zeros((self.slots, J), np.float64), np.zeros((self.slots, J), np.int64)
        self.lengths = self._table()

    def _table(self):
        if self.given is not None:
            return self.given.copy()
        is_bone = np.array(self.skeleton.parents) >= 0
        with np.errstate(all="ignore"):
            return np.where(is_bone, np.where(self.count > 0, self.total / self.count.astype(np.float64), np.nan), 0.0)

    def reset(self, slots=None):
        which = slice(None) if slots is None else np.asarray(slots, np.int64).reshape(-1)
        self.total[which] = 0
        self.count[which] = 0
        self.lengths = self._table()

    def step(self, poses, fresh, active=None):
        J = self.skeleton.joints
        X = np.asarray(poses, np.float32).reshape(self.slots, J, 3)
        fresh = np.asarray(fresh).reshape(self.slots) != 0
        active = np.ones(self.slots, bool) if active is None else np.asarray(active).reshape(self.slots) != 0
        if self.given is None:
            is_bone = np.array(self.skeleton.parents) >= 0
            with np.errstate(all="ignore"):
                ln = _bone_offsets(X, self.skeleton)[2]
                ok = (active & fresh)[:, None] & is_bone & np.isfinite(ln) & (ln > 0)
                self.total = np.where(ok, self.total + ln, self.total)
                self.count = self.count + ok
        self.lengths = self._table()
        return fix_bones_host(X, np.ones(self.slots, np.int64), self.lengths, self.skeleton)

    def drain(self, poses, fresh, chosen=None):
        return self.step(poses, fresh, chosen)


class LiveBones(object):
    """uu3d_stream_bones as an output-side stage of a ``StreamSession`` (the interface: ``smooth.LiveOneEuro``); ``given``: None = "track"."""

    def __init__(self, slots, joints, skeleton, given, device):
        import torch
        self._lib = _capi.load_library()
        size = int(self._lib.uu3d_stream_bones_bytes(slots, joints))
        if size == 0:
            raise ValueError(f"bones: slots = {slots}, joints = {joints} are out of uu3d_stream_bones' range")
        self.slots, self.joints, self.depth = slots, joints, skeleton.depth
        self._tables = skeleton.device_tables(device)
        self._state = torch.zeros(size, dtype=torch.uint8, device=device)
        self._given = None if given is None else _upload(given, given.dtype, device)
        self.lengths = torch.zeros((slots, joints), dtype=torch.float64, device=device)
        self.out = torch.zeros((slots, joints, 3), dtype=torch.float32, device=device)
        self.outputs = (("poses", "fixed_poses", self.out),)

    def launch(self, active, frames=None, drain_state=None):
        parents, paths = self._tables
        return (self._lib.uu3d_stream_bones, (self.slots, self.joints, _ptr(self._state), _ptr(parents), _ptr(paths), self.depth, _ptr(active),
                                              _ptr(self.read.fresh), _ptr(self.read.poses), _ptr(self._given), _ptr(self.out), _ptr(self.lengths)))

    def reset_launch(self):
        return (self._lib.uu3d_stream_bones_reset, (self.slots, self.joints, _ptr(self._state)))
