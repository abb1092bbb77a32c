"""The rotations stage of the track pipeline: per-joint quaternions of every pose (include/uu3d.h, JOINT ROTATIONS).  Wraps
uu3d_joint_rotations (``joint_rotations``; the rule in numpy: ``joint_rotations_host``); ``quat_to_matrix`` and ``forward_kinematics`` are
host helpers, ``bvh.write_bvh`` writes the result as a BVH file.

Joint rotations: ``predict_tracks`` and ``StreamSession`` return joint POSITIONS; a character rig, a game engine or a BVH file takes
ROTATIONS.  ``predict_tracks(..., rotations=True)`` appends, per track, one unit quaternion (w, x, y, z; v' = q v q*) per frame and
joint -- joint j's rotation relative to its parent's frame, the root's relative to the pose's space -- computed on the device from the
RETURNED poses (behind ``bones``, behind ``smooth``, at the returned frame times) in one launch over all tracks' rows.  The quaternions
turn a REST POSE onto the pose: ``rotations=Rotations(rest, skeleton=..., primary=..., secondary=...)`` gives the rest pose -- the
direction of every bone by child joint, only directions matter -- of any ``Skeleton``; ``True`` is ``Rotations("h36m17")``, a T-pose in
the camera's convention (``REST_POSES``: a convenience, not a tuned or claimed value).  A joint with one child turns its rest bone onto
the pose's bone by the shortest arc; a joint with more children then twists about that PRIMARY bone until its SECONDARY child is where
the pose has it.  WHAT THE RULE CANNOT SEE: positions do not show the twist about a bone with a single child -- it is zero relative to
the parent --, so the orientation of the head, hand and foot segments is limited.  Together with ``bones`` (rigid lengths) forward
kinematics of the quaternions gives the poses back (``forward_kinematics``).  No accuracy figure is claimed: the mechanism is the
feature.  ``rotations=None`` is the call before, bit for bit: no further launch or buffer.

Live joint rotations -- ``StreamSession(..., rotations=R)``: ONE more launch, the LAST step of the one captured tick, behind the bone fix,
the root solve and the filters: uu3d_joint_rotations reads the pose buffer ``push`` returns and writes a (slots, J, 4) buffer of the
session's own, which ``push`` / ``push_detections`` append to what they return.  A slot that is not fresh keeps its previous quaternions,
before a slot's first pose they are identities, ``reset`` and a birth at a ``push_detections`` tick set them back to identities on the
device, ``finish`` runs the same step in every drain tick.  The stage has no state: the result is ``joint_rotations`` of the pose that
``push`` returned, bit for bit.  ``captures`` stays 1 and ``push`` never waits.  Not together with ``out_fps`` (ValueError: several rows
per push)."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import ptr as _ptr
from .bones import skeleton_of
from .tracks import _host_array, _upload

# Rest poses by name: (J, 3), the direction of the bone from joint j's parent to j, by CHILD joint (the root's row is ignored).
# "h36m17": a T-pose of ``SKELETONS["h36m17"]`` in the camera's convention (x right, y down, z forward) for a person who faces the
# camera: the legs point along +y, spine, neck and head along -y, the right arm and hip along -x, the left ones along +x.
REST_POSES = {
    "h36m17": np.array([[0, 1, 0], [0, 1, 0], [-1, 0, 0], [1, 0, 0], [0, 1, 0], [0, 1, 0], [0, 0, 0], [0, -1, 0], [0, -1, 0], [0, -1, 0],
                        [0, -1, 0], [-1, 0, 0], [-1, 0, 0], [-1, 0, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0]], np.float64),
}
# ... and the primary / secondary children that go with a named rest pose where the two lowest child indices would not do: the pelvis
# of "h36m17" (joint 6) has the two hips as its lowest children, which are collinear in a T-pose, so it takes the spine and the left hip.
REST_CHILDREN = {
    "h36m17": ({6: 8}, {6: 3}),
}


class Rotations(object):
    """``rotations=`` of ``predict_tracks`` / ``StreamSession``, and what ``joint_rotations`` takes: a rest pose on a tree.
    ``rest``: a name of ``REST_POSES`` or a (J, 3) array, the offset of joint j from its parent in the rest pose, by CHILD joint (the
    root's row is ignored); only directions matter: every row is normalised, r / sqrt((r0 r0 + r1 r1) + r2 r2) in float64.  A zero or
    non-finite row of a non-root joint is a ValueError.  ``skeleton``: a name of ``SKELETONS`` or a ``Skeleton`` (J <= 64).
    ``primary`` / ``secondary``: None, a dict {joint: child} or a length-J sequence (-1: the default) naming, for joints with children,
    the child whose bone the joint's rotation follows and, for joints with two or more, the child that fixes the twist about that bone;
    the default is the two lowest child indices (for a named rest pose: ``REST_CHILDREN``).  A joint that is not a child of the joint
    it is named for, or a secondary child equal to the primary one, is a ValueError, and so is a secondary child whose rest bone is
    exactly parallel to the primary one's (it fixes no twist).  ``return_global``: also return the global quaternions.
    Derived -- ``primary`` / ``secondary`` / ``level`` (J,) int arrays (-1: no such child; level: bones between joint and root),
    ``depth`` the largest level, ``rest`` the (J, 3) float64 unit directions (zeros for the root).  Immutable; the tables are made once
    and uploaded once per device (``device_tables``), as a ``Skeleton``'s."""

    def __init__(self, rest="h36m17", skeleton="h36m17", primary=None, secondary=None, return_global=False):
        sk = self.skeleton = skeleton_of(skeleton)
        J = sk.joints
        named = isinstance(rest, str)
        if named:
            if rest not in REST_POSES:
                raise ValueError(f"rest must be a ({J}, 3) array or one of {sorted(REST_POSES)}, got {rest!r}")
            r = REST_POSES[rest]
        else:
            try:
                r = np.array(_host_array(rest), np.float64)
            except (TypeError, ValueError):
                raise ValueError(f"rest must be a ({J}, 3) array or one of {sorted(REST_POSES)}") from None
        if r.shape != (J, 3):
            raise ValueError(f"the rest pose has shape {r.shape}, the skeleton {sk!r} needs ({J}, 3): one bone direction per child joint")
        r = r.copy()
        r[sk.root] = 0.0
        with np.errstate(all="ignore"):
            n = np.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2])
        bad = [j for j in range(J) if j != sk.root and not (np.isfinite(n[j]) and n[j] > 0)]
        if bad:
            raise ValueError(f"rest: the row of joint {bad[0]} is zero or not finite: a bone needs a direction in the rest pose")
        n[sk.root] = 1.0
        self.rest = r / n[:, None]
        children = [[c for c in range(J) if sk.parents[c] == j] for j in range(J)]
        preset = REST_CHILDREN.get(rest, ({}, {})) if named and primary is None and secondary is None else ({}, {})
        first = self._named_children(primary, preset[0], "primary", children)
        second = self._named_children(secondary, preset[1], "secondary", children)
        self.primary, self.secondary = np.full(J, -1, np.int32), np.full(J, -1, np.int32)
        for j in range(J):
            if not children[j]:
                continue
            c1, c2 = first.get(j), second.get(j)
            if c1 is None:
                c1 = min([c for c in children[j] if c != c2] or children[j])
            if c1 == c2:
                raise ValueError(f"secondary: joint {c2} is the primary child of joint {j}: the secondary child must be another one")
            self.primary[j] = c1
            others = [c for c in children[j] if c != c1]
            if others:
                c2 = self.secondary[j] = others[0] if c2 is None else c2
                a, b = self.rest[c1], self.rest[c2]
                if not np.any(np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])):
                    raise ValueError(f"rest: the bones to joint {j}'s primary child {c1} and secondary child {c2} are parallel in the rest "
                                     f"pose, so the second fixes no twist about the first: name another child (primary= / secondary=)")
        self.level = np.array([len(q) for q in sk.paths], np.int32)
        self.depth = int(self.level.max())
        self.return_global = bool(return_global)
        self._tables = {}

    @staticmethod
    def _named_children(given, preset, what, children):
        J = len(children)
        if given is None:
            named = dict(preset)
        elif isinstance(given, dict):
            named = {int(k): int(v) for k, v in given.items()}
        else:
            a = np.asarray(given)
            if a.shape != (J,) or a.dtype.kind not in "iu":
                raise ValueError(f"{what} must be None, a dict {{joint: child}} or {J} integers (-1: the default), got {given!r}")
            named = {j: int(v) for j, v in enumerate(a) if v != -1}
        for j, c in named.items():
            if not 0 <= j < J or c not in children[j]:
                raise ValueError(f"{what}: joint {c} is not a child of joint {j} (its children: {children[j] if 0 <= j < J else []})")
        return named

    def tables(self):
        """-> (tree (4, J) int32: parents, primary child, secondary child, level; rest (J, 3) float64): what the device reads."""
        return np.stack([np.array(self.skeleton.parents, np.int32), self.primary, self.secondary, self.level]).astype(np.int32), self.rest

    def device_tables(self, device):
        """The two tables on ``device``: uploaded at the first call, which waits for the copy once, and kept for the life of the object."""
        import torch
        key = str(torch.device(device))
        if key not in self._tables:
            tree, rest = self.tables()
            self._tables[key] = (_upload(tree, np.int32, device), _upload(rest, np.float64, device))
            torch.cuda.current_stream(device).synchronize()
        return self._tables[key]

    def __repr__(self):
        return f"Rotations(skeleton={self.skeleton!r}, return_global={self.return_global})"


_NAMED = {}


def rotations_of(skeleton="h36m17", rest="h36m17", primary=None, secondary=None, return_global=False):
    """What ``joint_rotations`` and ``joint_rotations_host`` take -> a ``Rotations``: ``skeleton`` may be one already (the other arguments
    are then ignored but ``return_global``, which is ORed in by the caller); a rest pose and a skeleton given by name are made once."""
    if isinstance(skeleton, Rotations):
        return skeleton
    if isinstance(rest, str) and isinstance(skeleton, str) and primary is None and secondary is None:
        if (rest, skeleton) not in _NAMED:
            _NAMED[rest, skeleton] = Rotations(rest, skeleton)
        return _NAMED[rest, skeleton]
    return Rotations(rest, skeleton, primary, secondary, return_global)


def check_rotations(rotations, J):
    """``rotations`` of ``predict_tracks`` / ``StreamSession`` -> None (no such stage) or a ``Rotations``: True is ``Rotations("h36m17")``.
    ``J``: the joints of the poses -- another count than the skeleton's is a ValueError."""
    if rotations is None or rotations is False:
        return None
    if rotations is True:
        rotations = rotations_of()
    if not isinstance(rotations, Rotations):
        raise ValueError(f"rotations must be None, True or a predict.Rotations(rest, skeleton=...), got {rotations!r}")
    if rotations.skeleton.joints != int(J):
        raise ValueError(f"rotations: the skeleton {rotations.skeleton!r} has {rotations.skeleton.joints} joints, the poses have {int(J)}: describe "
                         f"the layout's tree with predict.Skeleton(parents) and pass predict.Rotations(rest, skeleton=...)")
    return rotations


# ---- the rule in numpy: arrays of quaternions (..., 4) as (w, x, y, z) and of vectors (..., 3), every operation written out ------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _mul(a, b):
    aw, ax, ay, az = (a[..., k] for k in range(4))
    bw, bx, by, bz = (b[..., k] for k in range(4))
    return np.stack([((aw * bw - ax * bx) - ay * by) - az * bz, ((aw * bx + ax * bw) + ay * bz) - az * by,
                     ((aw * by - ax * bz) + ay * bw) + az * bx, ((aw * bz + ax * by) - ay * bx) + az * bw], -1)


def _unit(q):
    n = np.sqrt(((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) + q[..., 3] * q[..., 3])
    return q / n[..., None]


def _conj(q):
    return np.stack([q[..., 0], -q[..., 1], -q[..., 2], -q[..., 3]], -1)


def _rotate(q, v):
    t = 2.0 * _cross(q[..., 1:], v)
    return (v + q[..., :1] * t) + _cross(q[..., 1:], t)


def _arc(a, b, axis=None):
    w = np.sqrt(_dot(a, a)) * np.sqrt(_dot(b, b)) + _dot(a, b)
    c = _cross(a, b)
    anti = (w <= 0.0) & (c[..., 0] == 0.0) & (c[..., 1] == 0.0) & (c[..., 2] == 0.0)
    if axis is None:                                                  # a x e, e the axis of a's smallest-magnitude component
        m = np.abs(a[..., 0])
        k1 = np.abs(a[..., 1]) < m
        m = np.where(k1, np.abs(a[..., 1]), m)
        k = np.where(np.abs(a[..., 2]) < m, 2, np.where(k1, 1, 0))
        axis = np.stack([np.where(k == 0, 0.0, np.where(k == 1, -a[..., 2], a[..., 1])),
                         np.where(k == 0, a[..., 2], np.where(k == 1, 0.0, -a[..., 0])),
                         np.where(k == 0, -a[..., 1], np.where(k == 1, a[..., 0], 0.0))], -1)
    return _unit(np.concatenate([np.where(anti, 0.0, w)[..., None], np.where(anti[..., None], axis, c)], -1))


def _usable(v):
    return np.isfinite(v).all(-1) & ~((v[..., 0] == 0.0) & (v[..., 1] == 0.0) & (v[..., 2] == 0.0))


def _host_poses(poses, J):
    X = np.asarray(_host_array(poses), np.float32)
    if X.ndim != 3 or X.shape[2] != 3:
        raise ValueError(f"poses must be (G, J, 3), got {X.shape}")
    if X.shape[1] != J:
        raise ValueError(f"the skeleton has {J} joints, the poses have {X.shape[1]}")
    return X


def joint_rotations_host(poses, skeleton="h36m17", rest="h36m17", primary=None, secondary=None, return_global=False, rounded=True,
                         exact_input=False):
    """The rule of JOINT ROTATIONS (include/uu3d.h) in numpy, written to be read: what uu3d_joint_rotations computes, bit for bit.  This
    docstring is the normative text.

    ``poses`` (G, J, 3) float32; ``skeleton`` / ``rest`` / ``primary`` / ``secondary`` as ``Rotations`` takes them (or a ``Rotations`` in
    ``skeleton``'s place) -> (local (G, J, 4) float32, flags (G, J) uint8), with ``return_global`` (local, flags, global (G, J, 4)
    float32).  Quaternions are (w, x, y, z), unit, and turn a vector as v' = q v q*.  ``local[g, j]`` is joint j's rotation relative to
    its parent's frame, the root's relative to the pose's space; ``flags``: 1 = determined from the pose, 0 = fell back.
    ``rounded=False``: the float64 quaternions before the one rounding to float32 (not a device output; for tests and for judging).
    ``exact_input=True``: ``poses`` is taken as the float64 array it is instead of being rounded to float32 first (not a device path
    either: it shows what the rule does with a pose that float32 cannot hold exactly, such as a rotated one).

    Arithmetic: float64; every product, sum, difference, quotient and square root is rounded once, in the order written; no fused
    multiply-add; no trigonometry.
        dot(a, b) = (a0 b0 + a1 b1) + a2 b2       cross(a, b) = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0)       |a| = sqrt(dot(a, a))
        mul(a, b):  w = ((aw bw - ax bx) - ay by) - az bz      x = ((aw bx + ax bw) + ay bz) - az by
                    y = ((aw by - ax bz) + ay bw) + az bx      z = ((aw bz + ax by) - ay bx) + az bw
        unit(q) = q / sqrt(((w w + x x) + y y) + z z), component by component
        rotate(q, v):  t = 2 cross(q.xyz, v);  v'_c = (v_c + q.w t_c) + cross(q.xyz, t)_c
        arc(a, b) = unit((|a| |b| + dot(a, b), cross(a, b))): the shortest arc from a onto b.  ANTIPARALLEL -- the scalar part <= 0 and
            all three components of the cross product == 0 --: a half turn, unit((0, cross(a, e))), e the coordinate axis of a's
            smallest-magnitude component, ties to the lowest index; inside the twist below the half turn is about the primary bone,
            unit((0, u)), the one axis that leaves that bone where it is.
    Per frame, joints in tree order (``skeleton.order``: every parent before its children); Qpar is the parent's global quaternion Q,
    (1, 0, 0, 0) for the tree root; rest[c] is the unit rest direction of the bone to child c:
      * p has no child: Q[p] = Qpar, local[p] = (1, 0, 0, 0) exactly, flag 1.
      * otherwise b = x[c1] - x[p], widened to float64 first, c1 = p's primary child.  If |b| is not finite or not > 0 the bone is
        DEGENERATE: Q[p] = Qpar, local[p] = (1, 0, 0, 0) exactly, flag 0.  Else flag 1 and
            Q1 = unit(mul(arc(rotate(Qpar, rest[c1]), b), Qpar)).
      * p has a secondary child c2: u = b / |b|; s = rotate(Q1, rest[c2]) and t = x[c2] - x[p] are projected onto the plane across the
        primary bone, s_c = s_c - u_c dot(s, u) and t likewise.  Where both projections are finite and neither is all == 0,
            Q[p] = unit(mul(arc(s, t), Q1)),
        a twist about the primary bone; otherwise the twist is the identity, Q[p] = Q1, and the flag stays 1.  Without c2, Q[p] = Q1.
      * local[p] = unit(mul(conj(Qpar), Q[p])), negated as a whole where w < 0, or w == 0 and the first non-zero of x, y, z is negative;
        then every component is rounded once to float32.  global[p] is Q[p] rounded to float32, with the sign it came out with.
    The twist about a bone with a single child is not visible in positions: by this rule it is zero relative to the parent."""
    R = rotations_of(skeleton, rest, primary, secondary)
    sk = R.skeleton
    X = _host_poses(poses, sk.joints).astype(np.float64)
    if exact_input:
        X = np.asarray(_host_array(poses), np.float64)
    G, J = X.shape[0], sk.joints
    one = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (G, 1))
    Q, local, flags = np.tile(one[:, None], (1, J, 1)), np.tile(one[:, None], (1, J, 1)), np.ones((G, J), np.uint8)
    with np.errstate(all="ignore"):
        for p in sk.order:
            par = one if sk.parents[p] < 0 else Q[:, sk.parents[p]]
            c1, c2 = int(R.primary[p]), int(R.secondary[p])
            if c1 < 0:
                Q[:, p] = par
                continue
            b = X[:, c1] - X[:, p]
            nb = np.sqrt(_dot(b, b))
            ok = np.isfinite(nb) & (nb > 0)
            q = _unit(_mul(_arc(_rotate(par, R.rest[c1]), b), par))
            if c2 >= 0:
                u = b / nb[:, None]
                s, t = _rotate(q, R.rest[c2]), X[:, c2] - X[:, p]
                s, t = s - u * _dot(s, u)[:, None], t - u * _dot(t, u)[:, None]
                twisted = _unit(_mul(_arc(s, t, axis=u), q))
                q = np.where((_usable(s) & _usable(t))[:, None], twisted, q)
            loc = _unit(_mul(_conj(par), q))
            w, x, y, z = (loc[:, k] for k in range(4))
            negative = (w < 0) | ((w == 0) & ((x < 0) | ((x == 0) & ((y < 0) | ((y == 0) & (z < 0))))))
            loc = np.where(negative[:, None], -loc, loc)
            Q[:, p] = np.where(ok[:, None], q, par)
            local[:, p] = np.where(ok[:, None], loc, one)
            flags[:, p] = ok
    if rounded:
        Q, local = Q.astype(np.float32), local.astype(np.float32)
    return (local, flags, Q) if return_global or R.return_global else (local, flags)


def joint_rotations(poses, skeleton="h36m17", rest="h36m17", primary=None, secondary=None, return_global=False, row_mask=None, out=None):
    """uu3d_joint_rotations on the current stream: ``joint_rotations_host`` on a device tensor, one launch, nothing copies to the host or
    waits (the tables of a ``Rotations`` go up once per device, at its first use).  ``poses``: a contiguous (G, J, 3) float32 device
    tensor, only read -> (local (G, J, 4) float32, flags (G, J) uint8) on the device, with ``return_global`` (local, flags, global).
    ``row_mask``: None or a (G,) uint8 device tensor -- a row whose entry is 0 is not touched; ``out``: None (fresh tensors: the rows a
    mask leaves out are identities with flag 0) or the (local, flags, global or None) tensors to write.  G == 0 launches nothing."""
    import torch
    R = rotations_of(skeleton, rest, primary, secondary)
    if not isinstance(poses, torch.Tensor) or poses.dim() != 3 or poses.shape[2] != 3 or poses.dtype != torch.float32 or not poses.is_contiguous() \
            or not poses.is_cuda:
        raise ValueError(f"poses must be a contiguous (G, J, 3) float32 device tensor, got {tuple(getattr(poses, 'shape', ()))}")
    dev, G, J = poses.device, int(poses.shape[0]), R.skeleton.joints
    if int(poses.shape[1]) != J:
        raise ValueError(f"the skeleton has {J} joints, the poses have {int(poses.shape[1])}")
    want_global = bool(return_global or R.return_global)
    if out is None:
        local = torch.empty((G, J, 4), dtype=torch.float32, device=dev)
        flags = torch.empty((G, J), dtype=torch.uint8, device=dev)
        glob = torch.empty((G, J, 4), dtype=torch.float32, device=dev) if want_global else None
        if row_mask is not None:
            flags.zero_()
            for q in (local, glob):
                if q is not None:
                    q.zero_()
                    q[:, :, 0] = 1.0
    else:
        local, flags, glob = out
    if G:
        tree, rest_dev = R.device_tables(dev)
        lib = _capi.load_library()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _capi.check(lib, lib.uu3d_joint_rotations(_ptr(poses), G, J, _ptr(tree), R.depth, _ptr(rest_dev), _ptr(row_mask), _ptr(local), _ptr(glob),
                                                      _ptr(flags), C.c_void_p(stream)), None)
    return (local, flags, glob) if want_global else (local, flags)


class LiveRotations(object):
    """uu3d_joint_rotations as an output-side stage of a ``StreamSession`` (``smooth.LiveOneEuro``'s interface): no state, the reset writes identities."""

    def __init__(self, slots, joints, rotations, device):
        import torch
        self._lib = _capi.load_library()
        self.slots, self.joints, self.depth = slots, joints, rotations.depth
        self._tables = rotations.device_tables(device)
        self.local = torch.zeros((slots, joints, 4), dtype=torch.float32, device=device)
        self.flags = torch.zeros((slots, joints), dtype=torch.uint8, device=device)
        self.glob = torch.zeros((slots, joints, 4), dtype=torch.float32, device=device) if rotations.return_global else None
        self.outputs = (("extras", "rotations", self.local),) + (() if self.glob is None else (("extras", "global_rotations", self.glob),))
        for _, _, q in self.outputs:
            q[:, :, 0] = 1.0

    def launch(self, active=None, frames=None, drain_state=None):
        tree, rest = self._tables
        return (self._lib.uu3d_joint_rotations, (_ptr(self.read.poses), self.slots, self.joints, _ptr(tree), self.depth, _ptr(rest),
                                                 _ptr(self.read.fresh), _ptr(self.local), _ptr(self.glob), _ptr(self.flags)))

    def reset_launch(self):
        return (self._lib.uu3d_joint_rotations_reset, (self.slots, self.joints, _ptr(self.local), _ptr(self.glob), _ptr(self.flags)))


# ---- host helpers ---------------------------------------------------------------------------------------------------------------------
def quat_to_matrix(q):
    """(..., 4) unit quaternions (w, x, y, z) -> (..., 3, 3) float64 rotation matrices M with v' = M v (numpy, on the host)."""
    q = np.asarray(_host_array(q), np.float64)
    w, x, y, z = (q[..., k] for k in range(4))
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def forward_kinematics(local, rest, lengths, root=None, skeleton="h36m17"):
    """The poses a rig makes of the quaternions (numpy, on the host, float64): ``local`` (G, J, 4) as ``joint_rotations`` gives them,
    ``rest`` as ``Rotations`` takes it (or a ``Rotations``, whose skeleton is then used), ``lengths`` (J,) or (G, J) by child joint,
    ``root`` None (the origin) or (G, 3): the tree root's position -> (G, J, 3):  Q[j] = Q[parent] local[j] and
    x[c] = x[parent] + rotate(Q[parent], rest[c]) lengths[c], from the root outwards."""
    R = rest if isinstance(rest, Rotations) else rotations_of(skeleton, rest)
    sk = R.skeleton
    q = np.asarray(_host_array(local), np.float64)
    G, J = q.shape[0], sk.joints
    if q.shape != (G, J, 4):
        raise ValueError(f"local must be (G, {J}, 4), got {q.shape}")
    L = np.broadcast_to(np.asarray(_host_array(lengths), np.float64), (G, J))
    X, Q = np.zeros((G, J, 3)), np.zeros((G, J, 4))
    if root is not None:
        X[:, sk.root] = np.asarray(_host_array(root), np.float64).reshape(G, 3)
    for j in sk.order:
        p = sk.parents[j]
        if p < 0:
            Q[:, j] = q[:, j]
            continue
        Q[:, j] = _mul(Q[:, p], q[:, j])
        X[:, j] = X[:, p] + _rotate(Q[:, p], R.rest[j]) * L[:, j, None]
    return X
