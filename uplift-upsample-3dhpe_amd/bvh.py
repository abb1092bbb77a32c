"""BVH files from joint rotations: ``write_bvh`` writes the quaternions of ``rotations.joint_rotations`` (``predict_tracks(rotations=...)``,
``StreamSession(rotations=...)``) as a Biovision hierarchy file for Blender, MotionBuilder and the like; ``read_bvh`` reads back what
``write_bvh`` writes, for round-trip tests and sanity checks.  The quaternion -> Euler conversion runs on the host in numpy: this is a
file writer, nothing here is bit-pinned.

    python -m uplift_upsample_3dhpe_amd.bvh --input out.npz --output DIR [--fps F] [--skeleton h36m17] [--lengths FILE.npy]
                                            [--smooth MIN_CUTOFF BETA D_CUTOFF] [--smooth_root MIN_CUTOFF BETA D_CUTOFF]

takes the .npz the predict command writes (per track NAME a (T, J, 3) array of poses, and NAME__root where a camera placed them),
measures each track's bone lengths (``bone_lengths``) unless ``--lengths`` gives them, makes the skeleton rigid (``fix_bones``) and takes
its rotations (``joint_rotations``) on the device, and writes DIR/NAME.bvh per track.  The command is offline by nature, so its filters are
the zero-lag ones (``smooth.OneEuro(..., zero_lag=True)``, ``smooth.one_euro``): ``--smooth`` passes the track's poses through the two-pass
One-Euro filter at ``--fps`` BEFORE bone lengths, the rigid rebuild and the rotations; ``--smooth_root`` does the same for NAME__root, with
NAME__root_state as the filter's state where the file has it.  Without them the files are what they were.

The hierarchy is the tree of the ``Skeleton``: joint j is called ``joint<j>``, its OFFSET is ``rest[j] * lengths[j] * scale`` (the rest
pose's unit direction of the bone above j, at the bone's length; ``scale`` 100: metres -> centimetres), leaves end in an ``End Site``
with a zero offset.  The root has six channels -- its translation (``roots * scale``, zeros without ``roots``) and its rotation --, every
other joint three: Euler angles in degrees in the order ``order`` (default "ZXY": the channels Zrotation Xrotation Yrotation, the
rotation Rz Rx Ry), printed with six decimals."""
import argparse
import os
import re

import numpy as np

from .bones import skeleton_of
from .rotations import Rotations, quat_to_matrix, rotations_of
from .smooth import OneEuro
from .tracks import _host_array

_AXES = "XYZ"
_FILTER = dict(type=float, nargs=3, metavar=("MIN_CUTOFF", "BETA", "D_CUTOFF"), default=None)      # --smooth / --smooth_root


def _check_order(order):
    if not isinstance(order, str) or sorted(order.upper()) != list(_AXES):
        raise ValueError(f'order must be a permutation of "XYZ", got {order!r}')
    return order.upper()


def _axis_matrix(axis, angle):
    """(...,) angles in radians about the coordinate axis ``axis`` (0, 1, 2) -> (..., 3, 3)."""
    c, s = np.cos(angle), np.sin(angle)
    j, k = (axis + 1) % 3, (axis + 2) % 3
    M = np.zeros(np.shape(angle) + (3, 3))
    M[..., axis, axis] = 1.0
    M[..., j, j], M[..., j, k], M[..., k, j], M[..., k, k] = c, -s, s, c
    return M


def euler_to_matrix(angles, order="ZXY"):
    """(..., 3) angles in DEGREES, in the order of the channels -> (..., 3, 3): the product of the three axis rotations in that order."""
    order = _check_order(order)
    a = np.radians(np.asarray(angles, np.float64))
    i, j, k = (_AXES.index(ch) for ch in order)
    return _axis_matrix(i, a[..., 0]) @ _axis_matrix(j, a[..., 1]) @ _axis_matrix(k, a[..., 2])


def matrix_to_euler(M, order="ZXY"):
    """(..., 3, 3) rotation matrices -> (..., 3) angles in DEGREES with ``euler_to_matrix(angles, order) == M``; the middle angle is in
    [-90, 90], and at its ends (gimbal lock) the last angle is 0."""
    order = _check_order(order)
    M = np.asarray(M, np.float64)
    i, j, k = (_AXES.index(ch) for ch in order)
    sign = 1.0 if (i, j, k) in ((0, 1, 2), (1, 2, 0), (2, 0, 1)) else -1.0
    sb = np.clip(sign * M[..., i, k], -1.0, 1.0)
    lock = np.hypot(M[..., k, k], M[..., j, k]) < 1e-9
    first = np.where(lock, np.arctan2(sign * M[..., k, j], M[..., j, j]), np.arctan2(-sign * M[..., j, k], M[..., k, k]))
    last = np.where(lock, 0.0, np.arctan2(-sign * M[..., i, j], M[..., i, i]))
    return np.degrees(np.stack([first, np.arcsin(sb), last], -1))


def write_bvh(path, skeleton, rest, lengths, local, roots=None, fps=50.0, order="ZXY", scale=100.0):
    """One track as a BVH file.  ``skeleton`` / ``rest`` as ``rotations.Rotations`` takes them (or a ``Rotations`` in ``rest``'s place,
    whose skeleton is then used); ``lengths`` (J,) by child joint, in the poses' units; ``local`` (G, J, 4) unit quaternions (w, x, y, z)
    as ``joint_rotations`` gives them, a host array or a tensor; ``roots`` None or (G, 3): the root's translation per frame, in the
    poses' units; ``fps``: the frame rate; ``order``: the Euler order, a permutation of "XYZ"; ``scale``: file units per pose unit."""
    R = rest if isinstance(rest, Rotations) else rotations_of(skeleton, rest)
    sk = R.skeleton
    J = sk.joints
    order = _check_order(order)
    q = np.asarray(_host_array(local), np.float64)
    if q.ndim != 3 or q.shape[1:] != (J, 4):
        raise ValueError(f"local must be (G, {J}, 4), got {q.shape}")
    G = q.shape[0]
    L = np.asarray(_host_array(lengths), np.float64)
    if L.shape != (J,):
        raise ValueError(f"lengths must be ({J},), got {L.shape}")
    if not float(fps) > 0:
        raise ValueError(f"fps must be > 0, got {fps!r}")
    move = np.zeros((G, 3)) if roots is None else np.asarray(_host_array(roots), np.float64).reshape(G, 3) * float(scale)
    offsets = R.rest * np.where(np.arange(J) == sk.root, 0.0, L)[:, None] * float(scale)
    children = [[c for c in range(J) if sk.parents[c] == j] for j in range(J)]
    rot_channels = " ".join(ch + "rotation" for ch in order)
    lines, file_order = ["HIERARCHY"], []

    def joint(j, indent):
        pad = "  " * indent
        file_order.append(j)
        lines.append(f"{pad}{'ROOT' if j == sk.root else 'JOINT'} joint{j}")
        lines.append(pad + "{")
        lines.append(f"{pad}  OFFSET {offsets[j, 0]:.6f} {offsets[j, 1]:.6f} {offsets[j, 2]:.6f}")
        lines.append(f"{pad}  CHANNELS 6 Xposition Yposition Zposition {rot_channels}" if j == sk.root else f"{pad}  CHANNELS 3 {rot_channels}")
        for c in children[j]:
            joint(c, indent + 1)
        if not children[j]:
            lines.extend([pad + "  End Site", pad + "  {", pad + "    OFFSET 0.000000 0.000000 0.000000", pad + "  }"])
        lines.append(pad + "}")

    joint(sk.root, 0)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)                # (float32 quaternions are unit to 2^-24 only: an orthogonal matrix)
    angles = matrix_to_euler(quat_to_matrix(q), order)[:, file_order]
    angles = np.where(angles == 0.0, 0.0, angles)                    # (no "-0.000000")
    lines += ["MOTION", f"Frames: {G}", f"Frame Time: {1.0 / float(fps):.9f}"]
    values = np.concatenate([move, angles.reshape(G, -1)], 1)
    lines += [" ".join(f"{v:.6f}" for v in row) for row in values]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


def read_bvh(path):
    """What ``write_bvh`` wrote -> a dict: ``names`` (J,), ``parents`` (J,) ints (-1: the root), ``offsets`` (J, 3), ``end_sites`` {joint:
    (3,) offset}, ``order`` the Euler order, ``frames``, ``frame_time``, ``translations`` (frames, 3), ``angles`` (frames, J, 3) degrees in
    channel order and ``text``, the file.  Joints called ``joint<j>`` come back at index j, others in file order."""
    text = open(path).read()
    tokens = text.split()
    names, parents, offsets, channels, end_sites, stack = [], [], [], [], {}, []
    at, in_end = 0, False
    if not tokens or tokens[0] != "HIERARCHY":
        raise ValueError(f"{path}: not a BVH file (no HIERARCHY)")
    at = 1
    while tokens[at] != "MOTION":
        t = tokens[at]
        if t in ("ROOT", "JOINT"):
            names.append(tokens[at + 1])
            parents.append(stack[-1] if stack else -1)
            offsets.append(None)
            channels.append([])
            stack.append(len(names) - 1)
            at += 2
        elif t == "End":
            in_end = True
            stack.append(stack[-1])
            at += 2
        elif t == "OFFSET":
            v = np.array([float(x) for x in tokens[at + 1:at + 4]])
            if in_end:
                end_sites[stack[-1]] = v
            else:
                offsets[stack[-1]] = v
            at += 4
        elif t == "CHANNELS":
            n = int(tokens[at + 1])
            channels[stack[-1]] = tokens[at + 2:at + 2 + n]
            at += 2 + n
        elif t == "}":
            stack.pop()
            in_end = False
            at += 1
        else:                                                         # "{"
            at += 1
    J = len(names)
    orders = {"".join(ch[0] for ch in c if ch.endswith("rotation")) for c in channels}
    if len(orders) != 1:
        raise ValueError(f"{path}: the joints do not share one Euler order: {sorted(orders)}")
    frames, frame_time = int(tokens[at + 2]), float(tokens[at + 5])
    values = np.array([float(x) for x in tokens[at + 6:]], np.float64).reshape(frames, -1)
    translations, angles, col = np.zeros((frames, 3)), np.zeros((frames, J, 3)), 0
    for j, c in enumerate(channels):
        for ch in c:
            if ch.endswith("position"):
                translations[:, _AXES.index(ch[0])] = values[:, col]
            col += 1
        angles[:, j] = values[:, col - 3:col]
    own = [re.fullmatch(r"joint(\d+)", n) for n in names]
    place = [int(m.group(1)) for m in own] if all(own) and sorted(int(m.group(1)) for m in own) == list(range(J)) else list(range(J))
    inverse = np.argsort(place)
    return {"names": [names[i] for i in inverse], "parents": [-1 if parents[i] < 0 else place[parents[i]] for i in inverse],
            "offsets": np.array(offsets)[inverse], "end_sites": {place[j]: v for j, v in end_sites.items()}, "order": orders.pop(),
            "frames": frames, "frame_time": frame_time, "translations": translations, "angles": angles[:, inverse], "text": text}


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m uplift_upsample_3dhpe_amd.bvh", description="Write one .bvh file per track of the .npz the predict "
                                "command wrote: bone lengths, rigid skeleton and joint rotations are computed on the device.")
    p.add_argument("--input", required=True, help=".npz with one (T, J, 3) array per track (and NAME__root where a camera placed it)")
    p.add_argument("--output", required=True, help="directory to write NAME.bvh into")
    p.add_argument("--fps", type=float, default=50.0, help="frame rate of the poses (default 50)")
    p.add_argument("--skeleton", default="h36m17", help="name of the skeleton and its rest pose (default h36m17)")
    p.add_argument("--lengths", default=None, help=".npy with (J,) bone lengths by child joint (default: measured per track)")
    p.add_argument("--smooth", **_FILTER, help="pass the poses through a zero-lag (two-pass) One-Euro filter (Hz, 1 / unit speed, Hz) at --fps, "
                                               "before bone lengths and rotations")
    p.add_argument("--smooth_root", **_FILTER, help="the same for NAME__root (NAME__root_state, where the file has it, says which rows are roots)")
    args = p.parse_args(argv)
    try:
        args.pose_filter, args.root_filter = (None if v is None else OneEuro(*v, zero_lag=True) for v in (args.smooth, args.smooth_root))
    except ValueError as e:
        raise SystemExit(f"--smooth / --smooth_root: {e}") from None
    return args


def main(argv=None):
    import torch

    from .bones import bone_lengths, fix_bones
    from .rotations import joint_rotations
    from .smooth import one_euro
    args = parse_args(argv)
    R = Rotations(args.skeleton, skeleton_of(args.skeleton))
    data = np.load(args.input)
    names = [k for k in data.files if "__" not in k]
    given = None if args.lengths is None else np.load(args.lengths).astype(np.float64)
    os.makedirs(args.output, exist_ok=True)
    for name in names:
        poses = torch.from_numpy(np.ascontiguousarray(data[name], np.float32)).to("cuda:0")
        if args.pose_filter is not None:
            poses = one_euro(poses, None, args.fps, args.pose_filter)
        lengths = bone_lengths(poses, None, R.skeleton) if given is None else given
        local = joint_rotations(fix_bones(poses, None, lengths, R.skeleton), R)[0]
        L = (lengths[0].cpu().numpy() if given is None else given).copy()
        L[~np.isfinite(L)] = 0.0
        roots = data[name + "__root"] if name + "__root" in data.files else None
        if roots is not None and args.root_filter is not None:
            state = data[name + "__root_state"] if name + "__root_state" in data.files else None
            roots = one_euro(torch.from_numpy(np.ascontiguousarray(roots, np.float32).reshape(-1, 3)).to("cuda:0"), None, args.fps, args.root_filter,
                             None if state is None else torch.from_numpy(np.ascontiguousarray(state != 0).reshape(-1)).to("cuda:0"))
        path = write_bvh(os.path.join(args.output, name + ".bvh"), R.skeleton, R, L, local, roots, fps=args.fps)
        print(f"wrote {path}: {int(poses.shape[0])} frames", flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
