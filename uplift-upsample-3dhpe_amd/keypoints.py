"""The keypoint stage of the track pipeline: a detector's joint layout mapped onto the model's joints, in front of everything else.
Wraps uu3d_keypoint_map_bytes / uu3d_keypoint_map_pack (``KeypointMap.packed``) and uu3d_map_keypoints (``map_keypoints``; the rule in
numpy: ``map_keypoints_host``).

Any skeleton: ``predict_tracks(..., keypoints="coco17")`` takes tracks in the DETECTOR's joint layout, (T_i, K_in, 2), and maps them onto the
model's joints on the device before anything else looks at them (uu3d_map_keypoints; ``KeypointMap``, ``KEYPOINT_PRESETS``; the rule in
numpy: ``map_keypoints_host``); per-joint flags and scores are then per detector joint.

Any skeleton -- ``StreamSession(..., keypoints=M)`` (a name of ``predict.KEYPOINT_PRESETS`` or a ``predict.KeypointMap``): ``push`` takes
frames in the DETECTOR's joint layout, (slots, K_in, 2), and one more launch in front of the stage (uu3d_map_keypoints) writes the session's
own (slots, J, 2) frame -- with ``repair_joints`` its (slots, J) joint flags as well, from (slots, K_in) flags per detector joint.  In a
session without ``fps`` that launch is the first step of the ONE captured tick graph; with ``fps`` it sits in front of
uu3d_stream_source_push, not captured, like the launches around it.  ``captures`` stays 1 and ``push`` still never waits.  The session's
contract is its usual one with the mapped track: the same session without ``keypoints``, pushed ``predict.map_keypoints_host``'s frames and
flags, returns the same bits.  ``keypoints=None`` is the session above, bit for bit."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import ptr as _ptr
from .tracks import _host_array, _shape, _upload
from .validity import _device_joint_flags, check_valid


MAX_KEYPOINT_SOURCES = 8                                              # sources per model joint: the fixed stride of the device table


class KeypointMap(object):
    """An affine map from a detector's joints onto the model's (include/uu3d.h, ANY SKELETON): ``inputs`` = K_in joints come in; model joint
    j is ``sum_k weights[j][k] * in[sources[j][k]]``, summed in the listed order.  ``sources``: per model joint 1 to 8 distinct indices in
    [0, inputs); ``weights``: as many float64 weights each, finite, non-zero, summing to 1 within 1e-12 (negative ones allowed: the map is
    affine, so it commutes, mathematically, with the screen normalisation).  Anything else is a ValueError.  ``joints`` = J = len(sources).
    Immutable; the packed table is made once and uploaded once per device (``device_table``)."""

    def __init__(self, inputs, sources, weights):
        if isinstance(inputs, bool) or not isinstance(inputs, (int, np.integer)) or int(inputs) < 1:
            raise ValueError(f"inputs must be an int >= 1: the joints the detector emits, got {inputs!r}")
        sources, weights = list(sources), list(weights)
        if len(sources) < 1 or len(sources) != len(weights):
            raise ValueError(f"sources and weights need one entry per model joint, got {len(sources)} and {len(weights)}")
        self.inputs, self.joints = int(inputs), len(sources)
        src, wts = [], []
        for j, (s, w) in enumerate(zip(sources, weights)):
            s, w = [int(i) for i in np.asarray(s).reshape(-1)], [float(x) for x in np.asarray(w, np.float64).reshape(-1)]
            if not 1 <= len(s) <= MAX_KEYPOINT_SOURCES or len(s) != len(w):
                raise ValueError(f"model joint {j} needs 1 to {MAX_KEYPOINT_SOURCES} sources and as many weights, got {len(s)} and {len(w)}")
            if len(set(s)) != len(s) or min(s) < 0 or max(s) >= self.inputs:
                raise ValueError(f"model joint {j}: sources must be distinct indices in [0, {self.inputs}), got {s}")
            if not all(np.isfinite(x) and x != 0.0 for x in w):
                raise ValueError(f"model joint {j}: weights must be finite and non-zero, got {w}")
            total = 0.0
            for x in w:
                total = total + x
            if not abs(total - 1.0) <= 1e-12:
                raise ValueError(f"model joint {j}: weights must sum to 1 (an affine map), they sum to {total!r}")
            src.append(tuple(s))
            wts.append(tuple(w))
        self.sources, self.weights = tuple(src), tuple(wts)
        self._packed, self._tables = None, {}

    def planes(self):
        """-> (counts (J,) int32, sources (J, 8) int32 with -1 behind a joint's last source, weights (J, 8) float64 with 0 there)."""
        counts = np.array([len(s) for s in self.sources], np.int32)
        src = np.full((self.joints, MAX_KEYPOINT_SOURCES), -1, np.int32)
        w = np.zeros((self.joints, MAX_KEYPOINT_SOURCES), np.float64)
        for j, (s, x) in enumerate(zip(self.sources, self.weights)):
            src[j, :len(s)], w[j, :len(s)] = s, x
        return counts, src, w

    def packed(self):
        """The table of uu3d_keypoint_map_pack as a host uint8 array (the library checks the map once more, the index range included)."""
        if self._packed is None:
            lib = _capi.load_library()
            nbytes = int(lib.uu3d_keypoint_map_bytes(self.inputs, self.joints))
            if nbytes == 0:
                raise ValueError(f"a map from {self.inputs} onto {self.joints} joints is out of uu3d_keypoint_map_pack's range")
            counts, src, w = self.planes()
            out = np.zeros(nbytes // 8, np.float64)                   # (8-byte aligned)
            _capi.check(lib, lib.uu3d_keypoint_map_pack(self.inputs, self.joints, counts.ctypes.data, src.ctypes.data, w.ctypes.data,
                                                        out.ctypes.data, nbytes), None)
            self._packed = out.view(np.uint8)
        return self._packed

    def device_table(self, device):
        """The packed table on ``device``: uploaded at the first call, which waits for the copy once -- whatever stream uses it later finds
        it there --, and kept for the life of the map: no call does host work per frame."""
        import torch
        key = str(torch.device(device))
        if key not in self._tables:
            self._tables[key] = _upload(self.packed(), np.uint8, device)
            torch.cuda.current_stream(device).synchronize()
        return self._tables[key]

    def __repr__(self):
        return f"KeypointMap(inputs={self.inputs}, joints={self.joints})"


def _h36m17_from(inputs, r_leg, l_leg, r_arm, l_arm, pelvis, neck, torso, head, head_top):
    """A ``KeypointMap`` onto ``H36MOrder17P``: 0-2 right ankle, knee, hip; 3-5 left hip, knee, ankle; 6 pelvis; 7 neck; 8 torso; 9 head;
    10 head top; 11-13 right wrist, elbow, shoulder; 14-16 left shoulder, elbow, wrist.  Limbs are (ankle, knee, hip) / (wrist, elbow,
    shoulder) source indices; the other five are (sources, weights)."""
    one = lambda i: ((i,), (1.0,))
    rows = [one(r_leg[0]), one(r_leg[1]), one(r_leg[2]), one(l_leg[2]), one(l_leg[1]), one(l_leg[0]), pelvis, neck, torso, head, head_top,
            one(r_arm[0]), one(r_arm[1]), one(r_arm[2]), one(l_arm[2]), one(l_arm[1]), one(l_arm[0])]
    return KeypointMap(inputs, [r[0] for r in rows], [r[1] for r in rows])


# Named maps onto H36MOrder17P (J = 17), the layout of the shipped configs.  They are GEOMETRIC APPROXIMATIONS of joints the detector does
# not emit (a pelvis between the hips, a head top beyond the eyes): the shipped weights were trained on Human3.6M 2D detections and no
# accuracy figure is claimed for these tables -- the mechanism is the feature, the tables are a convenience.
# Left-right consistency: mirroring the input (x negated, joints permuted by the detector's own left-right order) and then mapping gives the
# bits of mapping and then mirroring by AUGM_FLIP_KEYPOINT_ORDER.  The sources are ORDERED for that: a mirrored pair comes first, left then
# right (its sum, the first one of the expression, is the same either way round: a + b == b + a), unpaired sources behind it -- the nose
# last in head_top.  The torso of "coco17" sums two pairs; mirrored, the hips arrive in the other order behind the shoulders' sum, which
# gives the same bits wherever the float64 partial sums are exact -- four float32 coordinates within a factor of 2^26 of each other, or
# zero -- and elsewhere the same value up to one float64 rounding, which reaches the float32 result about once in 2^29 times.
KEYPOINT_PRESETS = {
    # COCO-17: 0 nose, 1 l_eye, 2 r_eye, 3 l_ear, 4 r_ear, 5 l_sho, 6 r_sho, 7 l_elb, 8 r_elb, 9 l_wri, 10 r_wri, 11 l_hip, 12 r_hip,
    # 13 l_knee, 14 r_knee, 15 l_ank, 16 r_ank
    "coco17": _h36m17_from(17, r_leg=(16, 14, 12), l_leg=(15, 13, 11), r_arm=(10, 8, 6), l_arm=(9, 7, 5),
                           pelvis=((11, 12), (0.5, 0.5)), neck=((5, 6), (0.5, 0.5)), torso=((5, 6, 11, 12), (0.25, 0.25, 0.25, 0.25)),
                           head=((0,), (1.0,)), head_top=((1, 2, 0), (1.0, 1.0, -1.0))),
    # OpenPose BODY_25: 0 Nose, 1 Neck, 2 RShoulder, 3 RElbow, 4 RWrist, 5 LShoulder, 6 LElbow, 7 LWrist, 8 MidHip, 9 RHip, 10 RKnee,
    # 11 RAnkle, 12 LHip, 13 LKnee, 14 LAnkle, 15 REye, 16 LEye, 17 REar, 18 LEar, 19 LBigToe, 20 LSmallToe, 21 LHeel, 22 RBigToe,
    # 23 RSmallToe, 24 RHeel
    "body25": _h36m17_from(25, r_leg=(11, 10, 9), l_leg=(14, 13, 12), r_arm=(4, 3, 2), l_arm=(7, 6, 5),
                           pelvis=((8,), (1.0,)), neck=((1,), (1.0,)), torso=((1, 8), (0.5, 0.5)),
                           head=((0,), (1.0,)), head_top=((16, 15, 0), (1.0, 1.0, -1.0))),
}


def keypoint_map(name_or_map, J=None):
    """``predict_tracks``' ``keypoints`` argument -> a ``KeypointMap``: a name of ``KEYPOINT_PRESETS`` or a map of your own.  ``J``: the
    model's joint count; a map onto another number of joints is a ValueError (the presets target 17)."""
    if isinstance(name_or_map, KeypointMap):
        M, what = name_or_map, repr(name_or_map)
    elif isinstance(name_or_map, str):
        if name_or_map not in KEYPOINT_PRESETS:
            raise ValueError(f"keypoints must be a KeypointMap or one of {sorted(KEYPOINT_PRESETS)}, got {name_or_map!r}")
        M, what = KEYPOINT_PRESETS[name_or_map], repr(name_or_map)
    else:
        raise ValueError(f"keypoints must be a KeypointMap or one of {sorted(KEYPOINT_PRESETS)}, got {name_or_map!r}")
    if J is not None and M.joints != int(J):
        raise ValueError(f"keypoints={what} maps onto {M.joints} joints, the model has {int(J)}")
    return M


def check_keypoint_inputs(M, counts, what="track"):
    """Every track (slot, array) has the K_in joints ``M`` takes: ValueError naming both numbers otherwise."""
    for i, k in enumerate(counts):
        if int(k) != M.inputs:
            raise ValueError(f"{what} {i} has {int(k)} keypoints, keypoints={M!r} takes {M.inputs}")


def map_keypoints_host(M, tracks, valid=None):
    """The rule of ``predict_tracks(keypoints=M)`` (include/uu3d.h, ANY SKELETON) in numpy, written to be read: what uu3d_map_keypoints
    computes, bit for bit.  ``tracks``: list of (T_i, K_in, 2) arrays; ``valid``: None, "finite" or a list with one (T_i,) or (T_i, K_in)
    entry per track -> (mapped, flags): per track (T_i, J, 2) float32, and ``flags`` as the call behind the map takes them --
        None            -> None: the expression alone, a NaN source gives a NaN joint;
        (T_i, K_in)     -> (T_i, J) bool: a source is observed when its flag is non-zero and both coordinates are finite, a model joint iff
                           every one of its sources is; an unobserved joint's coordinates are zeros ("finite": every flag set);
        (T_i,)          -> the entry itself, unchanged: frame flags pass through, the coordinates are the expression.
    So ``predict_tracks(model, cfg, tracks, keypoints=M, valid=V, **kw)`` equals ``predict_tracks(model, cfg, mapped, valid=flags, **kw)``."""
    M = keypoint_map(M)
    tracks = [np.asarray(_host_array(t), np.float32) for t in tracks]
    check_keypoint_inputs(M, [t.shape[1] for t in tracks])
    if valid is not None and not isinstance(valid, str):
        check_valid(valid, [len(t) for t in tracks], joints=M.inputs)
    elif valid is not None and valid != "finite":
        raise ValueError('valid must be None, "finite" or a list with one entry per track')
    mapped, flags = [], None if valid is None else []
    for i, src in enumerate(tracks):
        T = len(src)
        v = None if valid is None else np.ones((T, M.inputs), bool) if isinstance(valid, str) else _host_array(valid[i]) != 0
        per_joint = v is not None and v.ndim == 2
        if per_joint:
            observed = v & np.isfinite(src).all(axis=2)
        out = np.zeros((T, M.joints, 2), np.float32)
        joint_flags = np.zeros((T, M.joints), bool)
        for j, (sources, weights) in enumerate(zip(M.sources, M.weights)):
            with np.errstate(invalid="ignore", over="ignore"):
                acc = np.float64(weights[0]) * src[:, sources[0]].astype(np.float64)
                for s, w in zip(sources[1:], weights[1:]):
                    acc = acc + np.float64(w) * src[:, s].astype(np.float64)
                r = acc.astype(np.float32)
            r[np.isnan(r)] = np.float32(np.nan)                       # THE quiet NaN 0x7fc00000, as the device stores it
            if per_joint:
                joint_flags[:, j] = observed[:, list(sources)].all(axis=1)
                r[~joint_flags[:, j]] = 0.0
            out[:, j] = r
        mapped.append(out)
        if flags is not None:
            flags.append(joint_flags if per_joint else valid[i])
    return mapped, flags


def map_keypoints(src, flags, M, model):
    """uu3d_map_keypoints on the current stream.  ``src`` (F, K_in, 2) float32 on the device, contiguous (only read); ``flags`` (F, K_in)
    uint8 on the device or None; ``M``: a ``KeypointMap`` onto the joints of ``model`` (its handle says J) -> (mapped (F, J, 2) float32,
    joint flags (F, J) uint8 or None), fresh device buffers."""
    import torch
    lib = _capi.load_library()
    dev = src.device
    F, J = int(src.shape[0]), M.joints
    if src.dtype != torch.float32 or not src.is_contiguous() or tuple(src.shape) != (F, M.inputs, 2):
        raise ValueError(f"src must be a contiguous (F, {M.inputs}, 2) float32 device tensor, got {tuple(src.shape)}")
    if flags is not None and (flags.dtype != torch.uint8 or not flags.is_contiguous() or tuple(flags.shape) != (F, M.inputs)):
        raise ValueError(f"flags must be a contiguous ({F}, {M.inputs}) uint8 device tensor")
    if int(model.arch.num_keypoints) != J:
        raise ValueError(f"keypoints={M!r} maps onto {J} joints, the model has {int(model.arch.num_keypoints)}")
    table = M.device_table(dev)
    out = torch.empty((F, J, 2), dtype=torch.float32, device=dev)
    flags_out = None if flags is None else torch.empty((F, J), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(lib, lib.uu3d_map_keypoints(model._h, _ptr(table), M.inputs, _ptr(src), _ptr(flags), F, _ptr(out), _ptr(flags_out),
                                                C.c_void_p(stream)), model._h)
    return out, flags_out


def _map_front(M, model, src, given, valid):
    """The map in front of everything else: the given frames of all tracks (R, K_in, 2) and ``valid`` per detector joint -> (the frames
    (R, J, 2), ``valid`` per model joint, as ``_front_validity`` takes it).  One launch; a list that mixes (T_i, K_in) and (T_i,) entries
    takes one launch with and one without flags, and every track the rows of its own kind."""
    import torch
    if model is None:
        raise ValueError("keypoints needs the model: its handle says which joints the map must give")
    K, dev, sizes = M.inputs, src.device, [int(n) for n in given]
    if valid is None:
        return map_keypoints(src, None, M, model)[0], None
    if isinstance(valid, str):                                        # "finite": the finite test per SOURCE joint, every flag set
        out, flags = map_keypoints(src, torch.ones((int(src.shape[0]), K), dtype=torch.uint8, device=dev), M, model)
        return out, list(torch.split(flags, sizes, 0))
    per_joint = [len(_shape(v)) == 2 for v in valid]
    if not any(per_joint):                                            # frame flags pass through unchanged
        return map_keypoints(src, None, M, model)[0], valid
    out, flags = map_keypoints(src, _device_joint_flags(valid, K, dev), M, model)
    flags = list(torch.split(flags, sizes, 0))
    if all(per_joint):
        return out, flags
    plain = torch.split(map_keypoints(src, None, M, model)[0], sizes, 0)
    out = torch.cat([a if p else b for p, a, b in zip(per_joint, torch.split(out, sizes, 0), plain)], 0)
    return out, [f if p else v for p, f, v in zip(per_joint, flags, valid)]
