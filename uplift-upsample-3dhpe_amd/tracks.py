"""The table stage of the track pipeline: the tracks' 2D keypoints become the dense, normalised ``data.PoseTable`` the windows are cut from,
and the network's raw predictions become one pose per returned frame.  Wraps uu3d_normalize_tracks / uu3d_normalize_tracks_valid
(``normalize_tracks``), uu3d_resample_tracks (``resample_tracks``), uu3d_assemble_tracks (``assemble_tracks``) and
uu3d_assemble_tracks_cubic (``assemble_tracks_cubic``: ``interpolation="cubic"``); ``pose_table`` and ``resampled_pose_table`` put the validity and keypoint stages in front of the first two.  Also the small helpers every stage uploads and
checks shapes with (``_upload``: pinned, asynchronous, never waits)."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import ptr as _ptr
from .data import PoseTable
from .rates import resample_plan


def _upload(a, dtype, device):
    """Host array -> device tensor through pinned memory, asynchronously: the host never waits for the stream."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).pin_memory().to(device, non_blocking=True)


def _host_array(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _shape(a):
    return tuple(a.shape) if hasattr(a, "shape") else np.asarray(a).shape


def _device_track(t, device):
    import torch
    if isinstance(t, torch.Tensor):
        t = t.to(device=device, dtype=torch.float32)
    else:
        t = _upload(np.asarray(t), np.float32, device)
    if t.dim() != 3 or t.shape[2] != 2:
        raise ValueError(f"a track must be (T, J, 2), got {tuple(t.shape)}")
    return t


def _device_tracks(tracks, device):
    """The tracks on the device -> (list of (T_i, J, 2) tensors, J, frames given per track)."""
    tr = [_device_track(t, device) for t in tracks]
    if not tr:
        raise ValueError("no tracks")
    J = int(tr[0].shape[1])
    if any(int(t.shape[1]) != J for t in tr):
        raise ValueError("all tracks must have the same number of keypoints")
    return tr, J, np.array([int(t.shape[0]) for t in tr], np.int64)


def keyframe_count(length, stride):
    """Frames 0, stride, 2 stride, ... of a track of ``length`` frames."""
    return (int(length) + int(stride) - 1) // int(stride)


def check_resolutions(resolutions, count, per="track"):
    """None, one (w, h) or one per track (per slot, for a session) -> None or (count, 2) float64, contiguous."""
    if resolutions is None:
        return None
    r = np.asarray(resolutions, np.float64)
    if r.shape == (2,):
        r = np.tile(r, (count, 1))
    if r.shape != (count, 2) or not np.isfinite(r).all() or not (r > 0).all():
        raise ValueError(f"resolutions must be one positive (w, h) or one per {per}")
    return np.ascontiguousarray(r)


def normalize_tracks(src, table, lens, resolutions=None, key_stride=0, src_lens=None, valid_in=None, valid_out=None):
    """uu3d_normalize_tracks on the current stream.  ``src`` (R, J, 2) float32 on the device; ``table`` (sum(lens), J, 2) float32 (may be
    ``src`` when ``key_stride`` is 0); ``lens``: frames per track; ``resolutions`` (T, 2) (w, h) per track or None (no conversion);
    ``key_stride`` > 0: ``src`` holds ``src_lens[t]`` keyframes of track t (frames 0, key_stride, ...), scattered into the zero-filled table.
    ``valid_out`` (sum(lens),) uint8 on the device: uu3d_normalize_tracks_valid -- it receives the per-frame flags (``valid_in`` (R,) uint8 or
    None AND all coordinates finite) and the table rows of missing frames are zeros."""
    import torch
    lib = _capi.load_library()
    dev = table.device
    lens = np.asarray(lens, np.int64)
    T, rows, J = len(lens), int(lens.sum()), int(table.shape[1])
    row_track = _upload(np.repeat(np.arange(T, dtype=np.int32), lens), np.int32, dev)
    res = None if resolutions is None else _upload(np.asarray(resolutions, np.float64).reshape(T, 2), np.float64, dev)
    tstart = sstart = None
    if key_stride > 0:
        src_lens = np.asarray(src_lens, np.int64)
        tstart = _upload(np.concatenate([[0], np.cumsum(lens)[:-1]]), np.int64, dev)
        sstart = _upload(np.concatenate([[0], np.cumsum(src_lens)[:-1]]), np.int64, dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        if valid_out is None:
            _capi.check(lib, lib.uu3d_normalize_tracks(_ptr(src), int(src.shape[0]), _ptr(table), rows, J, _ptr(row_track), T, _ptr(res),
                                                       _ptr(tstart), _ptr(sstart), int(key_stride), C.c_void_p(stream)), None)
        else:
            _capi.check(lib, lib.uu3d_normalize_tracks_valid(_ptr(src), int(src.shape[0]), _ptr(table), rows, J, _ptr(row_track), T, _ptr(res),
                                                             _ptr(tstart), _ptr(sstart), int(key_stride), _ptr(valid_in), _ptr(valid_out),
                                                             C.c_void_p(stream)), None)
    return table


def resample_tracks(src, table, model_lens, left, right, weight, resolutions=None, valid_in=None, valid_out=None):
    """uu3d_resample_tracks on the current stream.  ``src`` (R, J, 2) float32 on the device; ``table`` (sum(model_lens), J, 2) float32, never
    ``src``; ``left`` / ``right`` / ``weight``: the plan of ``resample_plan`` (host arrays); ``resolutions`` (T, 2) (w, h) per track or None
    (no conversion).  ``valid_out`` (sum(model_lens),) uint8 on the device receives the per-model-frame flags (``valid_in`` (R,) uint8 or
    None, ANDed with all coordinates finite, of the left source frame and, where weight > 0, the right one) and the table rows of missing
    frames are zeros."""
    import torch
    lib = _capi.load_library()
    dev = table.device
    model_lens = np.asarray(model_lens, np.int64)
    T, rows, J = len(model_lens), int(model_lens.sum()), int(table.shape[1])
    if not (len(left) == len(right) == len(weight) == rows == int(table.shape[0])):
        raise ValueError("the plan must have one entry per table row")
    row_track = _upload(np.repeat(np.arange(T, dtype=np.int32), model_lens), np.int32, dev)
    res = None if resolutions is None else _upload(np.asarray(resolutions, np.float64).reshape(T, 2), np.float64, dev)
    d_left, d_right, d_weight = _upload(left, np.int64, dev), _upload(right, np.int64, dev), _upload(weight, np.float64, dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(lib, lib.uu3d_resample_tracks(_ptr(src), int(src.shape[0]), _ptr(table), rows, J, _ptr(row_track), T, _ptr(res), _ptr(d_left),
                                                  _ptr(d_right), _ptr(d_weight), _ptr(valid_in), _ptr(valid_out), C.c_void_p(stream)), None)
    return table


def _check_predictions(plain, flipped, flip_order):
    """The raw predictions as the two assemble launches take them -> (W, J)."""
    import torch
    if plain.dtype != torch.float32 or not plain.is_contiguous() or plain.dim() != 3 or plain.shape[2] != 3:
        raise ValueError("plain must be a contiguous (W, J, 3) float32 device tensor")
    J = int(plain.shape[1])
    if flipped is not None and (flipped.shape != plain.shape or flipped.dtype != torch.float32 or not flipped.is_contiguous()):
        raise ValueError("flipped must match plain")
    if flipped is not None and (flip_order is None or len(flip_order) != J):
        raise ValueError("flipped predictions need the J entries of AUGM_FLIP_KEYPOINT_ORDER")
    return int(plain.shape[0]), J


def assemble_tracks(plain, flipped, left, right, weight, flip_order=None, root=-1):
    """uu3d_assemble_tracks on the current stream.  ``plain`` / ``flipped`` (W, J, 3) float32 on the device (``flipped`` None: no flip);
    ``left`` / ``right`` / ``weight``: the plan of ``evaluation.keyframe_plan`` with rows of those arrays (host arrays of F entries);
    ``root`` >= 0: that joint is subtracted.  -> (F, J, 3) float32 on the device."""
    import torch
    lib = _capi.load_library()
    dev = plain.device
    F = len(left)
    W, J = _check_predictions(plain, flipped, flip_order)
    d_left, d_right = _upload(left, np.int32, dev), _upload(right, np.int32, dev)
    d_weight = _upload(weight, np.float64, dev)
    d_order = None if flipped is None else _upload(flip_order, np.int32, dev)
    out = torch.empty((F, J, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(lib, lib.uu3d_assemble_tracks(_ptr(plain), _ptr(flipped), W, _ptr(d_order), _ptr(d_left), _ptr(d_right), _ptr(d_weight),
                                                  F, J, int(root), _ptr(out), C.c_void_p(stream)), None)
    return out


def assemble_tracks_cubic(plain, flipped, before, left, right, after, weight, flip_order=None, root=-1):
    """uu3d_assemble_tracks_cubic on the current stream: ``assemble_tracks`` with the plan of ``evaluation.keyframe_plan_cubic`` /
    ``keyframe_plan_cubic_at`` -- ``before`` / ``after``: the predicted frame in front of ``left`` and the one behind ``right``, -1: none
    (host arrays of F entries each) -- and a C1 cubic between the predicted frames (``evaluation.interpolate_cubic_host`` is the rule in
    numpy, and the result equals it bit for bit).  -> (F, J, 3) float32 on the device."""
    import torch
    lib = _capi.load_library()
    dev = plain.device
    F = len(left)
    W, J = _check_predictions(plain, flipped, flip_order)
    if not (len(before) == len(right) == len(after) == len(weight) == F):
        raise ValueError("the plan must have one entry per frame in each of its five arrays")
    d_plan = [_upload(a, np.int32, dev) for a in (before, left, right, after)]
    d_weight = _upload(weight, np.float64, dev)
    d_order = None if flipped is None else _upload(flip_order, np.int32, dev)
    out = torch.empty((F, J, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(lib, lib.uu3d_assemble_tracks_cubic(_ptr(plain), _ptr(flipped), W, _ptr(d_order), *(_ptr(a) for a in d_plan), _ptr(d_weight),
                                                        F, J, int(root), _ptr(out), C.c_void_p(stream)), None)
    return out


def _table_front(tracks, device, resolutions, valid, repair_joints, keypoints, model, keep_source, frames, write, distortion=None):
    """What ``pose_table`` and ``resampled_pose_table`` share, in the order of the launches: the tracks on the device, the checks of
    ``valid`` / ``repair_joints`` / ``keypoints`` / ``resolutions``, the given frames back to back, with ``distortion`` -- the (tracks, 10)
    rows of a ``camera.Camera`` with distortion per track -- uu3d_undistort_points on them in the detector's layout (a fresh buffer: the
    caller's memory is never written; everything behind reads the undistorted points), uu3d_map_keypoints (``_map_front``),
    ``table.source`` for the root solve, uu3d_repair_joints and the ``valid_in`` flags (``_front_validity``), then the entry's own front
    kernel and the ``data.PoseTable``.  ``frames(given)`` -> the frames per track the given ones stand for (every track needs one);
    ``write(src, J, given, lens, resolutions, valid_in)`` -> (the table's rows (R', J, 2), their (R',) uint8 flags or None, rows per track).
    -> (table, rows per track, frames given per track)."""
    import torch
    from .keypoints import _map_front, check_keypoint_inputs, keypoint_map            # (here: both stages build on this module's helpers)
    from .validity import _front_validity, _source_joint_flags, check_repair_joints, check_valid
    check_repair_joints(repair_joints, valid)
    tr, J, given = _device_tracks(tracks, device)
    if keypoints is not None:
        keypoints = keypoint_map(keypoints)
        check_keypoint_inputs(keypoints, [J])
    check_valid(valid, given, joints=J)
    lens = frames(given)
    if (lens < 1).any():
        raise ValueError("every track needs at least one frame")
    resolutions = check_resolutions(resolutions, len(tr))
    src = torch.cat(tr, 0).contiguous() if len(tr) > 1 else tr[0].contiguous()
    if distortion is not None:
        from .camera import undistort_rows
        src = undistort_rows(src, distortion, given)
    if keypoints is not None:
        (src, valid), J = _map_front(keypoints, model, src, given, valid), keypoints.joints
    source = (src, _source_joint_flags(valid, J, src.device)) if keep_source else None
    src, valid_in, state = _front_validity(src, given, J, valid, repair_joints, None if source is None else source[1])
    kp, flags, lens = write(src, J, given, lens, resolutions, valid_in)
    table = PoseTable.from_device(kp, lens, valid=flags)
    table.joint_state, table.source = state, source
    return table, lens, given


def pose_table(tracks, device, resolutions=None, key_stride=0, lengths=None, valid=None, repair_joints=None, keypoints=None, model=None,
               keep_source=False, distortion=None):
    """The dense, normalised ``data.PoseTable`` of the tracks (uu3d_normalize_tracks) -> (table, frames per track).  ``valid`` as in
    ``predict_tracks`` (not None: uu3d_normalize_tracks_valid into a fresh buffer; the table carries the per-frame flags).
    ``repair_joints`` = G: uu3d_repair_joints runs on the given frames first; ``table.joint_state`` is its (given frames, J) uint8 state.
    ``keypoints``: a ``KeypointMap`` or a preset's name (with ``model``): the tracks are (T_i, K_in, 2), per-joint entries of ``valid``
    (T_i, K_in), and uu3d_map_keypoints runs in front of all of that (``_map_front``).  ``keep_source``: ``table.source`` = (the given
    frames (R, J, 2) raw in the model's layout, their (R, J) uint8 joint flags or None) as the root solve reads them.
    ``distortion``: the (tracks, 10) float64 rows of ``options.stage_options(...).lens``: uu3d_undistort_points runs first of all."""
    import torch

    def frames(given):
        if key_stride <= 0:
            return given
        if lengths is None or len(lengths) != len(given):
            raise ValueError("keyframes_only needs `lengths`: the number of frames of every track")
        lens = np.asarray(lengths, np.int64)
        want = np.array([keyframe_count(n, key_stride) for n in lens], np.int64)
        if (given != want).any():
            i = int(np.flatnonzero(given != want)[0])
            raise ValueError(f"track {i}: {int(lens[i])} frames at keyframe stride {key_stride} are {int(want[i])} keyframes, got {int(given[i])}")
        return lens

    def write(src, J, given, lens, resolutions, valid_in):
        if valid is None and key_stride <= 0 and resolutions is None:
            return src, None, lens                                    # nothing to write: the caller's own tensor is the table
        kp = torch.empty((int(lens.sum()), J, 2), dtype=torch.float32, device=src.device)      # (never in the caller's own memory)
        flags = None if valid is None else torch.empty((int(lens.sum()),), dtype=torch.uint8, device=src.device)
        normalize_tracks(src, kp, lens, resolutions, key_stride, given, valid_in=valid_in, valid_out=flags)
        return kp, flags, lens

    return _table_front(tracks, device, resolutions, valid, repair_joints, keypoints, model, keep_source, frames, write, distortion)[:2]


def resampled_pose_table(tracks, device, fps, resolutions=None, valid=None, model_fps=50, repair_joints=None, keypoints=None, model=None,
                         keep_source=False, distortion=None):
    """``pose_table`` for tracks at ``fps`` frames per second: the dense, normalised table on the MODEL's time grid (``resample_plan``,
    uu3d_resample_tracks; always a fresh buffer) -> (table, model frames per track, source frames per track).  With ``valid`` the table
    carries one flag per model frame.  ``repair_joints`` = G: uu3d_repair_joints runs on the source frames first; ``table.joint_state`` is
    its (source frames, J) uint8 state.  ``keypoints`` / ``model`` / ``keep_source`` / ``distortion`` as ``pose_table``: the undistortion
    and the map run on the source frames, in front of the rest."""
    import torch

    def write(src, J, given, lens, resolutions, valid_in):
        model_lens, left, right, weight = resample_plan(given, fps, model_fps)
        kp = torch.empty((int(model_lens.sum()), J, 2), dtype=torch.float32, device=src.device)
        flags = None if valid is None else torch.empty((int(model_lens.sum()),), dtype=torch.uint8, device=src.device)
        resample_tracks(src, kp, model_lens, left, right, weight, resolutions, valid_in=valid_in, valid_out=flags)
        return kp, flags, model_lens

    return _table_front(tracks, device, resolutions, valid, repair_joints, keypoints, model, keep_source, lambda given: given, write, distortion)
