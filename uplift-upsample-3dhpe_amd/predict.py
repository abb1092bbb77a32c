"""3D poses for your own 2D keypoint tracks: ``predict_tracks`` takes the 2D keypoints of any number of videos -- from any detector, given
for every frame or only for every ``s_in``-th one -- and returns one 3D pose per frame of every video, on the device.

    pixel coordinates  ->  uu3d_normalize_tracks (normalised screen coordinates, keyframes scattered into the dense pose table)
    ->  data.PoseTable / data.SequenceGenerator with the evaluation settings  ->  the windows ``eval.needed_windows`` keeps
    ->  eval.predict_windows' pipeline (device window gather, stride masks, flip in the same forward, ``reuse_frames``)
    ->  uu3d_assemble_tracks (un-flip, average, linear interpolation between predicted frames by ``evaluation.keyframe_plan``, root shift)

Any frame rate: the model was trained at one rate (Human3.6M: 50 Hz).  ``predict_tracks(..., fps=F)`` takes tracks filmed at F frames per
second -- 24, 25, 29.97, 30, 60, one rate per track if need be -- and returns the poses at the tracks' own frames (or at ``out_fps``):

    pixel coordinates  ->  uu3d_resample_tracks (the pose table on the MODEL's time grid: ``resample_plan`` places model frame k at source
    position k F / 50 in exact integer arithmetic; a model frame that coincides with a source frame is that frame's bits, the others are
    mixed from their two neighbours in float64)  ->  the same windows and forwards  ->  uu3d_assemble_tracks with the plan of
    ``evaluation.keyframe_plan_at`` (the piecewise-linear motion through the predicted model frames, read at the times of the output frames)

The network only reads model frames whose index is a multiple of the input stride s_in; at 30 fps and s_in = 5 these are the video frames
0, 3, 6, ..., at 25 fps every video frame (s_in even), at 60 fps and s_in = 5 the video frames 0, 6, 12, ...: nothing is interpolated on
the input side then.  Without ``fps`` the tracks are taken at the model's rate and nothing is resampled.  Between the first window
gather and the return nothing is copied to the host.  What still waits for the device inside the call: ``eval.predict_windows``
synchronises the stream once after the last forward (its pipeline's buffers go away) and reads the f16x3 range flag; with
``reuse_frames`` it also reads one frame count per chunk of the feature table.  The kernels of this module and their uploads
(pinned, asynchronous) never wait.

    python -m uplift_upsample_3dhpe_amd.predict --config C --weights W.h5 --input tracks.npz --output out.npz \\
        [--resolution W H] [--mask_stride S] [--keyframes_only] [--mask_missing] [--fps F] [--out_fps F]
"""
import argparse
import ctypes as C

import numpy as np

from . import _capi, evaluation
from . import eval as ev
from ._capi import ptr as _ptr
from .data import PoseTable, SequenceGenerator
from .rates import _rate_argument, default_mask_stride, frame_rate, frame_rates, output_positions, resample_plan  # noqa: F401 (re-exported)


def _upload(a, dtype, device):
    """Host array -> device tensor through pinned memory, asynchronously: the host never waits for the stream."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).pin_memory().to(device, non_blocking=True)


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


def assemble_tracks(plain, flipped, left, right, weight, flip_order=None, root=-1):
    """uu3d_assemble_tracks on the current stream.  ``plain`` / ``flipped`` (W, J, 3) float32 on the device (``flipped`` None: no flip);
    ``left`` / ``right`` / ``weight``: the plan of ``evaluation.keyframe_plan`` with rows of those arrays (host arrays of F entries);
    ``root`` >= 0: that joint is subtracted.  -> (F, J, 3) float32 on the device."""
    import torch
    lib = _capi.load_library()
    dev = plain.device
    W, J = int(plain.shape[0]), int(plain.shape[1])
    F = len(left)
    if plain.dtype != torch.float32 or not plain.is_contiguous() or plain.dim() != 3 or plain.shape[2] != 3:
        raise ValueError("plain must be a contiguous (W, J, 3) float32 device tensor")
    if flipped is not None and (flipped.shape != plain.shape or flipped.dtype != torch.float32 or not flipped.is_contiguous()):
        raise ValueError("flipped must match plain")
    if flipped is not None and (flip_order is None or len(flip_order) != J):
        raise ValueError("flipped predictions need the J entries of AUGM_FLIP_KEYPOINT_ORDER")
    d_left, d_right = _upload(left, np.int32, dev), _upload(right, np.int32, dev)
    d_weight = _upload(weight, np.float64, dev)
    d_order = None if flipped is None else _upload(flip_order, np.int32, dev)
    out = torch.empty((F, J, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(lib, lib.uu3d_assemble_tracks(_ptr(plain), _ptr(flipped), W, _ptr(d_order), _ptr(d_left), _ptr(d_right), _ptr(d_weight),
                                                  F, J, int(root), _ptr(out), C.c_void_p(stream)), None)
    return out


def _device_track(t, device):
    import torch
    if isinstance(t, torch.Tensor):
        t = t.to(device=device, dtype=torch.float32)
    else:
        t = _upload(np.asarray(t), np.float32, device)
    if t.dim() != 3 or t.shape[2] != 2:
        raise ValueError(f"a track must be (T, J, 2), got {tuple(t.shape)}")
    return t


def keyframe_count(length, stride):
    """Frames 0, stride, 2 stride, ... of a track of ``length`` frames."""
    return (int(length) + int(stride) - 1) // int(stride)


def check_valid(valid, given):
    """``predict_tracks``' ``valid`` argument against the frames given per track (``given``; keyframes with ``keyframes_only``): None,
    "finite" or one (T_i,) array / tensor per track.  Shapes only: nothing touches a device."""
    if valid is None or (isinstance(valid, str) and valid == "finite"):
        return
    if isinstance(valid, str) or not isinstance(valid, (list, tuple)):
        raise ValueError('valid must be None, "finite" or a list with one (T_i,) array per track')
    if len(valid) != len(given):
        raise ValueError(f"valid must have one entry per track: {len(given)} tracks, {len(valid)} entries")
    for i, (v, n) in enumerate(zip(valid, given)):
        shape = tuple(v.shape) if hasattr(v, "shape") else np.asarray(v).shape
        if shape != (int(n),):
            raise ValueError(f"valid[{i}] must be ({int(n)},): one flag per given frame of track {i}, got {shape}")


def _device_valid(valid, device):
    """The list form of ``valid`` -> one (sum of given frames,) uint8 device tensor; host arrays go up in one pinned, asynchronous copy."""
    import torch
    if not any(isinstance(v, torch.Tensor) for v in valid):
        return _upload(np.concatenate([np.asarray(v).reshape(-1) != 0 for v in valid]).view(np.uint8), np.uint8, device)
    parts = []
    for v in valid:
        if isinstance(v, torch.Tensor):
            v = v if v.is_cuda else v.contiguous().pin_memory().to(device, non_blocking=True)
            parts.append((v != 0).to(device=device, dtype=torch.uint8))
        else:
            parts.append(_upload((np.asarray(v) != 0).view(np.uint8), np.uint8, device))
    return torch.cat(parts, 0)


def _device_tracks(tracks, device):
    """The tracks on the device -> (list of (T_i, J, 2) tensors, J, frames given per track)."""
    tr = [_device_track(t, device) for t in tracks]
    if not tr:
        raise ValueError("no tracks")
    J = int(tr[0].shape[1])
    if any(int(t.shape[1]) != J for t in tr):
        raise ValueError("all tracks must have the same number of keypoints")
    return tr, J, np.array([int(t.shape[0]) for t in tr], np.int64)


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


def pose_table(tracks, device, resolutions=None, key_stride=0, lengths=None, valid=None):
    """The dense, normalised ``data.PoseTable`` of the tracks (uu3d_normalize_tracks) -> (table, frames per track).  ``valid`` as in
    ``predict_tracks`` (not None: uu3d_normalize_tracks_valid into a fresh buffer; the table carries the per-frame flags)."""
    import torch
    check_valid(valid, [len(t) for t in tracks])
    tr, J, given = _device_tracks(tracks, device)
    if key_stride > 0:
        if lengths is None or len(lengths) != len(tr):
            raise ValueError("keyframes_only needs `lengths`: the number of frames of every track")
        lens = np.asarray(lengths, np.int64)
        want = np.array([keyframe_count(n, key_stride) for n in lens], np.int64)
        if (given != want).any():
            i = int(np.flatnonzero(given != want)[0])
            raise ValueError(f"track {i}: {int(lens[i])} frames at keyframe stride {key_stride} are {int(want[i])} keyframes, got {int(given[i])}")
    else:
        lens = given
    if (lens < 1).any():
        raise ValueError("every track needs at least one frame")
    resolutions = check_resolutions(resolutions, len(tr))
    src = torch.cat(tr, 0).contiguous() if len(tr) > 1 else tr[0].contiguous()
    flags = None
    if valid is not None:
        kp = torch.empty((int(lens.sum()), J, 2), dtype=torch.float32, device=src.device)      # (never in the caller's own memory)
        flags = torch.empty((int(lens.sum()),), dtype=torch.uint8, device=src.device)
        normalize_tracks(src, kp, lens, resolutions, key_stride, given, valid_in=None if isinstance(valid, str) else _device_valid(valid, src.device),
                         valid_out=flags)
    elif key_stride > 0 or resolutions is not None:
        kp = torch.empty((int(lens.sum()), J, 2), dtype=torch.float32, device=src.device)      # (never in the caller's own memory)
        normalize_tracks(src, kp, lens, resolutions, key_stride, given)
    else:
        kp = src
    return PoseTable.from_device(kp, lens, valid=flags), lens


def resampled_pose_table(tracks, device, fps, resolutions=None, valid=None, model_fps=50):
    """``pose_table`` for tracks at ``fps`` frames per second: the dense, normalised table on the MODEL's time grid (``resample_plan``,
    uu3d_resample_tracks; always a fresh buffer) -> (table, model frames per track, source frames per track).  With ``valid`` the table
    carries one flag per model frame."""
    import torch
    check_valid(valid, [len(t) for t in tracks])
    tr, J, lens = _device_tracks(tracks, device)
    if (lens < 1).any():
        raise ValueError("every track needs at least one frame")
    resolutions = check_resolutions(resolutions, len(tr))
    model_lens, left, right, weight = resample_plan(lens, fps, model_fps)
    src = torch.cat(tr, 0).contiguous() if len(tr) > 1 else tr[0].contiguous()
    kp = torch.empty((int(model_lens.sum()), J, 2), dtype=torch.float32, device=src.device)
    flags = None if valid is None else torch.empty((int(model_lens.sum()),), dtype=torch.uint8, device=src.device)
    resample_tracks(src, kp, model_lens, left, right, weight, resolutions,
                    valid_in=None if valid is None or isinstance(valid, str) else _device_valid(valid, src.device), valid_out=flags)
    return PoseTable.from_device(kp, model_lens, valid=flags), model_lens, lens


def predict_tracks(model, config, tracks, resolutions=None, mask_stride=None, flip=None, keyframes_only=False, reuse_frames=True,
                   batch_size=None, root_relative=True, depth=None, lengths=None, graph=True, valid=None, return_valid=False, fps=None, out_fps=None,
                   model_fps=50):
    """One 3D pose per frame for each 2D keypoint track -> list of (T_i, J, 3) float32 tensors on the model's device (views of one buffer).

    ``tracks``: list of (T_i, J, 2) arrays or tensors, on the host or the device, at the frame rate the config was trained for (nothing is
    resampled) unless ``fps`` says otherwise.  ``resolutions``: None = the coordinates are normalised already (``h36m.normalize_screen_coordinates``), else one (w, h) in
    pixels or one per track.  ``mask_stride`` (default: the config's first MASK_STRIDE) is the input stride s_in: the network sees frames
    0, s_in, 2 s_in, ... of a track only.  ``flip`` (default config.EVAL_FLIP): mirrored copy in the same forward, averaged.
    ``root_relative``: joint config.ROOT_KEYTPOINT is subtracted (it comes out exactly 0), as the evaluation compares poses.

    ``keyframes_only=True``: ``tracks[i]`` holds only the frames 0, s_in, 2 s_in, ... and ``lengths[i]`` says how many frames T_i the video
    has.  All other frames are masked and never reach the network, so the result equals the full-track call bit for bit -- with one
    exception that the window rules of the reference bring: "copy" padding behind the end of a track repeats the last frame whose index is
    a multiple of SEQUENCE_STRIDE, and when s_in > SEQUENCE_STRIDE that frame need not be one of the given ones.  It is read as zeros
    then, and the frames whose window reaches beyond the end of their track (the last SEQUENCE_LENGTH // 2 * SEQUENCE_STRIDE) may differ
    from the full-track call; all earlier frames are still bit-identical (``padding_source_is_keyframe`` tells which case a track is).

    Frames are predicted by the model where ``eval.needed_windows`` keeps their window (every SEQUENCE_STRIDE-th with TEST_STRIDED_EVAL) and
    interpolated linearly in between by the rules of ``evaluation.interpolate_between_keyframes``; frames behind the last predicted one
    repeat it.  ``reuse_frames`` / ``batch_size`` (default config.BATCH_SIZE) / ``depth`` / ``graph`` go to ``eval.predict_windows``; a
    model with generic dimensions has no frames form and runs the window forward.  One rank only.

    Missed detections -- ``valid``: None = every frame is an observation (today's call, the same bits).  "finite": a frame with a NaN or
    Inf coordinate is MISSING.  A list with one (T_i,) array or tensor per track (host or device; with ``keyframes_only`` one entry per given
    keyframe): 0 = missing, ANDed with the finite test.  A missing frame is never shown to the network: every window token that would read
    it becomes the learned masked token, exactly like a frame the mask stride drops (also where "copy" padding would repeat it), and its
    row of the pose table is zeros -- whatever its coordinates were, they change no bit of the result.  Its 3D pose is still returned: the
    network upsamples over it as it does between keyframes.  The pose table is then a fresh buffer, the caller's memory is never written.
    Needs a model with strided input (ValueError otherwise).  ``return_valid=True``: -> (poses, flags), flags a list of (T_i,) bool device
    tensors with the effective per-frame flags (frames between keyframes that were not given: True).

    Any frame rate -- ``fps``: None = the tracks are at ``model_fps`` (today's call, the same bits, no further launch or buffer).  Else the
    rate the tracks were filmed at: one for all tracks or a list with one per track, each an int, a ``fractions.Fraction``, a
    ``(num, den)`` tuple of two integers (a tuple of two integers is always ONE rate; give two per-track rates as a list) or a float, which
    is taken as ``Fraction(f).limit_denominator(1001)`` (29.97 -> 2997/100, 23.976 -> 2997/125, 30000 / 1001 itself); non-finite or <= 0:
    ValueError.  The pose table is built on the model's time grid on the device (``resample_plan``, uu3d_resample_tracks): a track of T
    frames becomes T' = ceil((T - 1) model_fps / fps) + 1 model frames, model frame k at source position k fps / model_fps -- exactly a
    source frame where that is a whole number (its bits, nothing interpolated), else mixed linearly from its two neighbours; a position
    behind the last source frame repeats it.  ``out_fps`` (default ``fps``) is the rate of the returned poses: output frame i is the pose
    at time i / out_fps, read from the piecewise-linear motion through the predicted model frames (``evaluation.keyframe_plan_at``), and a
    track has floor((T - 1) out_fps / fps) + 1 of them -- T by default.  A detector that ran on every k-th frame of a video: fps =
    video rate / k, out_fps = video rate.  ``valid`` stays per SOURCE frame; a model frame is a real observation iff its left source frame
    is valid and finite and, where it is mixed from two, its right one too.  ``return_valid=True`` with ``fps`` returns the flags on the
    MODEL's grid, (T'_i,) tensors, not per returned pose.  ``fps`` with ``keyframes_only=True`` raises ValueError: say
    ``fps=video rate / s_in, out_fps=video rate`` instead."""
    import torch
    if fps is None and out_fps is not None:
        raise ValueError("out_fps needs fps: the rate the tracks were filmed at")
    if fps is not None and keyframes_only:
        raise ValueError("fps and keyframes_only exclude each other: for a detector that ran on every k-th frame pass the given frames with "
                         "fps=video_rate / k and out_fps=video_rate")
    if valid is not None and not model.has_strided_input:
        raise ValueError("valid needs a model with strided input: a missing frame becomes the learned masked token, which this model does not have")
    check_valid(valid, [len(t) for t in tracks])
    dev = model.device
    cfg = config.copy()
    if mask_stride is None:
        mask_stride = default_mask_stride(cfg)
    cfg.MASK_STRIDE = mask_stride
    flip = bool(cfg.EVAL_FLIP) if flip is None else bool(flip)
    if keyframes_only and mask_stride is None:
        raise ValueError("keyframes_only needs a mask stride")
    if fps is None:
        table, lens = pose_table(tracks, dev, resolutions, int(mask_stride) if keyframes_only else 0, lengths, valid=valid)
        model_lens = lens
    else:
        rates = frame_rates(fps, len(tracks))
        table, model_lens, src_lens = resampled_pose_table(tracks, dev, rates, resolutions, valid=valid, model_fps=model_fps)
        lens, positions = output_positions(src_lens, rates, rates if out_fps is None else out_fps, model_fps)
    gen = SequenceGenerator(table, seq_len=cfg.SEQUENCE_LENGTH, target_frame_rate=50, subsample=1, stride=cfg.SEQUENCE_STRIDE,
                            padding_type=cfg.PADDING_TYPE, flip_augment=False, flip_lr_indices=cfg.AUGM_FLIP_KEYPOINT_ORDER,
                            mask_stride=mask_stride, stride_mask_align_global=True, rand_shift_stride_mask=False, shuffle=False)
    desc = gen.descriptors()                                         # one window per frame, in table order: position p is table row p
    frame_idx = desc[:, 1]
    run = np.flatnonzero(ev.needed_windows(frame_idx, cfg))
    raw = ev._predict_windows_raw(model, gen, desc[run], int(batch_size or cfg.BATCH_SIZE), flip, depth, graph,
                                  bool(reuse_frames) and bool(model.arch.compiled_dims))
    rows = np.full(len(desc), -1, np.int64)
    rows[run] = np.arange(len(run))
    stride = ev.prediction_stride(cfg)
    if fps is not None:
        left, right, weight = evaluation.keyframe_plan_at(frame_idx, 1 if stride is None else stride, positions, rows=rows)
    elif stride is None:
        left = right = rows
        weight = np.zeros(len(desc), np.float64)
    else:
        left, right, weight, _ = evaluation.keyframe_plan(frame_idx, stride, rows=rows)
    out = assemble_tracks(raw[0], raw[1] if flip else None, left, right, weight, flip_order=cfg.AUGM_FLIP_KEYPOINT_ORDER,
                          root=int(cfg.ROOT_KEYTPOINT) if root_relative else -1)
    poses = list(torch.split(out, [int(n) for n in lens], 0))
    if not return_valid:
        return poses
    flags = table.valid.view(torch.bool) if table.valid is not None else torch.ones((int(model_lens.sum()),), dtype=torch.bool, device=out.device)
    return poses, list(torch.split(flags, [int(n) for n in model_lens], 0))


def padding_source_is_keyframe(length, config, mask_stride):
    """Whether the frame that "copy" padding repeats behind the end of a track of ``length`` frames (the last one whose index is a multiple
    of SEQUENCE_STRIDE: the windows that are run are centred on such frames) is a multiple of ``mask_stride`` too -- then
    ``keyframes_only`` input gives the bits of the full track on every frame.  True for zero padding."""
    if config.PADDING_TYPE != "copy":
        return True
    s = int(config.SEQUENCE_STRIDE)
    return ((int(length) - 1) // s * s) % int(mask_stride) == 0


def _load_model(config, weights_path):
    from .net.uplift_upsample_transformer_constructor import build_uplift_upsample_transformer
    model = build_uplift_upsample_transformer(config)
    model.load_weights(weights_path, skip_mismatch=False, verbose=False)
    return model


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m uplift_upsample_3dhpe_amd.predict", description="3D poses for the 2D keypoint tracks of an .npz file "
                                "(one (T, J, 2) array per track) -> an .npz with the same keys and (T, J, 3) float32 arrays.")
    p.add_argument("--config", required=True, help="model config (.json)")
    p.add_argument("--weights", required=True, help="weights (.h5)")
    p.add_argument("--input", required=True, help=".npz with one (T, J, 2) array per track")
    p.add_argument("--output", required=True, help=".npz to write")
    p.add_argument("--resolution", type=float, nargs=2, metavar=("W", "H"), default=None,
                   help="image size in pixels of all tracks; without it the coordinates are taken as normalised already")
    p.add_argument("--mask_stride", type=int, default=None, help="input stride s_in (default: the config's first MASK_STRIDE)")
    p.add_argument("--keyframes_only", action="store_true",
                   help="the arrays hold frames 0, s_in, 2 s_in, ... only; a track of K keyframes is taken to have (K - 1) * s_in + 1 frames")
    p.add_argument("--mask_missing", action="store_true",
                   help="a frame with a NaN or Inf coordinate is a missed detection: never shown to the network, its pose is still predicted")
    p.add_argument("--fps", type=_rate_argument, default=None, metavar="F",
                   help="frame rate of the tracks, a float or NUM/DEN (29.97, 30000/1001); without it they are taken at the model's rate")
    p.add_argument("--out_fps", type=_rate_argument, default=None, metavar="F", help="frame rate of the poses written (default: --fps)")
    return p.parse_args(argv)


def main(argv=None):
    from .net.uplift_upsample_transformer_config import UpliftUpsampleConfig
    args = parse_args(argv)
    config = UpliftUpsampleConfig(args.config)
    with np.load(args.input) as z:
        names = list(z.files)
        tracks = [np.asarray(z[k], np.float32) for k in names]
    if not names:
        raise SystemExit(f"{args.input} holds no arrays")
    for k, t in zip(names, tracks):
        if t.ndim != 3 or t.shape[2] != 2 or t.shape[1] != config.NUM_KEYPOINTS:
            raise SystemExit(f"{args.input}[{k}] has shape {t.shape}, expected (T, {config.NUM_KEYPOINTS}, 2)")
    ms = default_mask_stride(config) if args.mask_stride is None else args.mask_stride
    lengths = None
    if args.keyframes_only:
        if ms is None:
            raise SystemExit("--keyframes_only needs a mask stride")
        lengths = [(len(t) - 1) * int(ms) + 1 for t in tracks]
    model = _load_model(config, args.weights)
    if args.out_fps is not None and args.fps is None:
        raise SystemExit("--out_fps needs --fps")
    rate = {} if args.fps is None else {"fps": args.fps, **({} if args.out_fps is None else {"out_fps": args.out_fps})}
    poses = predict_tracks(model, config, tracks, resolutions=None if args.resolution is None else tuple(args.resolution), mask_stride=ms,
                           keyframes_only=args.keyframes_only, lengths=lengths, **({"valid": "finite"} if args.mask_missing else {}), **rate)
    np.savez(args.output, **{k: np.asarray(p.detach().cpu().numpy(), np.float32) for k, p in zip(names, poses)})
    print(f"wrote {args.output}: {len(names)} tracks, {sum(int(p.shape[0]) for p in poses)} frames", flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
