"""Live uplifting: ``StreamSession`` takes one frame of 2D keypoints per track and tick and returns one 3D pose per track, on the device.

    s = StreamSession(model, config, slots=T, resolutions=(1920, 1080), lookahead=0)
    poses, fresh = s.push(kp2d)            # (T, J, 2) host or device -> (T, J, 3) float32, (T,) bool, both on the device

The one rule (the truncation identity): after the push that made frame t the newest of a track, the session emits the pose of frame
c = t - lookahead -- when c >= 0 and ``eval.needed_windows`` keeps the window centred on c (TEST_STRIDED_EVAL: c % SEQUENCE_STRIDE == 0) --
and that pose is what ``predict.predict_tracks`` returns for frame c of the track cut to its first t + 1 frames (same ``mask_stride``,
``flip``, ``resolutions``, ``root_relative``).  Frames of the window that do not exist yet are padded by the config's PADDING_TYPE, as the
end of a video is.  On every other push the slot's previous pose is held and reported as not fresh; nothing is interpolated.

Per tick (include/uu3d.h, LIVE TRACKS): uu3d_stream_stage -> uu3d_frame_features on the ``slots`` (x 2 with flip) new
frames -> uu3d_stream_commit (counters, keyframe ring, edge row, this tick's window rows and masks) -> uu3d_forward_frames_ex from the
session's resident feature table -> uu3d_stream_emit.  The spatial stack runs once per pushed frame, not once per frame of the window.  The
per-track counters live on the device, so the five steps are ONE captured hipGraph (``graph=True``) replayed at every tick; ``push`` never
waits for the device.
All arguments are the same at every push, so the constructor decides the session's mode once and builds its launch tables (the steps of a
tick, the launches of a push around them, the reset: library functions with their prebuilt arguments); ``push`` and ``reset`` walk them.
The integer planning of rates and strides (``rate_plan``, ``push_plan``, ``out_push_plan``, ``session_strides``) is ``rates.py``.

Any frame rate -- ``StreamSession(..., fps=F, model_fps=50)``: one SOURCE frame per slot and push, at F frames per second, and one pose per
slot and push, at the source frame's own time; everything on the device, ``push`` still never waits.  With model_fps / F = A / B in lowest
terms (exact integers; ``rates.rate_plan``, ``rates.push_plan``):
  input   model frame k sits at source position k B / A (``rates.resample_plan``'s definition) and is made the moment source frame
          ceil(k B / A) has been pushed: that source frame's bits where the position is whole, else the two neighbours normalised and then
          mixed in float64 with resample_plan's own weight (the device functions of uu3d_resample_tracks).  After a slot's j-th push
          (0-based) its newest model frame is K = floor(j A / B); the push made K - floor((j - 1) A / B) model frames -- 1 at j = 0, then
          0 .. ceil(A / B).
  model   every new model frame is one tick of the plain session (a SUB-TICK: uu3d_stream_resample_stage in place of uu3d_stream_stage,
          then features, commit, forward, emit as above, then uu3d_stream_file_keyframe) at the model lookahead a_m: the session with ``fps``
          IS a plain session at lookahead a_m fed the resampled model-rate frames.
  output  ``poses[i]`` is the pose of source frame q = j - lookahead of slot i (``lookahead`` counts SOURCE frames), read at model position
          u = q A / B from the piecewise-linear motion through the emitted keyframes (centres that are multiples of the prediction stride
          P; the rule of ``evaluation.keyframe_plan_at``, as ``predict_tracks(fps=F)``): k0 = floor(u / P) P, k1 = k0 where u == k0, else
          k0 + P; u == k0 gives that keyframe's bits, anything else float32(p0 (1 - w) + p1 w) in float64, w = (q A - k0 B) / (P B).
          ``fresh[i]`` is set on EVERY push with q >= 0 of an active slot, not only at keyframes; otherwise the previous pose is held.
  a_m     the largest integer in [0, max_lookahead(config)] with k1(j - lookahead) <= floor(j A / B) - a_m for every j >= lookahead: k1 has
          been emitted when it is read.  The condition repeats in j with period B P and is enumerated exactly; when no a_m >= 0 exists
          the constructor raises ValueError naming the smallest sufficient ``lookahead``.  The emitted keyframes live per slot in a ring of
          D poses, centre c at place (c / P) % D, D - 1 = the largest distance in keyframes from the newest emitted centre back to k0.
``fps=None`` is the session above, bit for bit: the same launches, the same buffers, the same single captured graph.

Live upsampling -- ``StreamSession(..., fps=F, out_fps=G, model_fps=50)``: the session returns poses on a time grid of its own, G per second,
EVERY one that has become due per push -- a camera at 50 fps whose detector runs on every fifth frame (fps=10, out_fps=50) gets its 50
poses a second, five per push.  Input and model sides, ``lookahead`` (SOURCE frames), a_m and ``missed_detections`` as above; the rules are
``rates.output_positions``' and ``evaluation.keyframe_plan_at``'s, as ``predict_tracks(fps=F, out_fps=G)``:
  grid    output frame i of a slot lies at time i / G, model position u = i model_fps / G, and is read like a source frame above:
          k0 = floor(u / P) P; u == k0 gives that keyframe's bits, anything else float32(p0 (1 - w) + p1 w) in float64, w one float64
          division of two integers.
  push    after the push that made source frame j the newest of a slot, q = j - lookahead >= 0, the slot has emitted every output frame
          i <= floor(q G / F): the frames whose time is not later than source frame q's.  The push returns the ones that became due at it,
          oldest first -- frame 0 alone at q == 0, then floor(q G / F) - floor((q - 1) G / F): at most R = ceil(G / F) (``max_out``),
          possibly none when G < F; an inactive slot returns none.  ``push`` -> (poses (slots, R, J, 3), count (slots,) int32); rows
          r >= count[i] are zeros; ``out_frames`` counts the output frames per slot on the device.
  ring    the oldest output frame of a push lies just behind source frame q - 1, so its k0 can be one keyframe older than k0(q): D is
          enumerated over one common period of the three grids (source frames, output frames, keyframes); a_m needs no change -- no due
          frame is later than source frame q -- which the enumeration checks as well (``rate_plan``, ``out_push_plan``).
One launch (uu3d_stream_timed_emit_multi) in place of uu3d_stream_timed_emit; ``out_fps=None`` is the session above, bit for bit.

Live C1 motion -- ``StreamSession(..., fps=F, interpolation="cubic")``, with or without ``out_fps``: the poses of the two sessions above
read from the C1 Catmull-Rom cubic through the emitted keyframes in place of the line, as ``predict_tracks(interpolation="cubic")`` reads
them offline; the velocity of the returned motion no longer jumps at every keyframe.  One rule everywhere (``rates.keyframe_bracket``,
``evaluation.interpolate_cubic_host``; ``rates.push_plan_cubic`` / ``out_push_plan_cubic`` are the host mirrors):
  rule    k0, k1 and the weight w as above.  u == k0 gives keyframe k0's bits.  Anything else is the Hermite segment from keyframe k0 to
          keyframe k1 at t = w whose tangents come from keyframe k0 - P (a slot's first segment, k0 == 0, has none and takes the
          segment's own difference, as the offline rule does at a track's first segment) and keyframe k1 + P (always: a live track has no
          last segment, and ``finish`` stays refused with ``fps``): float64 on the float32 keyframes, every operation rounded, no fused
          multiply-add, rounded once to float32 -- the device equals numpy bit for bit.  The root joint of a root-relative pose stays 0.
  plan    ``rate_plan(..., interpolation="cubic")``: the newest emitted centre must reach k1 + P wherever a pose is not on a keyframe, so
          the smallest ``lookahead`` rises (ValueError naming the cubic's minimum) and a_m falls; with ``out_fps`` that slack is taken
          over the output frames of every push, because a frame just in front of a source frame that sits on a keyframe needs the
          keyframe behind it.  The ring keeps k0 - P of the oldest pose a push reads: D grows, through ``rate->key_ring`` alone.
  launch  uu3d_stream_timed_emit_cubic / uu3d_stream_timed_emit_multi_cubic in place of the linear emit, a plain launch as before; the
          ring, the state, the sub-tick graph (``captures`` stays 1), the resets and everything appended behind the emit (bones, root
          solve, filters, rotations: they read the buffer it wrote) are unchanged.  ``interpolation="linear"`` is the session above, bit for
          bit.  Without ``fps``: ValueError -- a plain session holds the previous pose between keyframes.

The options of a session, one stage module each -- what the option does live, its launches in the tick and its host mirror stand in the
module's docstring; every name is importable from here as before:
    validity.py   live per-joint missed detections: ``StreamSession(..., repair_joints=G)`` (``LiveRepairHost``, ``MAX_LIVE_REPAIR``)
    keypoints.py  any skeleton: ``StreamSession(..., keypoints=M)``
    associate.py  per-frame detections: ``StreamSession(..., detections=D, max_age=, max_dist=, min_common=)`` and ``push_detections``
    roots.py      live absolute root: ``StreamSession(..., camera=(fx, fy, cx, cy), min_root_joints=6)`` (``LiveRoot``, ``LiveRootHost``)
    smooth.py     steady output: ``StreamSession(..., smooth=F)`` (``LiveOneEuro``, ``LiveOneEuroHost``)
    bones.py      live constant bone lengths: ``StreamSession(..., bones=B)`` (``LiveBones``, ``LiveBonesHost``)
    rotations.py  live joint rotations: ``StreamSession(..., rotations=R)`` (``LiveRotations``: uu3d_joint_rotations as the tick's last launch)
    live_views.py live several views: ``StreamSession(..., slots=V * N, camera=[V Cameras with extrinsics], views=V)`` (``LiveViews``: uu3d_stream_views
                  behind uu3d_camera_to_world; ``LiveViewsHost``, ``replay_views``)
    camera.py     lens distortion: ``StreamSession(..., camera=Camera(fx, fy, cx, cy, distortion=...))`` (uu3d_undistort_points as the tick's first launch);
                  world space: ``StreamSession(..., camera=Camera(..., orientation=, translation=))`` (``LiveWorld``: uu3d_camera_to_world behind uu3d_stream_root)
The refusals these options share with ``predict_tracks`` are ``options.stage_options``; the ones only a session has are ``_init_plan``'s.
The output-side options (bones, root, world, views, the two filters, rotations) are device objects of one shape (``smooth.LiveOneEuro``); the
session hands a ``Scene`` through them in that order and walks the list for its launch tables.  The input-side ones stay inline.

The end of a track -- ``finish(slots)``: a session with lookahead a has not returned the poses of a track's last a frames when the track
ends (the person leaves, the video stops).  ``finish`` returns them -- (slots, a, J, 3) and (slots, a) on the device -- and resets exactly
those slots: it enqueues a DRAIN TICKS, each of which moves the centre of the slot's window one frame towards its newest frame and files
NOTHING (uu3d_stream_drain_commit: the window of centre len - 1 - a + k through the same row rule, the frames behind the track's end padded
as the end of a video is), then the tick's own forward and emit, the root solve from the ring (uu3d_stream_root_drain), the filters as they
are at the virtual counter len + k, and uu3d_stream_drain_file, which copies the tick's rows into row k - 1 of the result (include/uu3d.h,
LIVE TRACKS: END OF A TRACK; csrc/uu3d_stream_drain.h).  No stage, no uu3d_frame_features: everything a drain tick reads is in the ring.
The one rule, extended: row k - 1 is the pose ``predict_tracks`` gives for frame len - 1 - a + k of the WHOLE track, and the bits a session
with lookahead a - k returns at its last push.  The drain ticks are a second launch table (``_drain_steps``) captured lazily at the first
``finish`` as one more linear hipGraph: a session that never finishes a track allocates and launches none of it and ``captures`` stays 1;
afterwards it is 2.  Slots that were not chosen keep every bit of their state.  ``replay_tracks(drain=True)`` finishes each slot at the
tick its own track ends; ``window_plan(drained=k)``, ``LiveRootHost.drain`` and ``LiveOneEuroHost.drain`` are the host mirrors.  Not with
``fps`` / ``out_fps`` (ValueError: a later change).

    python -m uplift_upsample_3dhpe_amd.stream --config C --weights W.h5 --input tracks.npz --output out.npz [--lookahead A] [--resolution W H]
                                                 [--drain] [--mask_missing] [--fps F [--out_fps G]] [--repair_joints G [--min_score S]] [--keypoints NAME]
                                                 [--camera FX FY CX CY [--min_root_joints N]] [--smooth MIN_CUTOFF BETA D_CUTOFF]
                                                 [--smooth_root MIN_CUTOFF BETA D_CUTOFF] [--bones track|FILE.npy]
"""
import argparse
import collections
import ctypes as C
import functools
import gc

import numpy as np

from . import _capi
from ._capi import ptr as _ptr
# (noqa: F401 below -- re-exported: every name this module had before the stages became modules of their own)
from .associate import ASSOCIATION_DEFAULTS, check_association
from .bones import Bones, LiveBones, LiveBonesHost, _bone_offsets, check_bones, fix_bones_host, skeleton_of  # noqa: F401
from .camera import (Camera, LiveWorld, camera_to_world_host, distort_points_host, extrinsics_from_opencv, plain_camera, undistort_points,  # noqa: F401
                     undistort_points_host, world_to_camera_host)
from .cli import add_track_options, bones_option, input_joints, smooth_option, split_scores, track_keywords  # noqa: F401
from .keypoints import KEYPOINT_PRESETS, check_keypoint_inputs, keypoint_map  # noqa: F401
from .live_views import LiveViews, LiveViewsHost, check_live_views, person_mask, replay_views  # noqa: F401
from .options import check_interpolation, stage_options
from .predict import _load_model
from .rates import (RatePlan, _rate_argument, frame_rate, max_lookahead, newest_model_frame, out_push_plan, out_push_plan_cubic,  # noqa: F401
                    push_plan, push_plan_cubic, rate_plan, session_strides)
from .rotations import LiveRotations, Rotations, check_rotations, joint_rotations_host  # noqa: F401
from .roots import DEFAULT_MIN_ROOT_JOINTS, MAX_ROOT_JOINTS, LiveRoot, LiveRootHost, check_cameras, check_min_root_joints, solve_roots_host  # noqa: F401
from .smooth import (MAX_SMOOTH_CHANNELS, LiveOneEuro, LiveOneEuroHost, OneEuro, _live_filter_arguments, check_smooth,  # noqa: F401
                     one_euro_sample)
from .tracks import _host_array, check_resolutions
from .validity import MAX_LIVE_REPAIR, LiveRepairHost, check_repair_joints, check_valid, staged_frames  # noqa: F401


def ring_capacity(config, mask_stride=None, lookahead=0):
    """Keyframes kept per slot: a window centred on newest - lookahead reads frames from (SEQUENCE_LENGTH // 2) * SEQUENCE_STRIDE before its
    centre up to the newest one -- lookahead + half span + 1 consecutive indices, at most this many multiples of s_in."""
    S, s_in, _ = session_strides(config, mask_stride)
    return (int(lookahead) + max_lookahead(config)) // s_in + 1


def emits(frames, lookahead, config, mask_stride=None, drained=0):
    """Whether the push that brought a track to ``frames`` frames emits a pose (of frame ``frames - 1 - lookahead``).  ``drained`` = k in
    1 .. lookahead: whether the k-th drain tick of ``StreamSession.finish`` does, for a track that ended at ``frames`` frames (of frame
    ``frames - 1 - lookahead + k``)."""
    _, _, pred = session_strides(config, mask_stride)
    if not 0 <= int(drained) <= int(lookahead):
        raise ValueError(f"drained must be in [0, lookahead = {int(lookahead)}], got {drained}")
    c = int(frames) - 1 - int(lookahead) + int(drained)
    return int(frames) >= 1 and c >= 0 and c % pred == 0


def window_plan(frames, lookahead, config, mask_stride=None, valid=None, drained=0):
    """The host mirror of uu3d_stream_commit's row rule for a track of ``frames`` frames: None when no pose comes out, else a dict of (N,)
    arrays over the window centred on ``frames - 1 - lookahead`` --
        "mask": the stride mask bit; "src": the frame a real token reads (-1: none -- a masked token, or zero padding);
        "kind": 0 masked token, 1 zero row, 2 keyframe ring, 3 edge row; "place": the ring place of kind 2 (-1 otherwise)
    -- and "centre".  ``valid``: (frames,) flags, 0 = a missing frame (uu3d_stream_commit_valid): a token that reads one is masked --
    mask' = mask and (no frame is read or valid[the frame read]).
    ``drained`` = k in 1 .. lookahead: the mirror of uu3d_stream_drain_commit's k-th drain tick for a track that ENDED at ``frames`` frames
    -- the window centred on ``frames - 1 - lookahead + k``, the frames behind the track's end padded as the end of a video is, in the ring
    of capacity ``ring_capacity(lookahead=lookahead)``: the session files nothing while it drains, so the places are those of its pushes."""
    if not emits(frames, lookahead, config, mask_stride, drained):
        return None
    S, s_in, _ = session_strides(config, mask_stride)
    N, L = int(config.SEQUENCE_LENGTH), int(frames)
    cap = ring_capacity(config, mask_stride, lookahead)
    pad_edge = config.PADDING_TYPE == "copy"
    c = L - 1 - int(lookahead) + int(drained)
    n = np.arange(N, dtype=np.int64)
    f = c - ((N - 1) * S) // 2 + n * S
    src = np.where(f < 0, f + ((-f + S - 1) // S) * S, np.where(f >= L, f - ((f - L + S) // S) * S, f))
    inside = (f >= 0) & (f < L)
    have = inside | (pad_edge & (src >= 0) & (src < L))
    mask = np.mod((n - N // 2) * S + c, s_in) == 0
    if valid is not None:
        v = np.asarray(valid).reshape(-1) != 0
        if len(v) != L:
            raise ValueError(f"valid must have one flag per frame: {L} frames, {len(v)} flags")
        mask = mask & (~have | v[np.clip(src, 0, L - 1)])
    edge_frame = (L - 1) // S * S
    kind = np.zeros(N, np.int64)
    kind[mask & ~have] = 1
    is_edge = mask & have & ~inside & (src == edge_frame)
    kind[is_edge] = 3
    ring = mask & have & ~is_edge
    if (np.mod(src[ring], s_in) != 0).any() or (src[ring] < c - (N // 2) * S).any():
        raise AssertionError("a window token reads a frame that is neither a kept keyframe nor the edge frame")
    kind[ring] = 2
    return {"centre": c, "mask": mask, "src": np.where(kind >= 2, src, -1), "kind": kind,
            "place": np.where(kind == 2, (src // s_in) % cap, -1)}


LIVE_OPTIONS = ("repair_joints", "keypoints", "camera", "min_root_joints", "smooth", "bones", "rotations")  # the keywords ``StreamSession`` and ``replay_tracks`` take from **options
DETECTION_OPTIONS = ("detections",) + tuple(ASSOCIATION_DEFAULTS)    # ... and the ones only ``StreamSession`` takes: per-frame detections
VIEW_OPTIONS = ("views",)                                             # ... and the cameras of a rig (``live_views.py``)


def _live_options(options, who, names=LIVE_OPTIONS):
    """The keywords of ``names`` out of the ``**options`` of ``who``, in that order (None where one is not given); any other keyword
    is the TypeError Python itself raises for an unknown argument."""
    unknown = sorted(k for k in options if k not in names)
    if unknown:
        raise TypeError(f"{who}() got an unexpected keyword argument {unknown[0]!r}")
    return tuple(options.get(name) for name in names)


class Scene(collections.namedtuple("Scene", "poses fresh roots root_state extras")):
    """What a push returns so far, as the output-side stages hand it on: ``poses`` (slots, J, 3) float32, ``fresh`` (slots,) uint8, ``roots``
    (slots, 3) float32 and ``root_state`` (slots,) uint8 or both None (no camera), ``extras``: buffers appended behind them (quaternions)."""
    __slots__ = ()

    def as_result(self):
        import torch
        return (self.poses, self.fresh.view(torch.bool)) + (() if self.roots is None else (self.roots, self.root_state)) + self.extras


def scenes(raw, stages, rows=None):
    """Hand the raw scene through ``stages``, [(name of the scene it leaves, stage or None = absent)] in the tick's order -> {name: scene}: a stage
    reads the scene in front of it and puts its ``outputs`` in place.  ``rows``: the drained rows of ``finish`` by name stand in for the buffers."""
    named, scene = {"raw": raw}, raw
    for name, stage in stages:
        if stage is not None and rows is None:
            stage.read = scene
        for field, row, buffer in (() if stage is None else stage.outputs):
            value = buffer if rows is None else rows[row]
            scene = scene._replace(**{field: scene.extras + (value,) if field == "extras" else value})
        named[name] = scene
    return named


class StreamSession(object):

    def __init__(self, model, config, slots, resolutions=None, mask_stride=None, flip=None, lookahead=0, root_relative=True, graph=True,
                 missed_detections=False, fps=None, model_fps=50, out_fps=None, interpolation="linear", **options):
        """``slots``: tracks served side by side (a slot is a track: ``reset`` starts a new one).  ``resolutions``: None = the coordinates
        are normalised already, else one (w, h) in pixels or one per slot.  ``mask_stride`` / ``flip`` / ``root_relative`` as
        ``predict.predict_tracks``.  ``lookahead`` = a: frames the answer may lag behind the newest one, 0 <= a <=
        (SEQUENCE_LENGTH // 2) * SEQUENCE_STRIDE; with a at its maximum every window is complete.  ``graph``: replay one captured hipGraph
        per tick instead of enqueueing the five steps.  A model with generic dims whose frame does not fit a workgroup's LDS has no
        frames form (``model.has_frames_form``): NotImplementedError; with ``flip`` its config's AUGM_FLIP_KEYPOINT_ORDER must permute its joints.
        A session on a generic model must be rebuilt after a Trainer has stepped on that model: the captured tick replays on whatever the
        shared operand packs hold (include/uu3d.h, FRAMES FORM).
        ``missed_detections=True``: a pushed frame may be MISSING (``push(valid=...)``, or a row with a NaN / Inf coordinate) -- the slot's
        track still grows by that frame, but no window ever shows it to the network (``predict.predict_tracks(valid=...)``); the tick runs
        uu3d_stream_stage_valid / uu3d_stream_commit_valid.  Needs a model with strided input (ValueError).  False: today's session.
        ``fps``: None = the pushed frames are at the model's rate (today's session, bit for bit).  Else the ONE rate of the session's source
        frames, parsed by ``rates.frame_rate`` (int, ``Fraction``, ``(num, den)``, or a float read as
        ``Fraction(f).limit_denominator(1001)``), against ``model_fps``: the module docstring's "Any frame rate".  ``lookahead`` then counts
        SOURCE frames and must be at least ``rate_plan(...).min_lookahead`` (ValueError naming it); ``missed_detections`` flags are per
        source frame, and a model frame is missing under uu3d_resample_tracks' rule: its left source frame is missing or, where it is mixed
        from two, its right one.  ``captures`` counts captures of the sub-tick graph: 1 for the session's whole life -- the source push and
        the timed emit around the replays are two plain launches, not captured.
        ``out_fps``: None = one pose per push, at the source frame's own time (the session above, bit for bit).  Else the rate of the poses
        the session returns, parsed like ``fps`` (which it needs: ValueError without): the module docstring's "Live upsampling".  ``push``
        then returns (poses (slots, max_out, J, 3), count (slots,) int32), ``max_out`` = ceil(out_fps / fps) <= 64, and ``out_frames``
        counts the output frames per slot.
        ``interpolation``: "linear" (the default: the sessions above, bit for bit -- the same launches, buffers and bits) or "cubic": the
        module docstring's "Live C1 motion" -- with ``fps`` (ValueError without: a plain session holds the previous pose between keyframes,
        there is nothing to interpolate), with or without ``out_fps``; ``lookahead`` must then be at least
        ``rate_plan(..., interpolation="cubic").min_lookahead``, the cubic's own minimum.  ``s.interpolation`` tells which.
        ``repair_joints`` (keyword only, taken from ``options``; any other name there is a TypeError): None = a missing joint makes its frame missing (the session above, bit for bit).  Else G, an int in
        [1, ``MAX_LIVE_REPAIR``]: the module docstring's "Live per-joint missed detections".  Implies ``missed_detections=True``;
        ``push(valid=...)`` may then hold one flag per joint and ``joint_state`` tells what became of the newest frame's joints.  Not
        together with ``fps`` / ``out_fps`` (ValueError).
        ``keypoints`` (keyword only, from ``options`` as well): None = the pushed frames are in the model's own joint layout (the session
        above, bit for bit).  Else a name of ``predict.KEYPOINT_PRESETS`` or a ``predict.KeypointMap`` onto the model's joints: the module
        docstring's "Any skeleton".  ``push`` then takes (slots, K_in, 2) frames and, with ``repair_joints``, (slots, K_in) flags.
        ``detections`` (keyword only, from ``options`` as well): None = the caller pushes tracks (the session above, bit for bit).  Else D in
        [1, 64], the most people a frame lists: the module docstring's "Per-frame detections" -- ``push_detections`` in place of ``push``,
        ``slots`` <= 64 is the capacity, the joints the detector emits <= 64.  ``max_age`` / ``max_dist`` / ``min_common``: the rule's
        parameters (``predict.ASSOCIATION_DEFAULTS``: 10, 0.5, 3 -- conveniences, not tuned values).  Implies ``missed_detections=True``; not
        together with ``fps`` / ``out_fps`` (ValueError).
        ``camera`` (keyword only, from ``options`` as well): None = root-relative poses only (the session above, bit for bit).  Else the
        camera's intrinsics (fx, fy, cx, cy) in the units of the pushed frames, one tuple or one per slot (with ``detections`` one tuple
        only): the module docstring's "Live absolute root" -- ``push`` / ``push_detections`` then return (poses, fresh, roots (slots, 3)
        float32, root_state (slots,) uint8).  ``min_root_joints`` (default 6, an int >= 2; ValueError without ``camera``): the fewest used
        joints a frame's root is solved from.  Models of more than ``predict.MAX_ROOT_JOINTS`` joints and ``out_fps``: ValueError.
        A ``predict.Camera(fx, fy, cx, cy, distortion=(k1, k2, p1, p2, k3), tol=1e-3)`` in the tuple's place -- one, one per slot, or with
        ``detections`` one; a mix of tuples and ``Camera``s or of ``Camera``s with and without distortion: ValueError --: "Lens distortion"
        (``camera.py``).  ``push`` files the raw points in a buffer of the session and uu3d_undistort_points is the FIRST step of the one
        captured tick -- in front of uu3d_map_keypoints; with ``fps`` a plain launch in front of uu3d_stream_source_push; with
        ``detections`` on all D x K points in front of the association -- so every push returns, bit for bit, what a session with
        ``camera=(fx, fy, cx, cy)`` returns for ``predict.undistort_points_host`` of the frames.  A point that is not accepted is
        (NaN, NaN): ``missed_detections=True`` (or ``repair_joints``) is the companion option.  ``push`` still never waits, ``captures``
        stays 1; ``reset``, ``finish`` and the replays need nothing new.  Without distortion: the tuple's session, bit for bit.
        A ``predict.Camera(..., orientation=(w, x, y, z), translation=(tx, ty, tz))`` -- one, one per slot, or with ``detections`` one; a
        list of ``Camera``s with and without extrinsics: ValueError --: "World space" (``camera.py``).  uu3d_camera_to_world joins the
        launch table directly behind uu3d_stream_root, in front of the smoothers and the rotations: out of place and stateless, all
        slots at every tick, from the camera-space pose the root solve read and the root and state it wrote into two buffers of the
        session, which the filters and uu3d_joint_rotations read and ``push`` / ``push_detections`` return.  The root solve's held
        state stays in camera space; a slot that is not fresh gets its previous bits again.  ``raw_poses`` / ``raw_roots`` are then the
        unfiltered WORLD buffers, ``camera_poses`` / ``camera_roots`` the camera-space ones; ``finish`` runs the same step behind
        uu3d_stream_root_drain (``drain_raw_*`` / ``drain_camera_*`` likewise).  ``push`` still never waits, ``captures`` stays 1,
        ``reset`` and births need nothing new.  Every push returns, bit for bit, ``predict.camera_to_world_host`` of what the session
        without extrinsics returns.  Without extrinsics: that session, the same launches, buffers and bits.
        ``smooth`` (keyword only, from ``options`` as well): None = the poses and roots as they are solved (the session above, bit for
        bit).  True, a ``predict.OneEuro`` or a pair (pose_filter, root_filter), either of which may be None (``predict.check_smooth``; a
        root filter without ``camera``: ValueError): the module docstring's "Steady output" -- ``push`` / ``push_detections`` return the
        filtered buffers in place of poses and roots; ``raw_poses`` / ``raw_roots`` are the unfiltered ones.  With ``out_fps``: ValueError.
        A ``OneEuro(zero_lag=True)`` in either place: ValueError -- live filtering is causal, the two-pass form needs the whole track
        (``predict.predict_tracks(smooth=...)``).
        ``bones`` (keyword only, from ``options`` as well): None = the poses as the network gives them (the session above, bit for bit).
        "track", a (J,) array of lengths by child joint, a list of such arrays, one per slot, or a ``predict.Bones``: the module
        docstring's "Live constant bone lengths" -- ``push`` returns the rebuilt poses, ``raw_poses`` stays the model's output and
        ``bone_lengths`` is the slots' lengths table.  With ``out_fps``: ValueError.
        ``rotations`` (keyword only, from ``options`` as well): None = positions only (the session above, bit for bit).  True or a
        ``predict.Rotations``: "Live joint rotations" (``rotations.py``) -- ``push`` / ``push_detections`` append ``rotations``
        (slots, J, 4) float32, per slot and joint the unit quaternion (w, x, y, z) of the pose they return, behind what they return
        otherwise (with ``return_global`` the global quaternions behind that); ``rotation_flags`` is the (slots, J) uint8 table of the
        last tick.  uu3d_joint_rotations is the last launch of the captured tick.  With ``out_fps``: ValueError.
        ``views`` (keyword only, from ``options`` as well): None = every slot is a scene of its own (the session above, bit for bit: the
        same launches, buffers, refusals and bits).  Else V in [1, 8], the cameras of a calibrated rig: "Live several views"
        (``live_views.py``) -- ``slots`` = V N is VIEW-MAJOR, slot v N + i is person i in camera v, and ``camera`` is a list of V
        ``Camera`` objects with extrinsics, one per VIEW (all with distortion or all without).  uu3d_stream_views joins the launch table
        directly behind uu3d_camera_to_world; the filters and the rotations run behind it on N person rows.  ``push`` ->
        (poses (N, J, 3), fresh (N,), roots (N, 3), root_state (N,), view_count (N,) uint8, then ``rotations``); ``view_poses`` /
        ``view_roots`` are the per-slot world scene, ``raw_poses`` / ``raw_roots`` the unfiltered fused buffers.  ``reset(slots)`` resets a
        person iff all V of its slots are chosen.  With ``detections``, ``out_fps``, ``bones``: ValueError; ``finish``: ValueError."""
        (repair_joints, keypoints, camera, min_root_joints, smooth, bones, rotations, detections,
         *rule, views) = _live_options(options, "StreamSession", LIVE_OPTIONS + DETECTION_OPTIONS + VIEW_OPTIONS)
        res = self._init_plan(model, config, slots, resolutions, mask_stride, flip, lookahead, graph, missed_detections, fps, model_fps, out_fps,
                              repair_joints, keypoints, detections, dict(zip(ASSOCIATION_DEFAULTS, rule)), camera, min_root_joints, smooth,
                              bones=bones, root_relative=root_relative, rotations=rotations, interpolation=interpolation, views=views)
        import torch
        self._torch = torch
        self._lib = _capi.load_library()
        layouts = self._init_layout(config, root_relative)
        with torch.cuda.device(model.device):
            self._init_buffers(config, res, *layouts)
            self._init_launch_tables()
            self._zero_features()
            if self.detections is not None:                          # (a free slot's track id is -1, not 0)
                self._run([(fn, args + (None,)) for fn, args in self._reset_more[-1:]], torch.cuda.current_stream(model.device))
            if self.graph:
                self._capture()

    # ---- construction: checks and plan, layout and state, buffers, launch tables (then the capture) ---------------------------------
    def _init_plan(self, model, config, slots, resolutions, mask_stride, flip, lookahead, graph, missed_detections, fps, model_fps, out_fps,
                   repair_joints=None, keypoints=None, detections=None, rule=None, camera=None, min_root_joints=None, smooth=None, bones=None,
                   root_relative=True, rotations=None, interpolation="linear", views=None):
        """Every refusal that needs no device, and the session's plan.  -> the checked resolutions."""
        slots, lookahead = int(slots), int(lookahead)
        if slots < 1:
            raise ValueError("slots >= 1")
        # several views: the rig's own refusals, then ``camera`` is one Camera per slot, view-major, for everything below
        self.views = self.view_cameras = None
        if views is not None:
            self.views, self.view_cameras, camera = check_live_views(views, camera, slots, detections, out_fps, bones)
        # the refusals shared with ``predict_tracks`` (``options.stage_options``), then the ones only a session has
        opts = stage_options(config, slots, "slot", root_relative, keypoints, camera, min_root_joints, smooth, bones, repair_joints, fps, out_fps,
                             rotations=rotations)
        self.rotations = opts.rotations
        self.interpolation = check_interpolation(interpolation)
        if self.interpolation == "cubic" and fps is None:
            raise ValueError('interpolation="cubic" needs fps: a session without a frame rate holds the previous pose between keyframes, so there '
                             'is nothing to interpolate')
        self.bones, self.pose_filter, self.root_filter, self.keypoints = opts.rigid, opts.pose_filter, opts.root_filter, opts.keypoints
        self.cameras, self.min_root_joints = opts.cameras, opts.min_root_joints
        self.lens = opts.lens                                        # (slots, 10) rows of uu3d_undistort_points, or None: nothing to undistort
        self.world = opts.world                                      # (slots, 7) rows of uu3d_camera_to_world, or None: the scene stays in camera space
        self.smooth_rate = frame_rate(model_fps if fps is None else fps)     # the rate of the frames a push returns
        if self.bones is not None and out_fps is not None:
            raise ValueError("bones together with out_fps is not supported: a push then returns several rows per slot, and the live fix "
                             "rebuilds one pose per slot and push (multi-row emits are out of scope)")
        if (self.pose_filter is not None or self.root_filter is not None) and out_fps is not None:
            raise ValueError("smooth together with out_fps is not supported: a push then returns several rows per slot, and the live filter "
                             "takes one sample per slot and push (multi-row emits are out of scope)")
        if self.rotations is not None and out_fps is not None:
            raise ValueError("rotations together with out_fps is not supported: a push then returns several rows per slot, and the live "
                             "rotations are those of one pose per slot and push (multi-row emits are out of scope)")
        if camera is not None and out_fps is not None:
            raise ValueError("camera together with out_fps is not supported yet: the returned poses are not at source-frame times, so no "
                             "pushed frame is theirs to be solved against (a later change)")
        if camera is not None and detections is not None and np.ndim(plain_camera(camera)) != 1:
            raise ValueError("detections takes ONE camera (fx, fy, cx, cy), not one per slot: every person of a video shares one space")
        self.detections, self.association = None, None
        if detections is not None:
            rule = {k: (v if (rule or {}).get(k) is None else rule[k]) for k, v in ASSOCIATION_DEFAULTS.items()}
            joints = config.NUM_KEYPOINTS if self.keypoints is None else self.keypoints.inputs
            check_association(slots, detections, int(joints), **rule)
            if fps is not None or out_fps is not None:
                raise ValueError("detections together with fps / out_fps is not supported yet: the host mirror of the source counters cannot "
                                 "follow births that happen on the device")
            self.detections, self.association = int(detections), rule
        elif rule is not None and any(v is not None for v in rule.values()):
            raise ValueError("max_age / max_dist / min_common need detections=D: they are the parameters of the association")
        if repair_joints is not None and int(repair_joints) > MAX_LIVE_REPAIR:
            raise ValueError(f"repair_joints must be at most {MAX_LIVE_REPAIR} in a live session (the frames a tick re-stages and its buffers are "
                             f"fixed when the session is made), got {repair_joints}")
        if repair_joints is not None and (fps is not None or out_fps is not None):
            raise ValueError("repair_joints together with fps / out_fps is not supported yet: a revised source frame would re-make model frames "
                             "that were filed already")
        S, s_in, pred = session_strides(config, mask_stride)
        self.rate = None if fps is None else rate_plan(config, fps, lookahead, mask_stride, model_fps, out_fps, interpolation=self.interpolation)
        self.max_out = None if out_fps is None else self.rate.max_out
        if self.rate is None and not 0 <= lookahead <= max_lookahead(config):
            raise ValueError(f"lookahead must be in [0, {max_lookahead(config)}] = (SEQUENCE_LENGTH // 2) * SEQUENCE_STRIDE, got {lookahead}")
        res = check_resolutions(resolutions, slots, per="slot")
        if not getattr(model, "has_frames_form", model.arch.compiled_dims):
            raise NotImplementedError("StreamSession needs the frames form of the forward (uu3d_frame_features / uu3d_forward_frames_ex), "
                                      "which this model with generic dims does not have: one frame's spatial stack does not fit a workgroup's "
                                      "LDS (include/uu3d.h, FRAMES FORM)")
        J = int(getattr(model.arch, "num_keypoints", 17))
        if (bool(config.EVAL_FLIP) if flip is None else bool(flip)) and not model.arch.compiled_dims:
            order = np.asarray(config.AUGM_FLIP_KEYPOINT_ORDER).reshape(-1)
            if order.shape[0] != J or sorted(int(v) for v in order) != list(range(J)):
                raise ValueError(f"flip=True on a model with {J} keypoints: config.AUGM_FLIP_KEYPOINT_ORDER must be a permutation of range({J}), "
                                 f"got {order.shape[0]} entries")
        self.repair_joints = None if repair_joints is None else int(repair_joints)
        self.staged_frames = 1 if repair_joints is None else staged_frames(repair_joints, s_in)     # K: frames staged per slot and tick
        self.missed_detections = bool(missed_detections) or repair_joints is not None or detections is not None
        if self.missed_detections and not model.has_strided_input:
            raise ValueError("missed_detections needs a model with strided input: a missing frame becomes the learned masked token")
        self.model, self.slots, self.lookahead, self.graph = model, slots, lookahead, bool(graph)
        self.seq_stride, self.mask_stride, self.pred_stride = S, s_in, pred
        self.flip = bool(config.EVAL_FLIP) if flip is None else bool(flip)
        self.captures = 0                                             # hipGraph captures so far (graph=True: 1 for the session's whole life)
        self.model_lookahead = lookahead if self.rate is None else self.rate.a_m       # the lookahead of a (sub-)tick, in model frames
        self._key = ("stream", id(self))
        return res

    def _init_layout(self, config, root_relative):
        """The C structs of the session and the layouts of its state block -> (plain, rate, out), None where the session has no such part."""
        lib, h, r = self._lib, self.model._h, self.rate
        self._cfg = _capi.Uu3dStreamConfig(self.slots, self.seq_stride, self.mask_stride, self.pred_stride, self.model_lookahead, int(self.flip),
                                           int(config.PADDING_TYPE == "copy"), int(config.ROOT_KEYTPOINT) if root_relative else -1)
        self.model._sync_from_trainer()
        lay, rlay, olay = _capi.Uu3dStreamLayout(), None, None
        _capi.check(lib, lib.uu3d_stream_state_layout(h, C.byref(self._cfg), C.byref(lay)), h)
        self.ring_capacity = int(lay.ring_capacity)
        if r is not None:
            self._rate, rlay = _capi.Uu3dStreamRate(r.A, r.B, self.lookahead, r.D), _capi.Uu3dStreamRateLayout()
            _capi.check(lib, lib.uu3d_stream_rate_state_layout(h, C.byref(self._cfg), C.byref(self._rate), C.byref(rlay)), h)
        if self.max_out is not None:
            self._outp, olay = _capi.Uu3dStreamOut(r.out_c, r.out_d, r.pos_num, r.pos_den, r.max_out), _capi.Uu3dStreamOutLayout()
            _capi.check(lib, lib.uu3d_stream_out_state_layout(h, C.byref(self._cfg), C.byref(self._rate), C.byref(self._outp), C.byref(olay)), h)
        if self.detections is not None:
            K = config.NUM_KEYPOINTS if self.keypoints is None else self.keypoints.inputs
            a = self.association
            self._assoc = _capi.Uu3dAssociateParams(self.slots, self.detections, int(K), int(a["max_age"]), int(a["min_common"]), 0, float(a["max_dist"]))
        self._repair_bytes = 0
        if self.repair_joints is not None:
            play = _capi.Uu3dStreamRepairLayout()
            _capi.check(lib, lib.uu3d_stream_repair_layout(h, C.byref(self._cfg), self.repair_joints, C.byref(play)), h)
            if int(play.staged_frames) != self.staged_frames:
                raise AssertionError("the library and stream.staged_frames disagree")
            self._repair_bytes = int(play.bytes)
        return lay, rlay, olay

    def _init_buffers(self, config, res, lay, rlay, olay):
        """The state block and the buffers of a tick; what missed detections, the input-side options and the rates add; the output-side stages and their scenes."""
        torch, lib, m = self._torch, self._lib, self.model
        a, dev = m.arch, m.device
        T, J, N, dt, H, K = self.slots, a.num_keypoints, a.num_frames, a.d_temporal, 2 if self.flip else 1, self.staged_frames
        zeros = functools.partial(torch.zeros, device=dev)
        self._state = zeros(int((olay or rlay or lay).bytes), dtype=torch.uint8)
        view = lambda off, n, dtype: self._state[off:off + n * 4].view(dtype)
        self._frames = view(int(lay.frames_offset), T, torch.int32)
        self._table = view(int(lay.table_offset), int(lay.table_rows) * dt, torch.float32).view(int(lay.table_rows), dt)
        self._zero_row = int(lay.zero_row)
        self._kp = zeros((T, J, 2), dtype=torch.float32)
        self._kp_in = self._kp                                       # where push files the frame: with keypoints the detector's own layout
        if self.keypoints is not None:
            self._kp_in = zeros((T, self.keypoints.inputs, 2), dtype=torch.float32)
            self._map_table = self.keypoints.device_table(dev)
        self._push_in = self._kp_in                                  # where push copies the frame
        self._active = torch.ones((T,), dtype=torch.uint8, device=dev)
        self._active_all = True
        self._res = None if res is None else torch.from_numpy(res).pin_memory().to(dev, non_blocking=True)
        self._order = torch.from_numpy(np.ascontiguousarray(config.AUGM_FLIP_KEYPOINT_ORDER, np.int32)).to(dev) if self.flip else None
        self._staged = zeros((H * T * K, J, 2), dtype=torch.float32)   # (K = 1 without repair_joints)
        self._feats = zeros((H * T * K, dt), dtype=torch.float32)
        self._rows = torch.full((H * T, N), -1, dtype=torch.int32, device=dev)
        self._mask = zeros((H * T, N), dtype=torch.uint8)
        self._fresh = zeros((T,), dtype=torch.uint8)
        self._full = torch.empty((H * T, N, J, 3), dtype=torch.float32, device=dev) if m._returns_full else None
        self._central = zeros((H * T, J, 3), dtype=torch.float32)
        self._out = zeros((T, J, 3), dtype=torch.float32)
        # a workspace of the session's own for uu3d_frame_features: the graph holds its address
        self._fws = torch.empty(max(int(lib.uu3d_frame_features_bytes(m._h, H * T * K)), int(lib.uu3d_frame_features_bytes(m._h, 1))),
                                dtype=torch.uint8, device=dev)
        # missed detections: the caller's flags of this tick, the same ANDed with active and the finite test (stage), the flags kept per slot
        self._valid_in = self._valid = self._valid_state = None
        self._valid_in_all = True
        if self.missed_detections:
            self._valid_in = torch.ones((T, J) if self.repair_joints is not None else (T,), dtype=torch.uint8, device=dev)
            self._valid = zeros((T,), dtype=torch.uint8)
            self._valid_state = zeros(int(lib.uu3d_stream_valid_bytes(m._h, C.byref(self._cfg))), dtype=torch.uint8)
        # repair_joints: the repair state, what the stage hands to the commit (frames staged, their flags, the far list), the joint states
        if self.repair_joints is not None:
            G = self.repair_joints
            self._repair_state = zeros(self._repair_bytes, dtype=torch.uint8)
            self._stage_frame = torch.full((T, K), -1, dtype=torch.int32, device=dev)
            self._stage_valid = zeros((T, K), dtype=torch.uint8)
            self._far = torch.full((T, G), -1, dtype=torch.int32, device=dev)
            self._joint_state = zeros((T, J), dtype=torch.uint8)
        # where push files its flags: with keypoints and repair_joints one per DETECTOR joint, mapped onto _valid_in by the tick's first launch
        self._flags_in = self._valid_in
        if self.keypoints is not None and self.repair_joints is not None:
            self._flags_in = torch.ones((T, self.keypoints.inputs), dtype=torch.uint8, device=dev)
        # per-frame detections: what push_detections files (the frame's list, its count, one flag per detector joint), the association state
        # and what the tick's first launch writes beside the frame, flag and active buffers above
        if self.detections is not None:
            D, Kd = self.detections, int(self._kp_in.shape[1])
            self._dets = zeros((D, Kd, 2), dtype=torch.float32)
            self._det_count = torch.full((1,), D, dtype=torch.int32, device=dev)
            self._det_flags = torch.ones((D, Kd), dtype=torch.uint8, device=dev)
            self._det_count_full = self._det_flags_all = True
            self._assoc_state = zeros(int(lib.uu3d_associate_state_bytes(T, Kd)), dtype=torch.uint8)
            self._born = zeros((T,), dtype=torch.uint8)
            self._assignment = torch.full((D,), -1, dtype=torch.int32, device=dev)
            self._track_ids = torch.full((T,), -1, dtype=torch.int32, device=dev)
            self._dropped = zeros((1,), dtype=torch.int32)
            self._dets_in = self._dets                                # where push_detections copies the frame's list
        # lens distortion: push files the raw points in a buffer of their own; the tick's first launch writes the undistorted ones where
        # push filed them otherwise -- per slot its own camera, with detections the one camera for all D x K points
        if self.lens is not None:
            self._lens = torch.from_numpy(np.ascontiguousarray(self.lens)).pin_memory().to(dev, non_blocking=True)
            if self.detections is not None:
                self._dets_in, self._lens_track = torch.zeros_like(self._dets), None
            else:
                self._push_in, self._lens_track = torch.zeros_like(self._kp_in), torch.arange(T, dtype=torch.int32, device=dev)
        # what a (sub-)tick takes as `active` and where its emit writes: with a rate the sub-ticks' own buffers, else the session's
        self._tick_active, self._emit_out, self._emit_fresh = self._active, self._out, self._fresh
        self._source_frames, self._src_host, self._src_known = self._frames, None, None
        if rlay is not None:
            self._source_frames = view(int(rlay.source_frames_offset), T, torch.int32)
            self._tick_active = zeros((T,), dtype=torch.uint8)
            self._emit_out = zeros((T, J, 3), dtype=torch.float32)
            self._emit_fresh = zeros((T,), dtype=torch.uint8)
            self._src_host = np.zeros(T, np.int64)                    # host mirror of the source counters; exact where _src_known
            self._src_known = np.ones(T, bool)
        if olay is not None:                                         # (a case of its own: every output-side option is refused with it)
            self._out_frames = view(int(olay.out_frames_offset), T, torch.int32)
            self._poses = zeros((T, self.max_out, J, 3), dtype=torch.float32)
            self._count = zeros((T,), dtype=torch.int32)
            self._result = self._poses, self._count                   # what push returns: the session's own buffers
        # the output-side options in the one order a tick runs them, each under the scene it leaves: ``push`` returns the last one
        # (with ``views`` the stages behind the fusion have one row per PERSON)
        live = lambda option, make, *args, rows=T, **field: None if option is None else make(rows, *args, device=dev, **field)
        P = T // (self.views or 1)
        self._pose_smoother = live(self.pose_filter, LiveOneEuro, 3 * J, self.smooth_rate, self.pose_filter, self.lookahead, rows=P)
        self._root_smoother = live(self.root_filter, LiveOneEuro, 3, self.smooth_rate, self.root_filter, self.lookahead, rows=P, field="roots")
        root = live(self.cameras, LiveRoot, J, self.lookahead, self.cameras, self.min_root_joints, self._kp, self._valid_in)
        self._stages = [("fixed", live(self.bones, LiveBones, J, *(self.bones or ()))), ("camera", root),
                        ("world", live(self.world, LiveWorld, J, self.world)), ("fused", live(self.views, LiveViews, J, self.views, root, self.view_cameras)),
                        ("shown", self._pose_smoother), ("shown", self._root_smoother),
                        ("shown", live(self.rotations, LiveRotations, J, self.rotations, rows=P))]
        self._post = [stage for _, stage in self._stages if stage is not None]
        if olay is None:
            self._scenes = scenes(Scene(self._out, self._fresh, None, None, ()), self._stages)
            self._result = self._scenes["shown"].as_result()
        # the end of a track: nothing until the first ``finish`` (_init_drain)
        self._drain_result = self._drain_state = self._drain_graph = None
        self._drain_steps = []

    def _init_launch_tables(self):
        """All arguments are the same at every push (the buffers never move), so the mode is decided here, once: every launch of the
        session as (library function, its arguments up to the stream); a step whose arguments are None is a Python callable of the stream.
          _tick_steps   the steps of one (sub-)tick, in order -- what the graph captures
          _push_before  / _push_after   the launches of a push around its sub-ticks (a session with a rate; not captured)
          _reset_call   the reset of the session's kind; the slot mask and the stream follow its arguments (_reset_more: what a session
                        with repair_joints, output-side stages, detections or a drain resets beside it; _reset_persons: with ``views`` the
                        stages behind the fusion, whose rows are persons -- they take the mask of the persons all of whose slots are chosen)
          _drain_steps  the steps of one drain tick (``finish``), built at the first ``finish`` by _init_drain -- a second captured graph; the output-side stages (``_post``) give their own entries"""
        lib, m = self._lib, self.model
        h, cfg, state = m._h, C.byref(self._cfg), _ptr(self._state)
        kp, res, order, active, staged = _ptr(self._kp), _ptr(self._res), _ptr(self._order), _ptr(self._active), _ptr(self._staged)
        tick_active, valid, feats, rows, mask = _ptr(self._tick_active), _ptr(self._valid), _ptr(self._feats), _ptr(self._rows), _ptr(self._mask)
        emit_fresh = _ptr(self._emit_fresh)
        if self.rate is not None:
            rate = C.byref(self._rate)
            stage = (lib.uu3d_stream_resample_stage, (h, cfg, rate, state, res, order, tick_active, valid, staged))
        elif self.repair_joints is not None:
            G, handed = self.repair_joints, (_ptr(self._stage_frame), _ptr(self._stage_valid), _ptr(self._far))
            stage = (lib.uu3d_stream_repair_stage, (h, cfg, G, state, _ptr(self._repair_state), kp, res, active, order, _ptr(self._valid_in), staged)
                     + handed + (_ptr(self._joint_state),))
        elif self.missed_detections:
            stage = (lib.uu3d_stream_stage_valid, (h, cfg, kp, res, active, order, _ptr(self._valid_in), valid, staged))
        else:
            stage = (lib.uu3d_stream_stage, (h, cfg, kp, res, active, order, staged))
        features = (lib.uu3d_frame_features, (h, staged, int(self._staged.shape[0]), feats, _ptr(self._fws), C.c_size_t(self._fws.numel()), 0))
        if self.repair_joints is not None:
            commit = (lib.uu3d_stream_commit_repair, (h, cfg, G, state, feats, tick_active) + handed + (_ptr(self._valid_state), rows, mask, emit_fresh))
        elif self.missed_detections:
            commit = (lib.uu3d_stream_commit_valid, (h, cfg, state, feats, tick_active, valid, _ptr(self._valid_state), rows, mask, emit_fresh))
        else:
            commit = (lib.uu3d_stream_commit, (h, cfg, state, feats, tick_active, rows, mask, emit_fresh))
        # the latency schedule: what model.forward_frames takes (below 1024 token rows both schedules give the same bits)
        forward = (functools.partial(m._forward_frames, self._table, self._rows, self._mask if m.has_strided_input else None, self._full,
                                     self._central, self._key), None)
        emit = (lib.uu3d_stream_emit, (h, cfg, state, _ptr(self._central), order, emit_fresh, _ptr(self._emit_out)))
        self._tick_steps = [stage, features, commit, forward, emit]
        self._drain_shared = [forward, emit]                         # what a drain tick takes from the tick as it is (_init_drain)
        self._push_before, self._push_after = [], []
        # any skeleton: the detector's joints -> the session's own frame (with repair_joints: and its joint flags), in front of everything
        mapping = []
        if self.keypoints is not None:
            per_joint = self.repair_joints is not None
            mapping = [(lib.uu3d_map_keypoints, (h, _ptr(self._map_table), self.keypoints.inputs, _ptr(self._kp_in),
                                                 _ptr(self._flags_in) if per_joint else None, self.slots, kp,
                                                 _ptr(self._valid_in) if per_joint else None))]
        # lens distortion: the raw points as pushed -> the pinhole's pixels, in front of the map (and of the source push, and of the association)
        lens = []
        if self.lens is not None:
            raw, to = (self._push_in, self._kp_in) if self.detections is None else (self._dets_in, self._dets)
            lens = [(lib.uu3d_undistort_points, (_ptr(raw), _ptr(to), int(raw.shape[0]), int(raw.shape[1]), _ptr(self._lens_track),
                                                 self.slots if self.detections is None else 1, _ptr(self._lens)))]
        if self.rate is None:
            self._tick_steps = (lens if self.detections is None else []) + mapping + self._tick_steps
        self._reset_call = (lib.uu3d_stream_reset, (h, cfg, state))
        # the resets beside it: repair, then the stages in the order the options joined the session, which tests pin (each clears a block of its own; world has none)
        self._reset_more = [] if self.repair_joints is None else [(lib.uu3d_stream_repair_reset, (h, cfg, self.repair_joints, _ptr(self._repair_state)))]
        bones, root, _, fused, pose_filter, root_filter, rotations = (stage for _, stage in self._stages)
        behind = [stage.reset_launch() for stage in (pose_filter, root_filter, bones, rotations) if stage is not None]
        self._reset_more += [stage.reset_launch() for stage in (root, fused) if stage is not None] + ([] if fused is not None else behind)
        self._reset_persons = behind if fused is not None else []
        # per-frame detections: the association in front of everything -- it writes the frame, the flags, `active` and the born mask --, then
        # the resets of the slots born at this tick, with the mask on the device
        if self.detections is not None:
            assoc, born = C.byref(self._assoc), _ptr(self._born)
            front = [(lib.uu3d_stream_associate, (assoc, _ptr(self._assoc_state), _ptr(self._dets), _ptr(self._det_count), _ptr(self._det_flags), 1,
                                                  _ptr(self._kp_in), _ptr(self._flags_in), int(self._flags_in.dim() == 2), active, born,
                                                  _ptr(self._assignment), _ptr(self._track_ids), _ptr(self._dropped)))]
            front += [(fn, args + (born,)) for fn, args in [self._reset_call] + self._reset_more]
            self._tick_steps = lens + front + self._tick_steps
            self._reset_more = self._reset_more + [(lib.uu3d_associate_reset, (assoc, _ptr(self._assoc_state)))]
        if self.rate is not None:
            self._tick_steps.append((lib.uu3d_stream_file_keyframe, (h, cfg, rate, state, emit_fresh)))
            self._push_before = lens + mapping + [(lib.uu3d_stream_source_push, (h, cfg, rate, state, kp, active, _ptr(self._valid_in), int(self.missed_detections)))]
            cubic = self.interpolation == "cubic"                   # the C1 cubic through four kept keyframes: the emit's cubic sibling
            self._push_after = [(lib.uu3d_stream_timed_emit_cubic if cubic else lib.uu3d_stream_timed_emit,
                                 (h, cfg, rate, state, _ptr(self._out), _ptr(self._fresh)))]
            self._reset_call = (lib.uu3d_stream_rate_reset, (h, cfg, rate, state))
        if self.max_out is not None:
            outp = C.byref(self._outp)
            self._push_after = [(lib.uu3d_stream_timed_emit_multi_cubic if cubic else lib.uu3d_stream_timed_emit_multi,
                                 (h, cfg, rate, outp, state, _ptr(self._poses), _ptr(self._count)))]
            self._reset_call = (lib.uu3d_stream_out_reset, (h, cfg, rate, outp, state))
        # the output-side stages behind the emit that wrote the pose they read (with a rate: the timed emit), in the tick's order
        last = self._tick_steps if self.rate is None else self._push_after
        active, frames = self._active, self._source_frames
        for stage in self._post:
            last.append(stage.launch(active, frames))
            if isinstance(stage, LiveViews):                         # behind the fusion a row is a person: its own counter and flag
                active, frames = stage.active, stage.frames

    # ---- the steps of a tick, on ``stream`` ------------------------------------------------------------------------------------------
    def _run(self, steps, stream):
        """Enqueue the steps of a launch table on ``stream``, in order."""
        st = C.c_void_p(stream.cuda_stream)
        for fn, args in steps:
            if args is None:
                fn(stream)
            else:
                _capi.check(self._lib, fn(*args, st), self.model._h)

    def _zero_features(self):
        """The features of an all-zero frame (zero padding) into the table's zero row."""
        torch, lib, m = self._torch, self._lib, self.model
        zero = torch.zeros((1,) + tuple(self._kp.shape[1:]), dtype=torch.float32, device=m.device)
        self._run([(lib.uu3d_frame_features, (m._h, _ptr(zero), 1, _ptr(self._table[self._zero_row:]), _ptr(self._fws),
                                              C.c_size_t(self._fws.numel()), 0))], torch.cuda.current_stream(m.device))

    def _capture_steps(self, steps, warm):
        """``warm(side)``, a warm-up run in which nothing advances, on a side stream, then the capture of ``steps``: a linear chain on it -> the graph."""
        torch = self._torch
        dev = self.model.device
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        gc.collect()                                                  # (a collection inside a capture may free device memory: pipeline.py)
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.stream(side):
                warm(side)
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                self._run(steps, side)
            self.captures += 1
        finally:
            if gc_was_on:
                gc.enable()
        torch.cuda.current_stream(dev).wait_stream(side)
        return g

    def _capture(self):
        """The tick's graph; the warm-up tick has every slot inactive."""
        def warm(side):
            self._active.zero_()
            if self.detections is not None:                          # (no detection, no slot alive: the association changes nothing either)
                self._det_count.zero_()
                self._det_count_full = False
            self._run(self._tick_steps, side)
            self._active.fill_(1)
        self._graph = self._capture_steps(self._tick_steps, warm)
        self.reset()

    # ---- public ---------------------------------------------------------------------------------------------------------------------
    def _flags(self, flags, name, joints=None, rows=None):
        """(rows,) flags from the host or the device (``rows``: None = slots) -> a uint8 tensor, pinned when it is on the host.  ``joints`` = J:
        (rows, J) passes as well and (rows,) comes back as (rows, 1) -- one flag for all joints of a row, for a copy that broadcasts on the device."""
        torch = self._torch
        n = self.slots if rows is None else rows
        if isinstance(flags, torch.Tensor):
            f = flags.to(torch.uint8) if flags.dtype != torch.bool else flags.view(torch.uint8)
        else:
            f = torch.from_numpy(np.ascontiguousarray(np.asarray(flags) != 0).view(np.uint8))
        if tuple(f.shape) != (n,) and (joints is None or tuple(f.shape) != (n, joints)):
            raise ValueError(f"{name} must be ({n},)" + ("" if joints is None else f" or ({n}, {joints})"))
        if joints is not None and f.dim() == 1:
            f = f.reshape(n, 1) if f.is_cuda else f.reshape(n, 1).repeat(1, joints)
        return f if f.is_cuda else f.contiguous().pin_memory()

    def _sync_weights(self):
        """Weights changed since the last tick: the packs are rewritten on this stream, and the zero row's features with them."""
        m = self.model
        if m._weights_dirty or getattr(m, "_pending_assigns", False):
            m._sync_from_trainer()
            with self._torch.cuda.device(m.device):
                self._zero_features()

    def _host_frame(self, x, like, name):
        """What a push files, checked against the buffer ``like`` -> a tensor to copy from: host input goes through pinned memory."""
        torch = self._torch
        if not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.ascontiguousarray(x, np.float32))
        if tuple(x.shape) != tuple(like.shape):
            raise ValueError(f"{name} must be {tuple(like.shape)}, got {tuple(x.shape)}")
        return x if x.is_cuda else x.to(torch.float32).contiguous().pin_memory()

    def push(self, kp2d, active=None, valid=None):
        """One tick: ``kp2d`` (slots, J, 2) -- (slots, K_in, 2) in a session with ``keypoints`` --, a host array or a tensor on the host or the device; ``active`` (slots,) bools or None = every slot
        (an inactive slot's row of ``kp2d`` is ignored and its track does not grow).  -> (poses (slots, J, 3) float32, fresh (slots,) bool)
        on the device: the session's own buffers, valid until the next ``push``.  ``fresh[i]``: slot i's pose is new at this tick -- the
        pose of its frame ``frames[i] - 1 - lookahead``; otherwise ``poses[i]`` is the slot's previous pose (zeros before its first).
        ``valid`` (slots,) flags or None (sessions built with ``missed_detections=True`` only): 0 = slot i's frame of this tick is MISSING, as
        is a row of ``kp2d`` with a NaN or Inf coordinate.  The slot's track grows by the frame all the same (``frames`` counts it; with
        ``active[i] == 0`` it would not) and a pose comes out by the usual rule, from windows that never read the missing frame.
        A session with ``repair_joints``: ``valid`` may also be (slots, J), one flag per joint, ANDed with the finite test per joint; a
        joint that is not observed is filled by the rule where it can be, and only a frame with a joint that cannot is missing.
        A session with ``keypoints``: the per-joint form is (slots, K_in), one flag per DETECTOR joint, and a model joint is observed iff
        every one of its sources is flagged and finite; (slots,) flags stand for all joints of a slot as before.
        A session with ``fps``: ``kp2d`` holds one SOURCE frame per slot; ``poses[i]`` is the pose of slot i's source frame
        ``source_frames[i] - 1 - lookahead`` and ``fresh[i]`` is set at every push of an active slot once that index is >= 0.  The push
        enqueues uu3d_stream_source_push, n replays of the one sub-tick graph and uu3d_stream_timed_emit; n is the largest number of model
        frames an active slot makes at this push, known from a host mirror of the source counters.  ``active`` as a DEVICE tensor leaves the
        mirror unknown: ceil(A / B) sub-ticks are replayed per push (the surplus ones change nothing) until every such slot has been reset.
        A session with ``out_fps``: -> (poses (slots, max_out, J, 3) float32, count (slots,) int32) on the device, the session's own buffers,
        valid until the next ``push``: rows r < count[i] of slot i are the output frames that became due at this push, oldest first (the
        first is output frame ``out_frames[i] - count[i]``), rows r >= count[i] are zeros; an inactive slot has count 0.
        uu3d_stream_timed_emit_multi takes uu3d_stream_timed_emit's place.
        A session with ``interpolation="cubic"``: the same returns, read from the C1 cubic through the keyframes;
        uu3d_stream_timed_emit_cubic / uu3d_stream_timed_emit_multi_cubic take the emit's place, still a plain launch.
        A session with ``camera``: -> (poses, fresh, roots (slots, 3) float32, root_state (slots,) uint8), the session's own buffers as
        well: ``poses[i] + roots[i]`` stands in the camera's space; ``root_state[i]``: 1 solved at this push, 2 the slot's last solved
        root is held, 0 no frame of the slot was solved yet (zeros).  A slot that is not fresh returns its previous root and state.
        A session with ``smooth``: the same tuple with the filtered buffers in place of ``poses`` and, with a root filter, of ``roots``.
        Enqueues on the current stream and returns; never waits for the device."""
        torch = self._torch
        dev = self.model.device
        if getattr(self, "detections", None) is not None:
            raise ValueError("a session built with detections=D takes push_detections(dets, count, valid): the device decides which slot a person is")
        if valid is not None and not self.missed_detections:
            raise ValueError("push(valid=...) needs a session built with missed_detections=True")
        self._sync_weights()
        with torch.cuda.device(dev):
            self._push_in.copy_(self._host_frame(kp2d, self._kp_in, "kp2d"), non_blocking=True)
            if active is None:
                if not self._active_all:
                    self._active.fill_(1)
                    self._active_all = True
            else:
                self._active.copy_(self._flags(active, "active"), non_blocking=True)
                self._active_all = False
            if valid is not None:
                self._flags_in.copy_(self._flags(valid, "valid", None if self.repair_joints is None else self._kp_in.shape[1]), non_blocking=True)
                self._valid_in_all = False
            elif not self._valid_in_all:
                self._flags_in.fill_(1)
                self._valid_in_all = True
            cur = torch.cuda.current_stream(dev)
            self._run(self._push_before, cur)                         # (with a rate: file the source frames)
            for _ in range(self._sub_ticks(active)):                  # make the model frames that are due
                if self.graph:
                    self._graph.replay()
                else:
                    self._run(self._tick_steps, cur)
            self._run(self._push_after, cur)                          # (with a rate: read the poses)
        return self._result

    def push_detections(self, dets, count=None, valid=None):
        """One tick of a session built with ``detections=D``: ``dets`` (D, K, 2) -- the people the detector listed for this frame, in any
        order, in its own joint layout --, a host array or a tensor on the host or the device; ``count``: how many rows are given -- an int,
        an int32 tensor (a DEVICE tensor is never read on the host) or None = D; ``valid``: None, (D,) flags, one per detection, or
        (D, K), one per joint (``scores >= 0.3``).  uu3d_stream_associate matches the people to slots on the device; then the tick of
        ``push``.  -> (poses (slots, J, 3) float32, fresh (slots,) bool) as ``push``: row i belongs to the track in slot i,
        ``track_ids[i]``.  In a session without ``repair_joints`` a detection with a joint flag that is not set gives a MISSING frame (as
        a (T_i, J) entry of ``predict_tracks``' ``valid`` does); with it the joint is filled by the rule.  A session with ``camera``
        appends (roots, root_state) as ``push`` does.  Enqueues on the current stream
        and returns; never waits for the device."""
        torch = self._torch
        dev = self.model.device
        if getattr(self, "detections", None) is None:
            raise ValueError("push_detections needs a session built with detections=D")
        self._sync_weights()
        D, K = self._det_flags.shape
        with torch.cuda.device(dev):
            dets = self._host_frame(dets, self._dets, "dets")
            if valid is not None:                                     # ((D, 1) broadcasts over the joints in the copy, on the device)
                valid = self._flags(valid, "valid", int(K), int(D))
            self._dets_in.copy_(dets, non_blocking=True)
            if count is None:
                if not self._det_count_full:
                    self._det_count.fill_(int(D))
                    self._det_count_full = True
            else:
                if isinstance(count, torch.Tensor):
                    self._det_count.copy_(count.reshape(1), non_blocking=True)
                else:
                    self._det_count.fill_(min(max(int(count), 0), int(D)))
                self._det_count_full = False
            if valid is not None:
                self._det_flags.copy_(valid, non_blocking=True)
                self._det_flags_all = False
            elif not self._det_flags_all:
                self._det_flags.fill_(1)
                self._det_flags_all = True
            if self.graph:
                self._graph.replay()
            else:
                self._run(self._tick_steps, torch.cuda.current_stream(dev))
        return self._result

    def _sub_ticks(self, active):
        """How many (sub-)ticks this push needs, advancing the host mirror of the source counters (no rate: none, and one tick per push)."""
        if self._src_host is None:
            return 1
        torch = self._torch
        r = self.rate
        if isinstance(active, torch.Tensor) and active.is_cuda:
            self._src_known[:] = False
            return r.n_max
        act = np.ones(self.slots, bool) if active is None else np.asarray(active.numpy() if isinstance(active, torch.Tensor) else active) != 0
        n = r.n_max if (act & ~self._src_known).any() else 0
        for i in np.flatnonzero(act & self._src_known):
            j = int(self._src_host[i])
            n = max(n, 1 if j == 0 else newest_model_frame(j, r.A, r.B) - newest_model_frame(j - 1, r.A, r.B))
            self._src_host[i] = j + 1
        return n

    def reset(self, slots=None):
        """The given slots (indices; None = all) start a new track: zero frames, held pose 0, with ``out_fps`` output counter 0, with
        ``repair_joints`` no observation of any joint, with ``camera`` no filed frame, no held root and root state 0, with ``smooth`` no
        sample taken.  A session with ``detections``: the tracks in those slots END and the slots are
        free (the next unmatched person takes the lowest one, under a new id); None also sets the id and dropped counters back to 0.
        Stream-ordered like ``push``."""
        torch = self._torch
        m = self.model
        mask = None
        with torch.cuda.device(m.device):
            if slots is not None:
                h = np.zeros(self.slots, np.uint8)
                h[np.asarray(slots, np.int64).reshape(-1)] = 1
                mask = torch.from_numpy(h).pin_memory().to(m.device, non_blocking=True)
            self._run([(fn, args + (_ptr(mask),)) for fn, args in [self._reset_call] + self._reset_more], torch.cuda.current_stream(m.device))
            if self._reset_persons:                                   # (several views: a person is reset iff all of its slots are)
                persons = person_mask(slots, self.views, self.slots)
                pmask = None if persons is None else torch.from_numpy(persons).pin_memory().to(m.device, non_blocking=True)
                self._run([(fn, args + (_ptr(pmask),)) for fn, args in self._reset_persons], torch.cuda.current_stream(m.device))
            if self.detections is not None:                          # (what the properties show until the next tick)
                if mask is None:
                    self._track_ids.fill_(-1)
                    self._dropped.zero_()
                else:
                    self._track_ids.masked_fill_(mask.view(torch.bool), -1)
        self._mirror_reset(slots)

    def _mirror_reset(self, slots):
        """The host mirror of the source counters after a reset: the chosen slots are at zero, and known to be."""
        if self._src_host is None:
            return
        which = slice(None) if slots is None else np.asarray(slots, np.int64).reshape(-1)
        self._src_host[which] = 0
        self._src_known[which] = True

    # ---- the end of a track: the drain ticks of ``finish`` ----------------------------------------------------------------------------
    def _init_drain(self):
        """What ``finish`` needs, made at its first call: the result buffers (one block, so that one fill zeroes them: the raw scene's rows
        and every stage's), and with lookahead >= 1 the drain state, the chosen-slots mask, the launch table of a drain tick (the drain
        commit, the tick's forward and emit, every stage's launch, the filing) and its captured graph."""
        torch, lib, m = self._torch, self._lib, self.model
        dev, T, a, J = m.device, self.slots, self.lookahead, int(self._kp.shape[1])
        # (name, tick buffer or None for a byte buffer, shape of a row, dtype)
        parts = [("poses", self._out, (J, 3), torch.float32), ("fresh", None, (), torch.uint8)]
        # (the stages' rows follow in the tick's order, a byte buffer as None; until the stages were objects the roots came before fixed_poses)
        parts += [(row, None if b.dtype == torch.uint8 else b, tuple(b.shape[1:]), b.dtype) for stage in self._post for _, row, b in stage.outputs]
        nbytes = [T * a * int(np.prod(shape, dtype=np.int64)) * (4 if dt == torch.float32 else 1) for _, _, shape, dt in parts]
        offsets = [int(o) for o in np.cumsum([0] + [(n + 255) // 256 * 256 for n in nbytes])]
        self._drain_rows = torch.zeros(max(offsets[-1], 1), dtype=torch.uint8, device=dev)
        rows = {}
        for (name, _, shape, dt), off, n in zip(parts, offsets, nbytes):
            rows[name] = (self._drain_rows[off:off + n].view(dt).view((T, a) + shape) if a > 0 else
                          torch.zeros((T, 0) + shape, dtype=dt, device=dev))
        self._drain_named = rows
        self._drain_result = scenes(Scene(rows["poses"], rows["fresh"], None, None, ()), self._stages, rows)["shown"].as_result()
        if a == 0:
            return
        lay = _capi.Uu3dStreamDrainLayout()
        _capi.check(lib, lib.uu3d_stream_drain_layout(T, C.byref(lay)), None)
        self._drain_state = torch.zeros(int(lay.bytes), dtype=torch.uint8, device=dev)
        self._drained = self._drain_state[int(lay.drained_offset):int(lay.drained_offset) + 4 * T].view(torch.int32)
        self._virtual_frames = self._drain_state[int(lay.virtual_frames_offset):int(lay.virtual_frames_offset) + 4 * T].view(torch.int32)
        self._drain_mask = torch.zeros((T,), dtype=torch.uint8, device=dev)
        h, cfg, dstate, chosen, fresh = m._h, C.byref(self._cfg), _ptr(self._drain_state), _ptr(self._drain_mask), _ptr(self._fresh)
        steps = [(lib.uu3d_stream_drain_commit, (h, cfg, _ptr(self._state), dstate, chosen, _ptr(self._valid_state), _ptr(self._rows),
                                                 _ptr(self._mask), _ptr(self._emit_fresh)))] + self._drain_shared
        # the stages' launches of a drain tick: the chosen slots as `active`, the virtual counter as the frames, the root from the ring
        steps += [stage.launch(self._drain_mask, self._virtual_frames, self._drain_state) for stage in self._post]
        floats = [(src, rows[name], int(np.prod(shape))) for name, src, shape, _ in parts if src is not None]
        self._drain_file_args = []                                    # (uu3d_stream_drain_file takes four float buffers: a fifth goes in a launch of its own)
        for first in range(0, len(floats), 4):
            group = floats[first:first + 4]
            n = len(group)
            src, widths, dst = ((C.c_void_p * n)(*[t.data_ptr() for t, _, _ in group]), (C.c_int32 * n)(*[w for _, _, w in group]),
                                (C.c_void_p * n)(*[t.data_ptr() for _, t, _ in group]))
            self._drain_file_args.append((src, widths, dst))
            bytes_too = self.cameras is not None and first == 0
            steps.append((lib.uu3d_stream_drain_file, (T, a, dstate, n, src, widths, dst, fresh, _ptr(rows["fresh"]),
                                                       *((_ptr(self._scenes["camera"].root_state), _ptr(rows["root_state"])) if bytes_too else (None, None)))))
        self._drain_steps = steps
        # (every slot's `drained` is 0 outside ``finish`` -- it resets the slots it drained --, so the captured tick of a session with
        # detections, which resets the slots born on the device, needs no launch for the drain state; ``reset`` zeroes it all the same)
        self._reset_more = self._reset_more + [(lib.uu3d_stream_drain_reset, (T, dstate))]
        if self.graph:                                               # (the warm-up drain tick has no slot chosen: nothing advances)
            def warm(side):
                self._drain_mask.zero_()
                self._run(self._drain_steps, side)
            self._drain_graph = self._capture_steps(self._drain_steps, warm)

    def finish(self, slots=None):
        """The tracks in the given slots (indices; None = all) have ENDED: the poses of their last ``lookahead`` frames, which no push
        returned, and then ``reset`` for exactly those slots.  -> (poses (slots, a, J, 3) float32, fresh (slots, a) bool) on the device, a =
        ``lookahead``: buffers of the session, allocated at the first call and valid until the next ``finish``.  For a chosen slot with
        ``len`` frames row k - 1 (k = 1 .. a) holds the pose of frame c = len - 1 - a + k, ``fresh`` set iff c >= 0 and c is a multiple of
        the prediction stride; a row that is not fresh holds the slot's previous pose, as a push does.  Rows of slots that were not chosen
        are zeros with ``fresh`` 0.  The one rule, extended: row k - 1 is the pose ``predict.predict_tracks`` gives for frame c of the WHOLE
        track (same ``mask_stride``, ``flip``, ``resolutions``, ``root_relative``, ``valid``, ``repair_joints``, ``keypoints``) -- the
        frames behind the track's end are padded as the end of a video is --, and the pose a session of the same shape with lookahead
        a - k, pushed the same frames, returns at its last push.
        A session with ``camera``: roots (slots, a, 3) float32 and root_state (slots, a) uint8 are appended, by ``push``'s rule at frame c
        (``LiveRootHost.drain``).  A session with ``smooth``: the filtered rows stand in place of poses and roots (one sample per fresh
        row, at frame c: ``LiveOneEuroHost.drain``); ``drain_raw_poses`` / ``drain_raw_roots`` are the unfiltered rows.  A session with
        ``bones``: every drain tick rebuilds its pose between the emit and the root solve as a push does, the chosen slots as ``active``
        (``LiveBonesHost.drain``: a fresh drained pose joins the running mean of a "track" session); the rows are the rebuilt poses, roots
        and filters read them, and ``drain_raw_poses`` stays the model's output.
        Slots that were not chosen are untouched -- counters, rings, held pose, held root and filter state keep their bits -- and the next
        ``push`` continues their tracks; but the buffers the previous ``push`` returned are no longer meaningful after ``finish`` (the
        drain ticks write them).  A session with ``detections``: the tracks end as ``reset`` ends them (ids freed; None also zeroes the
        counters).  ``lookahead == 0``: empty second dimensions, only the reset is launched.  A session with ``fps`` / ``out_fps``:
        ValueError (a later change: its drain needs the end of the model-rate track).
        Enqueues a drain ticks (uu3d_stream_drain_commit, the tick's own forward and emit, uu3d_stream_root_drain, the filters,
        uu3d_stream_drain_file: no stage, no uu3d_frame_features; with ``graph`` ONE more captured graph, replayed a times) and the reset on
        the current stream.  The first ``finish`` of a session allocates and captures (``captures`` goes from 1 to 2 and stays), and so
        waits for the device once; every later one never waits."""
        if self.rate is not None:
            raise ValueError("finish in a session with fps / out_fps is not supported yet (a later change): the drain of a source-rate session "
                             "needs the end of the model-rate track")
        if self.views is not None:
            raise ValueError("finish in a session with views is not supported yet (a later change): the drain ticks of a person's V slots "
                             "would have to be fused as its pushes are")
        torch = self._torch
        m = self.model
        dev = m.device
        chosen = None
        if slots is not None:
            chosen = np.zeros(self.slots, np.uint8)
            chosen[np.asarray(slots, np.int64).reshape(-1)] = 1
        with torch.cuda.device(dev):
            self._sync_weights()
            if self._drain_result is None:
                self._init_drain()
            if self.lookahead > 0:
                if chosen is None:
                    self._drain_mask.fill_(1)
                else:
                    self._drain_mask.copy_(torch.from_numpy(chosen).pin_memory(), non_blocking=True)
                self._drain_rows.zero_()
                cur = torch.cuda.current_stream(dev)
                for _ in range(self.lookahead):
                    if self.graph:
                        self._drain_graph.replay()
                    else:
                        self._run(self._drain_steps, cur)
        self.reset(slots)
        return self._drain_result

    def _drain_rows_of(self, name, needs):
        if self._drain_result is None or name not in self._drain_named:
            raise AttributeError(f"drain_raw_{name} needs a session {needs} after its first finish()")
        return self._drain_named[name]

    @property
    def drain_raw_poses(self):
        """(slots, lookahead, J, 3) float32 on the device: the poses of the last ``finish`` as the drain ticks emitted them, unfiltered -- in
        a session without ``smooth`` the buffer ``finish`` returns.  A session with extrinsics: the unfiltered WORLD rows, as ``raw_poses``."""
        return self._drain_rows_of("poses" if self.world is None else "world_poses", "")

    @property
    def drain_raw_roots(self):
        """(slots, lookahead, 3) float32 on the device (sessions with ``camera``): the roots of the last ``finish``, unfiltered; with
        extrinsics the unfiltered WORLD rows, as ``raw_roots``."""
        return self._drain_rows_of("roots" if self.world is None else "world_roots", "with camera")

    @property
    def drain_camera_poses(self):
        """(slots, lookahead, J, 3) float32 on the device (sessions with ``camera``): the poses of the last ``finish`` in camera space, as
        the drain's root solve read them -- ``camera_poses`` per drained row."""
        if self.cameras is None:
            raise AttributeError("drain_camera_poses needs a session with camera")
        return self._drain_rows_of("poses" if self.bones is None else "fixed_poses", "")

    @property
    def drain_camera_roots(self):
        """(slots, lookahead, 3) float32 on the device (sessions with ``camera``): the roots of the last ``finish`` in camera space."""
        return self._drain_rows_of("roots", "with camera")

    @property
    def frames(self):
        """MODEL frames per slot since its last reset (without ``fps``: the frames pushed): the device counters themselves, (slots,) int32."""
        return self._frames

    @property
    def source_frames(self):
        """Source frames pushed per slot since its last reset, (slots,) int32 on the device; without ``fps`` the same tensor as ``frames``."""
        return self._source_frames

    @property
    def raw_poses(self):
        """(slots, J, 3) float32 on the device: the poses as the tick emits them, the model's output, unfiltered and with the bones as
        the network gave them -- in a session without ``smooth`` and ``bones`` the buffer ``push`` returns.  Not with ``out_fps``
        (AttributeError).  A session whose ``Camera`` has extrinsics: the unfiltered WORLD poses -- what uu3d_camera_to_world wrote and
        the pose filter reads (with ``bones`` the rebuilt poses in world axes); ``camera_poses`` is the camera-space buffer.  A session
        with ``views``: the unfiltered FUSED poses, (N, J, 3); ``view_poses`` is the per-slot world buffer."""
        if self.max_out is not None:
            raise AttributeError("raw_poses: a session with out_fps returns several rows per slot")
        return self._scenes["fused" if self.views is not None else "raw" if self.world is None else "world"].poses

    @property
    def raw_roots(self):
        """(slots, 3) float32 on the device (sessions with ``camera``): the roots as they are solved, unfiltered; with extrinsics the
        unfiltered WORLD roots, which the root filter reads (``camera_roots`` is the camera-space buffer).  A session with ``views``:
        the unfiltered world roots of the N persons, (N, 3); ``view_roots`` is the per-slot world buffer."""
        if self.cameras is None:
            raise AttributeError("raw_roots needs a session with camera")
        return self._scenes["fused"].roots

    @property
    def view_poses(self):
        """(slots, J, 3) float32 on the device (sessions with ``views``): the per-slot world poses the fusion reads, slot v N + i person i in
        camera v -- what the session without ``views`` returns."""
        if self.views is None:
            raise AttributeError("view_poses needs a session with views")
        return self._scenes["world"].poses

    @property
    def view_roots(self):
        """(slots, 3) float32 on the device (sessions with ``views``): every slot's own monocular root in world coordinates."""
        if self.views is None:
            raise AttributeError("view_roots needs a session with views")
        return self._scenes["world"].roots

    @property
    def camera_poses(self):
        """(slots, J, 3) float32 on the device (sessions with ``camera``): the poses in CAMERA space as the root solve read them (with
        ``bones`` the rebuilt ones), unfiltered -- without extrinsics the buffer the pose filter reads."""
        if self.cameras is None:
            raise AttributeError("camera_poses needs a session with camera")
        return self._scenes["camera"].poses

    @property
    def camera_roots(self):
        """(slots, 3) float32 on the device (sessions with ``camera``): the roots in CAMERA space as they are solved, unfiltered --
        without extrinsics the same tensor as ``raw_roots``."""
        if self.cameras is None:
            raise AttributeError("camera_roots needs a session with camera")
        return self._scenes["camera"].roots

    @property
    def fixed_poses(self):
        """(slots, J, 3) float32 on the device (sessions with ``bones``): the rebuilt poses, unfiltered -- in a session without ``smooth``
        the buffer ``push`` returns."""
        if self.bones is None:
            raise AttributeError("fixed_poses needs a session with bones")
        return self._scenes["fixed"].poses

    @property
    def drain_fixed_poses(self):
        """(slots, lookahead, J, 3) float32 on the device (sessions with ``bones``): the rebuilt poses of the last ``finish``, unfiltered."""
        return self._drain_rows_of("fixed_poses", "with bones")

    @property
    def bone_lengths(self):
        """(slots, J) float64 on the device (sessions with ``bones``): the lengths every slot's pose was rebuilt with at the last tick, by
        child joint -- the running means of a "track" session (NaN before a slot's first fresh pose), else the given ones; 0 for the root."""
        if self.bones is None:
            raise AttributeError("bone_lengths needs a session with bones")
        return self._stages[0][1].lengths

    @property
    def rotation_flags(self):
        """(slots, J) uint8 on the device (sessions with ``rotations``): per slot and joint 1 = the quaternion was determined from the slot's
        last fresh pose, 0 = it fell back (or the slot has had no pose since its reset)."""
        if self.rotations is None:
            raise AttributeError("rotation_flags needs a session with rotations")
        return self._stages[-1][1].flags

    @property
    def joint_state(self):
        """(slots, J) uint8 on the device (sessions with ``repair_joints``): what became of the joints of each slot's newest frame, in the
        coding of ``predict_tracks(return_valid=True)`` -- 1 observed, 2 filled (held from its last observation), 0 neither."""
        if self.repair_joints is None:
            raise AttributeError("joint_state needs a session with repair_joints")
        return self._joint_state

    def _detections_only(self, name):
        if self.detections is None:
            raise AttributeError(f"{name} needs a session with detections")

    @property
    def track_ids(self):
        """(slots,) int32 on the device (sessions with ``detections``): the track in each slot after the last tick, -1 for a free slot."""
        self._detections_only("track_ids")
        return self._track_ids

    @property
    def assignment(self):
        """(D,) int32 on the device (sessions with ``detections``): the slot each detection of the last tick went to, -1: none."""
        self._detections_only("assignment")
        return self._assignment

    @property
    def dropped(self):
        """(1,) int32 on the device (sessions with ``detections``): detections dropped so far because no slot was free."""
        self._detections_only("dropped")
        return self._dropped

    @property
    def out_frames(self):
        """Output frames emitted per slot since its last reset (sessions with ``out_fps``), (slots,) int32 on the device."""
        if self.max_out is None:
            raise AttributeError("out_frames needs a session with out_fps")
        return self._out_frames

    def check_range(self):
        """Range guard of precision f16x3 for everything pushed so far, as ``ForwardPipeline.check_range()``: waits for the current stream,
        then raises ``Uu3dRangeError`` if a tick produced non-finite values."""
        self._torch.cuda.current_stream(self.model.device).synchronize()
        return self.model.check_range()

    def close(self):
        """Wait for what is in flight and give the session's workspace back."""
        if getattr(self, "_state", None) is not None:
            self._torch.cuda.synchronize(self.model.device)
            self._graph = self._drain_graph = None
            self.model._ws.pop(self._key, None)
            self._state = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _TickRecorder(object):
    """What the replays keep per tick beside poses and fresh flags: with ``placed`` four 32-bit words per slot -- the root's bits, the
    root state --, and ``turned`` quaternion buffers, the last ones a push appends.  One copy to the host, at the end."""

    def __init__(self, torch, ticks, slots, joints, placed, turned, device):
        self.words = torch.zeros((ticks, slots, 4), dtype=torch.int32, device=device) if placed else None
        self.quats = [torch.zeros((ticks, slots, joints, 4), dtype=torch.float32, device=device) for _ in range(turned)]

    def record(self, k, rs):
        for dst, src in zip(self.quats, rs[len(rs) - len(self.quats):]):
            dst[k].copy_(src)
        if self.words is not None:
            self.words[k, :, :3].copy_(rs[0].view(self.words.dtype))
            self.words[k, :, 3].copy_(rs[1])

    def host(self):
        """-> ((roots (ticks, slots, 3) float32, root_state (ticks, slots) uint8: a slot's ticks contiguous) or (), [quaternions])."""
        placed = ()
        if self.words is not None:
            words = self.words.cpu().numpy()
            placed = np.ascontiguousarray(words[:, :, :3]).view(np.float32), np.asfortranarray(words[:, :, 3].astype(np.uint8))
        return placed, [q.cpu().numpy() for q in self.quats]


def replay_tracks(model, config, tracks, resolutions=None, mask_stride=None, flip=None, lookahead=0, root_relative=True, graph=True, valid=None, fps=None,
                  model_fps=50, out_fps=None, drain=False, interpolation="linear", **options):
    """Push complete tracks tick by tick, one slot per track (a slot is inactive once its track has ended) -> per track the pose the
    session returned at each of its ticks, (T_i, J, 3) float32, and the fresh flags (T_i,) bool, as host arrays.  One copy to the host,
    at the end.  ``valid`` as ``predict.predict_tracks``: None, "finite" (rows with a NaN / Inf coordinate are missing frames) or one (T_i,)
    host array per track -- a session with ``missed_detections=True``.  ``fps`` / ``model_fps``: the rate of the tracks, as ``StreamSession``.
    ``out_fps=G``: -> per track the poses the session emitted, concatenated in order, (n_out_i, J, 3) float32 -- output frames
    0 .. n_out_i - 1 at G per second --, and the number each of its ticks returned, (T_i,) int32; still one copy to the host, at the end.
    ``repair_joints=G`` (keyword only, taken from ``options``): a session with ``repair_joints`` (it needs ``valid``); an entry of ``valid`` may
    then be (T_i, J), one flag per joint.  ``keypoints=M`` (from ``options`` as well): a session with ``keypoints``; the tracks are
    (T_i, K_in, 2) and per-joint entries of ``valid`` (T_i, K_in).  ``camera=C, min_root_joints=N`` (from ``options`` as well): a session with
    ``camera`` -- the roots (T_i, 3) float32 and root states (T_i,) uint8 the session returned at each tick are appended per track:
    -> (poses, fresh, roots, root_state).  ``smooth=F`` (from ``options`` as well): a session with ``smooth``; the same return, filtered.
    ``bones=B`` (from ``options`` as well): a session with ``bones``, one slot per track; the same return, the poses rebuilt.
    ``rotations=R`` (from ``options`` as well): a session with ``rotations``; per track the quaternions (T_i, J, 4) float32 the session
    returned at each tick are appended (with ``return_global`` the global ones behind them): one row per pushed frame.
    ``drain=True``: every slot is finished (``StreamSession.finish``) at the tick its own track ends, while the other slots go on; per
    track the arrays then have T_i + lookahead rows -- row t is the pose of frame t - lookahead (where it is fresh), so all T_i frames of
    the track come out, as from ``predict_tracks``.  Still one copy to the host, at the end.  Not with ``fps`` / ``out_fps`` (ValueError).
    ``interpolation``: handed to ``StreamSession`` as it is ("cubic" needs ``fps``)."""
    if drain and (fps is not None or out_fps is not None):
        raise ValueError("drain=True together with fps / out_fps is not supported yet (a later change): the drain of a source-rate session "
                         "needs the end of the model-rate track")
    import torch
    repair_joints, keypoints, camera, min_root_joints, smooth, bones, rotations = _live_options(options, "replay_tracks")
    lens = [int(len(t)) for t in tracks]
    T, ticks = len(tracks), max(lens)
    K = J = int(np.asarray(tracks[0]).shape[1])                      # joints pushed, joints returned
    if keypoints is not None:
        keypoints = keypoint_map(keypoints, config.NUM_KEYPOINTS)
        check_keypoint_inputs(keypoints, [np.asarray(t).shape[1] for t in tracks])
        J = keypoints.joints
    check_repair_joints(repair_joints, valid)
    flags = None
    if valid is not None and not isinstance(valid, str):
        check_valid(valid, lens, joints=None if repair_joints is None else K)
        flags = [np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) != 0 for v in valid]
        if repair_joints is not None:                                # one flag per joint: a (T_i,) entry stands for all joints of its frames
            flags = [f if f.ndim == 2 else np.repeat(f.reshape(-1, 1), K, axis=1) for f in flags]
    elif valid is not None and valid != "finite":
        raise ValueError('valid must be None, "finite" or a list with one (T_i,) array per track')
    s = StreamSession(model, config, T, resolutions=resolutions, mask_stride=mask_stride, flip=flip, lookahead=lookahead,
                      root_relative=root_relative, graph=graph, missed_detections=valid is not None, fps=fps, model_fps=model_fps, out_fps=out_fps,
                      repair_joints=repair_joints, keypoints=keypoints, camera=camera, min_root_joints=min_root_joints, smooth=smooth, bones=bones,
                      rotations=rotations, interpolation=interpolation)
    turned = 0 if s.rotations is None else 2 if s.rotations.return_global else 1          # quaternion buffers a push appends
    more = _TickRecorder(torch, ticks, T, J, camera is not None, turned, model.device)
    tails = None
    if drain:                                                         # per slot what its finish returned: finish's buffers last until the next one
        a = int(lookahead)
        tails = [torch.zeros((T, a, J, 3), dtype=torch.float32, device=model.device), torch.zeros((T, a), dtype=torch.bool, device=model.device)]
        if camera is not None:
            tails += [torch.zeros((T, a, 3), dtype=torch.float32, device=model.device), torch.zeros((T, a), dtype=torch.uint8, device=model.device)]
        tails += [torch.zeros((T, a, J, 4), dtype=torch.float32, device=model.device) for _ in range(turned)]
    if out_fps is None:
        poses = torch.zeros((ticks, T, J, 3), dtype=torch.float32, device=model.device)
        fresh = torch.zeros((ticks, T), dtype=torch.bool, device=model.device)
    else:                                                             # one block of 32-bit words per tick and slot: the count, then the rows' bits
        R = s.max_out
        words = torch.zeros((ticks, T, 1 + R * J * 3), dtype=torch.int32, device=model.device)
    kp = np.zeros((T, K, 2), np.float32)
    try:
        for k in range(ticks):
            act = np.array([k < n for n in lens])
            for i, t in enumerate(tracks):
                if act[i]:
                    kp[i] = t[k]
            if flags is None:
                p, f, *rs = s.push(kp, None if act.all() else act)
            else:
                p, f, *rs = s.push(kp, None if act.all() else act, valid=np.array([flags[i][k] & True if act[i] else flags[i][0] & False for i in range(T)]))
            more.record(k, rs)
            if out_fps is None:
                poses[k].copy_(p)
                fresh[k].copy_(f)
            else:
                words[k, :, 0].copy_(f)
                words[k, :, 1:].copy_(p.view(torch.int32).view(T, -1))
            ended = [i for i, n in enumerate(lens) if n == k + 1]
            if drain and ended:                                       # these tracks end here: their last `lookahead` poses, then the slots are reset
                for dst, src in zip(tails, s.finish(ended)):
                    for i in ended:
                        dst[i].copy_(src[i])
        s.check_range()
    finally:
        s.close()
    if out_fps is not None:
        words = words.cpu().numpy()
        counts = words[:, :, 0]
        rows = np.ascontiguousarray(words[:, :, 1:]).view(np.float32).reshape(ticks, T, R, J, 3)
        return ([np.concatenate([rows[k, i, :counts[k, i]] for k in range(n)] + [np.zeros((0, J, 3), np.float32)]) for i, n in enumerate(lens)],
                [counts[:n, i].astype(np.int32) for i, n in enumerate(lens)])
    poses, fresh = poses.cpu().numpy(), fresh.cpu().numpy()
    out = [poses[:n, i] for i, n in enumerate(lens)], [fresh[:n, i] for i, n in enumerate(lens)]
    placed, quats = more.host()
    for x in placed + tuple(quats):
        out += ([x[:n, i] for i, n in enumerate(lens)],)
    if drain:
        tails = [t.cpu().numpy() for t in tails]
        out = tuple([np.concatenate([rows, tail[i]]) for i, rows in enumerate(per_track)] for per_track, tail in zip(out, tails))
    return out


def replay_detections(model, config, detections, counts=None, valid=None, slots=None, resolutions=None, mask_stride=None, flip=None, lookahead=0,
                      root_relative=True, graph=True, drain=False, **options):
    """Push ONE video's per-frame detections tick by tick through a ``StreamSession(detections=D)`` and collect the poses per track id.
    ``detections`` (T, D, K, 2); ``counts`` (T,) or None; ``valid``: None, (T, D) or (T, D, K); ``slots`` (None: D); ``resolutions``: None
    or one (w, h); ``options``: ``max_age`` / ``max_dist`` / ``min_common``, ``repair_joints``, ``keypoints``, ``camera`` (one tuple) /
    ``min_root_joints``, ``smooth``, ``bones`` ("track" or lengths per SLOT: the device decides which person a slot is).
    -> a list of (track_id, first_frame, poses (n, J, 3) float32, fresh (n,) bool) by track id, host arrays: what the session returned for
    the track's slot at the ticks first_frame .. first_frame + n - 1, the ticks the track was alive (its trailing missing frames
    included; ``predict.predict_detections`` ends a track at its last matched frame).  With ``camera`` every tuple carries two more
    entries: roots (n, 3) float32 and root_state (n,) uint8 of those ticks; with ``rotations`` the quaternions (n, J, 4) float32 of those
    ticks behind them (one row per pushed frame).  One copy to the host, at the end.
    ``drain=True``: ``finish()`` runs after the last tick and its ``lookahead`` rows are appended to the arrays of every track alive at the
    end of the video (n + lookahead rows).  The limit: a track that died in mid-video (``max_age``) still loses the poses of its last
    ``lookahead`` frames -- the death happens on the device, and no drain is run there."""
    import torch
    detections = _host_array(detections)
    if detections.ndim != 4 or detections.shape[3] != 2:
        raise ValueError(f"detections must be (T, D, K, 2), got {detections.shape}")
    ticks, D = int(detections.shape[0]), int(detections.shape[1])
    S = D if slots is None else int(slots)
    counts = None if counts is None else np.asarray(_host_array(counts)).reshape(ticks)
    valid = None if valid is None else _host_array(valid)
    s = StreamSession(model, config, S, resolutions=resolutions, mask_stride=mask_stride, flip=flip, lookahead=lookahead, root_relative=root_relative,
                      graph=graph, detections=D, **options)
    J = int(model.arch.num_keypoints)
    poses = torch.zeros((ticks, S, J, 3), dtype=torch.float32, device=model.device)
    words = torch.zeros((ticks, 2, S), dtype=torch.int32, device=model.device)            # per tick: the fresh flags, the track ids
    turned = 0 if s.rotations is None else 2 if s.rotations.return_global else 1          # quaternion buffers a push appends
    more = _TickRecorder(torch, ticks, S, J, s.cameras is not None, turned, model.device)
    try:
        for k in range(ticks):
            p, f, *rs = s.push_detections(detections[k], None if counts is None else int(counts[k]), None if valid is None else valid[k])
            poses[k].copy_(p)
            words[k, 0].copy_(f)
            words[k, 1].copy_(s.track_ids)
            more.record(k, rs)
        tails = [t.clone() for t in s.finish()] if drain else None   # (the ids of the last tick say whose rows they are)
        s.check_range()
    finally:
        s.close()
    if drain:
        tails = [t.cpu().numpy() for t in tails]
    poses, words = poses.cpu().numpy(), words.cpu().numpy()
    fresh, ids = words[:, 0] != 0, words[:, 1]
    placed, quats = more.host()
    out = []
    for tid in range(int(ids.max()) + 1 if ids.size else 0):
        t, slot = np.nonzero(ids == tid)
        arrays = (poses[t, slot], fresh[t, slot]) + tuple(x[t, slot] for x in placed + tuple(quats))
        if drain and ticks and t[-1] == ticks - 1:                    # alive at the end of the video: the rows finish() gave its slot
            arrays = tuple(np.concatenate([x, tail[slot[-1]]]) for x, tail in zip(arrays, tails))
        out.append((tid, int(t[0])) + arrays)
    return out


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="python -m uplift_upsample_3dhpe_amd.stream", description="Replay the 2D keypoint tracks of an .npz file (one "
                                "(T, J, 2) array per track) tick by tick through a StreamSession -> an .npz with, per track NAME, the pose returned at "
                                "every tick (NAME: (T, J, 3) float32; the pose of frame tick - lookahead where NAME_fresh is set, else the held one).")
    p.add_argument("--config", required=True, help="model config (.json)")
    p.add_argument("--weights", required=True, help="weights (.h5)")
    p.add_argument("--input", required=True, help=".npz with one (T, J, 2) array per track")
    p.add_argument("--output", required=True, help=".npz to write")
    p.add_argument("--lookahead", type=int, default=0, help="frames the answer may lag behind the newest one (default 0)")
    add_track_options(p, True, "resolution")
    p.add_argument("--drain", action="store_true",
                   help="finish every track at its end: the arrays get T + lookahead rows, row t the pose of frame t - lookahead, so the last "
                        "lookahead frames of a track come out as well; not with --fps")
    add_track_options(p, True, "mask_missing", "fps", "out_fps", "repair_joints", "min_score", "keypoints", "camera", "min_root_joints", "smooth",
                      "smooth_root", "bones")
    args = p.parse_args(argv)
    if args.smooth_root is not None and args.camera is None:
        p.error("--smooth_root needs --camera: without it no roots are written")
    if (args.smooth is not None or args.smooth_root is not None) and args.out_fps is not None:
        p.error("--smooth / --smooth_root with --out_fps is not supported")
    if args.bones is not None and args.out_fps is not None:
        p.error("--bones with --out_fps is not supported")
    if args.out_fps is not None and args.fps is None:
        p.error("--out_fps needs --fps")
    if args.drain and args.fps is not None:
        p.error("--drain with --fps is not supported yet")
    if args.min_root_joints is not None and args.camera is None:
        p.error("--min_root_joints needs --camera: it is a parameter of the root solve")
    if args.camera is not None and args.out_fps is not None:
        p.error("--camera with --out_fps is not supported yet")
    if args.min_score is not None and args.repair_joints is None:
        p.error("--min_score needs --repair_joints: scores say which joints were seen")
    if args.repair_joints is not None and args.fps is not None:
        p.error("--repair_joints with --fps is not supported yet")
    return args


def main(argv=None):
    from .net.uplift_upsample_transformer_config import UpliftUpsampleConfig
    args = parse_args(argv)
    config = UpliftUpsampleConfig(args.config)
    with np.load(args.input) as z:
        names = list(z.files)
        tracks = [np.asarray(z[k], np.float32) for k in names]
    if not names:
        raise SystemExit(f"{args.input} holds no arrays")
    K, _ = input_joints(config, args.keypoints)
    tracks, joint_flags = split_scores(names, tracks, K, args.min_score, args.input)
    for k, t in zip(names, tracks):
        if t.shape[0] < 1:
            raise SystemExit(f"{args.input}[{k}] has shape {t.shape}, expected (T >= 1, {K}, 2)")
    options = track_keywords(args, config, names, joint_flags, live=True)
    if args.fps is None and not 0 <= args.lookahead <= max_lookahead(config):
        raise SystemExit(f"--lookahead must be in [0, {max_lookahead(config)}]")
    if args.fps is not None:
        try:
            rate_plan(config, args.fps, args.lookahead, out_fps=args.out_fps)
        except ValueError as e:
            raise SystemExit(f"--fps / --out_fps / --lookahead: {e}") from None
    model = _load_model(config, args.weights)
    poses, fresh, *rs = replay_tracks(model, config, tracks, resolutions=None if args.resolution is None else tuple(args.resolution),
                                      lookahead=args.lookahead, **({"drain": True} if args.drain else {}), **options)
    out = {}
    if rs:
        out.update({k + "__root": np.asarray(r, np.float32) for k, r in zip(names, rs[0])})
        out.update({k + "__root_state": np.asarray(r, np.uint8) for k, r in zip(names, rs[1])})
    for k, p, f in zip(names, poses, fresh):
        out[k] = np.asarray(p, np.float32)
        if args.out_fps is None:
            out[k + "_fresh"] = np.asarray(f, bool)
        else:
            out[k + "_count"] = np.asarray(f, np.int32)
    np.savez(args.output, **out)
    if args.out_fps is not None:
        print(f"wrote {args.output}: {len(names)} tracks, {sum(len(f) for f in fresh)} ticks, {sum(len(p) for p in poses)} poses at {args.out_fps} fps", flush=True)
        return 0
    print(f"wrote {args.output}: {len(names)} tracks, {sum(len(p) for p in poses)} ticks, {int(sum(f.sum() for f in fresh))} fresh poses", flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
