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
        [--resolution W H] [--mask_stride S] [--keyframes_only] [--mask_missing] [--fps F] [--out_fps F] [--repair_joints G] [--min_score S]
        [--keypoints NAME] [--camera FX FY CX CY] [--min_root_joints N] [--smooth MIN_CUTOFF BETA D_CUTOFF] [--smooth_root MIN_CUTOFF BETA D_CUTOFF]
        [--bones track|FILE.npy]

The stages behind the options, one module each -- what an option does, its launches and its rule in numpy stand in the module's docstring;
every name is importable from here as before:
    validity.py   per-joint missed detections: ``predict_tracks(..., valid=..., repair_joints=G)`` (uu3d_repair_joints)
    keypoints.py  any skeleton: ``predict_tracks(..., keypoints="coco17")`` (uu3d_map_keypoints; ``KeypointMap``, ``KEYPOINT_PRESETS``)
    associate.py  per-frame detections: ``predict_detections`` (uu3d_associate_detections), then ``predict_tracks`` on the tracks
    roots.py      absolute root position: ``predict_tracks(..., camera=(fx, fy, cx, cy))`` (uu3d_solve_roots, uu3d_root_trajectory)
    smooth.py     steady output: ``predict_tracks(..., smooth=OneEuro(min_cutoff, beta, d_cutoff))`` (uu3d_one_euro_tracks; ``zero_lag=True``: uu3d_one_euro_tracks_two_pass)
    rotations.py  joint rotations: ``predict_tracks(..., rotations=True)`` (uu3d_joint_rotations; ``bvh.write_bvh``)
    bones.py      constant bone lengths: ``predict_tracks(..., bones="track")`` (uu3d_bone_lengths, uu3d_fix_bones)
    tracks.py     the pose table and the three uu3d_*_tracks launches above, and uu3d_assemble_tracks_cubic: C1 motion between the predicted
                  frames, ``predict_tracks(..., interpolation="cubic")`` (``evaluation.keyframe_plan_cubic``, ``interpolate_cubic_host``); options.py: the checks of all these options, shared with a live
                  session; cli.py: the command-line options, shared with ``stream``
    camera.py     lens distortion: ``predict_tracks(..., camera=Camera(fx, fy, cx, cy, distortion=(k1, k2, p1, p2, k3)))`` (uu3d_undistort_points;
                  ``undistort_points``, ``undistort_points_host``, ``distort_points_host``); world space: ``camera=Camera(..., orientation=(w, x,
                  y, z), translation=(tx, ty, tz))`` (uu3d_camera_to_world; ``camera_to_world``, ``camera_to_world_host``,
                  ``world_to_camera_host``, ``extrinsics_from_opencv``)
    views.py      several calibrated cameras, one scene: ``predict_views(model, config, views, cameras)`` (uu3d_fuse_views, uu3d_solve_view_roots;
                  ``fuse_views``, ``solve_view_roots``, ``fuse_views_host``, ``solve_view_roots_host``); who is who across cameras:
                  ``predict_views(..., match=True)`` / ``match_views`` (uu3d_view_pair_sums, uu3d_group_views, uu3d_gather_view_tracks;
                  ``view_pair_sums``, ``group_views``, ``gather_view_tracks`` and their ``_host`` mirrors, ``MatchViews``); one clock:
                  ``predict_views(..., align=True)`` / ``align_views`` / ``crop_views`` (uu3d_view_lag_sums, uu3d_view_offsets;
                  ``view_lag_sums``, ``view_offsets`` and their ``_host`` mirrors, ``AlignViews``); where rays meet:
                  ``predict_views(..., triangulate=True)`` (uu3d_triangulate_joints, uu3d_place_joints; ``triangulate_joints``,
                  ``place_joints`` and their ``_host`` mirrors, ``Triangulate``); where the cameras stand:
                  ``predict_views(..., calibrate=True)`` / ``calibrate_views`` / ``calibrated_cameras`` (uu3d_view_moment_sums,
                  uu3d_view_position_sums, uu3d_solve_view_pose; ``view_moment_sums``, ``view_position_sums``, ``solve_view_pose`` and their
                  ``_host`` mirrors, ``calibrate_views_host``, ``CalibrateViews``); who is who without a world:
                  ``predict_views(..., match=MatchLifts(...))`` / ``match_lifts`` (uu3d_lift_pair_sums; ``lift_pair_sums`` and the ``_host``
                  mirrors, ``MatchLifts``)
"""
import argparse
import types
# (noqa: F401 below -- re-exported: every name this module had before the stages became modules of their own)
from fractions import Fraction  # noqa: F401

import numpy as np

from . import _capi, evaluation  # noqa: F401
from . import eval as ev
from ._capi import ptr as _ptr  # noqa: F401
from .associate import (ASSOCIATION_DEFAULTS, MAX_ASSOCIATION, Association, AssociationHost, _association_options,  # noqa: F401
                        _detection_flags, _device_detections, associate_detections, associate_host, association_tracks_host, check_association)
from .bones import (MAX_BONE_JOINTS, SKELETONS, Bones, Skeleton, _bone_device_poses, _bone_length_table, _bone_offsets, _bone_poses,  # noqa: F401
                    bone_lengths, bone_lengths_host, check_bones, fix_bones, fix_bones_host, skeleton_of)
from .camera import (Camera, camera_to_world, camera_to_world_host, camera_to_world_rows, distort_points_host, extrinsics_from_opencv,  # noqa: F401
                     split_cameras, undistort_points, undistort_points_host, undistort_rows, world_to_camera_host)
from .cli import add_track_options, bones_option, input_joints, smooth_option, split_scores, track_keywords  # noqa: F401
from .data import PoseTable, SequenceGenerator  # noqa: F401
from .keypoints import (KEYPOINT_PRESETS, MAX_KEYPOINT_SOURCES, KeypointMap, _h36m17_from, _map_front, check_keypoint_inputs,  # noqa: F401
                        keypoint_map, map_keypoints, map_keypoints_host)
from .options import INTERPOLATIONS, check_interpolation, stage_options  # noqa: F401
from .rates import (_rate_argument, default_mask_stride, frame_rate, frame_rates, given_positions, output_positions,  # noqa: F401
                    resample_plan, root_plan)
from .rotations import (REST_POSES, Rotations, check_rotations, forward_kinematics, joint_rotations, joint_rotations_host,  # noqa: F401
                        quat_to_matrix)
from .roots import (DEFAULT_MIN_ROOT_JOINTS, MAX_ROOT_JOINTS, _root_lens, check_cameras, check_min_root_joints, poses_at_given_frames,  # noqa: F401
                    root_trajectory, root_trajectory_host, solve_roots, solve_roots_host)
from .smooth import (MAX_SMOOTH_CHANNELS, TWO_PI, OneEuro, _one_euro_rates, check_smooth, one_euro, one_euro_alpha, one_euro_host,  # noqa: F401
                     one_euro_sample)
from .tracks import (_device_track, _device_tracks, _host_array, _shape, _upload, assemble_tracks, assemble_tracks_cubic,  # noqa: F401
                     check_resolutions, keyframe_count, normalize_tracks, pose_table, resample_tracks, resampled_pose_table)
from .views import (ALIGN_DEFAULTS, MATCH_DEFAULTS, MATCH_LANES, MAX_ALIGN_LAG, MAX_MATCH_TRACKS, MAX_VIEWS, MIN_TRIANGULATE_VIEWS,  # noqa: F401
                    TRIANGULATE_DEFAULTS, VIEW_PARALLEL, AlignViews, MatchViews, Triangulate, align_views, align_views_host, check_align, check_match,
                    check_triangulate, check_view_cameras, check_view_of, crop_views, fuse_views, fuse_views_host, gather_view_tracks,
                    gather_view_tracks_host, group_views, group_views_host, match_views, match_views_host, place_joints, place_joints_host,
                    predict_views, solve_view_roots, solve_view_roots_host, triangulate_joints, triangulate_joints_host, view_lag_sums,
                    view_lag_sums_host, view_offsets, view_offsets_host, view_pair_sums, view_pair_sums_host, view_rows)
from .views import (VIEW_CALIBRATE_DEFAULTS, CalibrateViews, calibrate_views, calibrate_views_host, calibrated_cameras, check_calibrate,  # noqa: F401
                    solve_view_pose, solve_view_pose_host, view_moment_sums, view_moment_sums_host, view_position_sums, view_position_sums_host)
from .views import LIFT_MATCH_DEFAULTS, MatchLifts, lift_pair_sums, lift_pair_sums_host, match_lifts, match_lifts_host  # noqa: F401
from .validity import (_device_joint_flags, _device_valid, _front_validity, _source_joint_flags, check_repair_joints, check_valid,  # noqa: F401
                       repair_joints, repair_joints_host)


def predict_detections(model, config, detections, counts=None, valid=None, slots=None, **options):
    """3D poses straight from a multi-person detector's per-frame lists.  ``detections``: list of (T_v, D, K, 2) arrays or tensors, one
    per video: per frame up to D people in ANY order (``counts[v]`` (T_v,): how many rows are given; None = D); ``valid``: None, "finite"
    or a list of (T_v, D) / (T_v, D, K) flags (``scores >= 0.3``); ``slots`` = S (None: D): the people followed at the same time;
    ``max_age`` / ``max_dist`` / ``min_common``: the rule's parameters (``ASSOCIATION_DEFAULTS``: conveniences, not tuned values).
    Every other keyword goes to ``predict_tracks`` unchanged (``keypoints``, ``repair_joints``, ``fps``, ``resolutions`` -- one (w, h) or
    one per VIDEO --, ...); ``keyframes_only`` / ``lengths`` / ``return_valid`` are not taken.
    -> per video a list of (track_id, first_frame, poses (n, J, 3)) by track id: a track runs from its birth frame to its last matched
    frame; a frame in between without a match is a missed detection, as is a joint that was not observed (``repair_joints`` fills those).
    The association (``associate_host`` is its rule) runs on the device in one launch; then ONE small copy to the host -- the (frames, D)
    int32 track ids and two counters per video, which say where each track begins and ends -- and the tracks' coordinates and per-joint
    flags are gathered on the device for ``predict_tracks(valid=flags)``.  The result equals ``predict_tracks`` on the tracks of
    ``association_tracks_host``, bit for bit.  Needs a model with strided input.  Greedy, no motion model: no tracking accuracy is claimed.
    ``camera``: one (fx, fy, cx, cy) or one per VIDEO, handed to ``predict_tracks`` per track the way ``resolutions`` is: the tuples become
    (track_id, first_frame, poses, roots (n, 3) float32, root_state (n,) uint8) -- every person of a video in the same camera space.
    A ``Camera`` with distortion (one, or one per video): uu3d_undistort_points takes all D x K points of every frame back to the pinhole's
    pixels before the association looks at them (``camera.py``); the result equals the call on ``undistort_points_host`` of the
    detections with the plain tuple, bit for bit.  A ``Camera`` with extrinsics (one, or one per video): every track of a video goes
    to that video's world axes by uu3d_camera_to_world, behind the root solve and in front of ``smooth`` and ``rotations``, as in
    ``predict_tracks`` ("World space").
    ``smooth``: handed to ``predict_tracks`` as it is -- every track's poses (and roots) filtered from its birth frame on (a ``OneEuro``
    with ``zero_lag`` as well: forwards from the birth frame, then back from the track's last frame).
    ``bones``: handed to ``predict_tracks`` as it is -- "track" or one (J,) array of lengths for every person (the tracks are only known
    after the association, so there is no per-track list here).
    ``rotations``: handed to ``predict_tracks`` as it is -- every tuple carries the track's (n, J, 4) quaternions behind what it has
    otherwise (and, with ``return_global``, the global ones behind those).
    ``interpolation``: "linear" (the default) or "cubic", handed to ``predict_tracks`` as it is; anything else is refused here, before the
    association runs."""
    import torch
    assoc, options = _association_options(options)
    check_interpolation(options.get("interpolation", "linear"))
    camera, lens, placed = options.pop("camera", None), None, None
    if camera is not None:
        given = camera
        camera, lens = split_cameras(camera, len(detections), per="video")
        camera = check_cameras(camera, len(detections), per="video")
        cams = [given] * len(detections) if isinstance(given, Camera) else given
        if isinstance(cams[0], Camera) and cams[0].has_extrinsics:     # world space: each video's extrinsics go on to its tracks
            placed = [c.without(distortion=True) for c in cams]      # (the lens is taken off here, in front of the association)
    for k in ("keyframes_only", "lengths", "return_valid"):
        if options.get(k):
            raise ValueError(f"predict_detections does not take {k}")
    if not model.has_strided_input:
        raise ValueError("predict_detections needs a model with strided input: a frame without a match becomes the learned masked token")
    if lens is not None:                                              # lens distortion: all D x K points of every frame, before the association
        flat, _, _, _, frames = _device_detections(detections, None, None, torch.device(model.device))
        flat = undistort_rows(flat.reshape(flat.shape[0], -1, 2), lens, frames).reshape(flat.shape)
        detections = list(torch.split(flat, [int(n) for n in frames], 0))
    r = associate_detections(detections, counts, valid, slots=slots, device=model.device, **assoc)
    dets, flags, per_joint, lens, track_of = r._flat
    F, D, K = int(dets.shape[0]), int(dets.shape[1]), int(dets.shape[2])
    V = len(lens)
    back = torch.cat([track_of.reshape(-1), r.counters.reshape(-1)]).cpu().numpy()      # the one copy to the host (it waits for the launch)
    ids, num = back[:F * D].reshape(F, D), back[F * D:].reshape(V, 2)[:, 0]
    start = np.concatenate([[0], np.cumsum(lens)])
    rows, spans = [], []                                              # per track the row of (F * D) it reads at each of its frames; F * D: none
    for v in range(V):
        own = ids[start[v]:start[v + 1]]
        for tid in range(int(num[v])):
            frames, which = np.nonzero(own == tid)
            first, n = int(frames[0]), int(frames[-1]) - int(frames[0]) + 1
            idx = np.full(n, F * D, np.int64)
            idx[frames - first] = (start[v] + frames) * D + which
            rows.append(idx)
            spans.append((v, tid, first))
    if not rows:
        return [[] for _ in range(V)]
    index = _upload(np.concatenate(rows), np.int64, dets.device)
    xy = torch.cat([dets.reshape(F * D, K, 2), torch.zeros((1, K, 2), dtype=torch.float32, device=dets.device)], 0).index_select(0, index)
    if flags is None:
        jf = (index < F * D).to(torch.uint8).reshape(-1, 1).expand(-1, K).contiguous()
    else:
        per = flags.reshape(F * D, K) if per_joint else flags.reshape(F * D, 1).expand(-1, K)
        jf = torch.cat([per, torch.zeros((1, K), dtype=torch.uint8, device=dets.device)], 0).index_select(0, index)
    sizes = [len(i) for i in rows]
    res = options.pop("resolutions", None)
    if res is not None:
        res = check_resolutions(res, V, per="video")[[v for v, _, _ in spans]]
    if camera is not None:
        options["camera"] = camera[[v for v, _, _ in spans]] if placed is None else [placed[v] for v, _, _ in spans]
    poses = predict_tracks(model, config, list(torch.split(xy, sizes, 0)), valid=list(torch.split(jf, sizes, 0)), resolutions=res, **options)
    out = [[] for _ in range(V)]
    for (v, tid, first), *p in zip(spans, *(poses if isinstance(poses, tuple) else (poses,))):
        out[v].append((tid, first, *p))
    return out


def predict_tracks(model, config, tracks, resolutions=None, mask_stride=None, flip=None, keyframes_only=False, reuse_frames=True,
                   batch_size=None, root_relative=True, depth=None, lengths=None, graph=True, valid=None, return_valid=False, fps=None, out_fps=None,
                   model_fps=50, repair_joints=None, keypoints=None, camera=None, min_root_joints=DEFAULT_MIN_ROOT_JOINTS, smooth=None,
                   bones=None, rotations=None, interpolation="linear"):
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
    model with generic dimensions runs the window forward here whatever ``reuse_frames`` says (its results stay what they were).  One rank only.

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
    ``fps=video rate / s_in, out_fps=video rate`` instead.

    Per-joint missed detections -- ``repair_joints``: None = today's call, the same bits, no further launch or buffer; an entry of ``valid``
    may then also be (T_i, J) and counts per frame, all of its joints.  An int G >= 1 (needs ``valid``; ValueError otherwise): a joint the
    detector lost for up to G consecutive given frames -- source frames with ``fps``, given keyframes with ``keyframes_only`` -- is filled
    on the device (uu3d_repair_joints) before anything else looks at the track.  A joint is OBSERVED when its flag is non-zero (``valid``
    "finite": no flags; a (T_i,) entry: the frame's flag for all joints; a (T_i, J) entry, e.g. ``scores >= 0.3``: its own) and both
    coordinates are finite.  An unobserved joint between two observations l < t < r of the same joint with r - l - 1 <= G becomes
    ``src[l] * (1.0 - w) + src[r] * w``, w = (t - l) / (r - l), in float64 on the raw coordinates, rounded once to float32; before the
    joint's first observation r (r - t <= G) or behind its last one l (t - l <= G) it is held.  A frame with at least one observed joint
    and all others filled is a real observation; a frame with no observed joint is never filled, and a frame with a joint that cannot be
    filled is missing as well -- the network upsamples over both as over any missing frame.  The result equals, bit for bit,
    ``predict_tracks(repaired, valid=frame_flags)`` with the output of ``repair_joints_host``, the rule in numpy.
    ``return_valid=True`` then returns (poses, flags, joint_state): joint_state a list of (given frames of track i, J) uint8 device tensors,
    1 observed, 2 filled, 0 neither.  ``StreamSession`` and ``replay_tracks`` have no such option and keep refusing anything but (T_i,)
    flags: a session computes a frame's spatial features once, at its push, when the joint's right neighbour is not known yet, so a causal
    fill would break the session's contract (the pose of ``predict_tracks`` on the track cut at that frame).

    Any skeleton -- ``keypoints``: None = the tracks are in the model's own joint layout (today's call, the same bits, no further launch or
    buffer).  Else a name of ``KEYPOINT_PRESETS`` ("coco17", "body25": onto the 17 Human3.6M joints of the shipped configs; geometric
    approximations of the joints a detector does not emit, no accuracy figure claimed) or a ``KeypointMap`` of your own onto the model's J
    joints (ValueError for another J): ``tracks[i]`` is then (T_i, K_in, 2) in the DETECTOR's layout -- a wrong joint count is a ValueError
    naming both numbers -- and uu3d_map_keypoints turns it into (T_i, J, 2) on the device, on the raw coordinates, before anything else
    looks at the track: model joint j is ``sum_k w[j][k] * in[src[j][k]]`` in float64, summed in the listed order, rounded once.  Per-joint
    entries of ``valid`` are (T_i, K_in), one flag (``scores >= 0.3``) per DETECTOR joint, and "finite" is the finite test per source joint:
    a model joint is observed iff every one of its sources is, and an unobserved one is zeros with flag 0 -- a lost COCO shoulder is a
    lost neck and a lost torso, and nothing else; (T_i,) frame flags pass through.  ``joint_state`` stays per model joint.  The result
    equals, bit for bit, ``predict_tracks(mapped, valid=flags)`` with the output of ``map_keypoints_host``, the rule in numpy.

    Absolute root position -- ``camera``: None = today's call, the same bits, no further launch or buffer.  Else the camera's intrinsics
    (fx, fy, cx, cy), in the units of the tracks AS GIVEN (pixels when ``resolutions`` is given), one tuple or one per track
    (non-finite, fx <= 0 or fy <= 0: ValueError): ``roots``, a list of (T_i, 3) float32 device tensors (views of one buffer), and
    ``root_state``, a list of (T_i,) uint8 ones, are APPENDED to whatever the call returns -- (poses, roots, root_state), (poses, flags,
    roots, root_state) or (poses, flags, joint_state, roots, root_state); the poses are those of the call without ``camera``, bit for bit,
    and ``poses[i] + roots[i][:, None]`` stands in the camera's space.  At every GIVEN frame the root is where the returned pose must stand
    so that it projects onto the frame's 2D keypoints: linear least squares over the USED joints -- the joint's flag is set (after the
    ``keypoints`` map; ``valid=None``: all of them) and both raw coordinates are finite; with ``repair_joints`` a filled joint is not used
    (an interpolation, not a measurement), and a frame the network never saw still fixes its root from the joints that were seen.  A frame
    is SOLVED with at least ``min_root_joints`` (an int >= 2) used joints that do not share one pixel, a finite root with Tz > 0 and every
    used joint in front of the camera (uu3d_solve_roots; the rule in numpy: ``solve_roots_host``).  The root motion is the
    piecewise-linear function through a track's solved given frames, read at the times of the returned frames -- frame i at given-frame
    position i (plain, ``fps``), i / s_in (``keyframes_only``) or i fps / out_fps (with ``out_fps``; the poses at the given frames' times
    then come from a second uu3d_assemble_tracks over the same raw predictions, no further forward) -- and held before the first and
    behind the last solved frame (uu3d_root_trajectory; ``root_trajectory_host``).  ``root_state``: 1 solved here, 2 interpolated or held,
    0 the track has no solved frame (zeros).  With ``root_relative=False`` the solve takes the pose as returned.  No accuracy is claimed:
    the model's scale error goes 1:1 into the depth.  The live form is ``StreamSession(camera=...)`` / ``replay_tracks(camera=...)``: the
    same solve per emitted pose at any ``lookahead``, the last solved root held where a frame is not solved (causal: no interpolation).

    Lens distortion -- ``camera=Camera(fx, fy, cx, cy, distortion=(k1, k2, p1, p2, k3), tol=1e-3)``, one or one per track (a list that
    mixes tuples and ``Camera``s, or ``Camera``s with and without distortion: ValueError): the intrinsics as above, and the given points
    are first taken back to the pixels an ideal pinhole would have seen -- uu3d_undistort_points, the FIRST launch of the call, on the
    given frames in the detector's layout, in front of uu3d_map_keypoints; one lane per point, 20 steps of OpenCV's fixed-point iteration
    in float64 and an acceptance check against the forward model (``camera.py``; ``undistort_points`` is the launch alone; the rule in
    numpy: ``undistort_points_host``).  Everything behind reads the undistorted points: the ``keypoints`` map, ``repair_joints``, the
    normalisation or resampling, and the root solve; the caller's memory is never written.  A point that is not accepted -- non-finite,
    or outside the region where the model can be inverted -- becomes (NaN, NaN): ``valid="finite"`` is the companion option, which makes
    it a lost joint (``repair_joints``) or a missing frame; the root solve never uses it.  The result equals, bit for bit,
    ``predict_tracks(undistort_points_host(tracks, camera), camera=(fx, fy, cx, cy))`` in every form of the call.  A ``Camera`` without
    distortion (None or all zeros) is the plain tuple: the same launches, buffers and bits.  No accuracy is claimed.

    World space -- ``camera=Camera(fx, fy, cx, cy, orientation=(w, x, y, z), translation=(tx, ty, tz))``, one or one per track (with or
    without ``distortion``; a list of ``Camera``s with and without extrinsics: ValueError): the camera's extrinsics in the convention of
    ``h36m.camera_to_world``, ``X_world = qrot(orientation, X_cam) + translation`` (``extrinsics_from_opencv`` makes them from OpenCV's
    (R, tvec)).  The stages then run in this order: assembly, ``bones``, the root solve and the trajectory in camera space as without
    extrinsics, then uu3d_camera_to_world -- one launch over all tracks' returned rows, one lane per joint and per root, float64 with
    every operation rounded once (``camera.py``; ``camera_to_world`` is the launch alone; the rule in numpy: ``camera_to_world_host``) --,
    then the pose filter and the root filter of ``smooth``, then ``rotations``.  Poses are rotated only and stay root-relative (the root
    joint's zeros stay +0.0; ``poses + roots[:, None]`` is the world scene, with ``root_relative=False`` as well), a root with state 1 or
    2 is rotated and translated, a root with state 0 stays zeros.  So the filters steady the world's axes, and the quaternions -- and a
    BVH written from them -- stand in world axes.  It holds in every form of the call (``keyframes_only``, ``fps``, ``out_fps``,
    ``valid`` / ``repair_joints``, ``keypoints``, ``interpolation="cubic"``; the poses re-read at the given frames' times for the root
    solve with ``out_fps`` stay in camera space).  The result equals, bit for bit, ``one_euro_host`` and ``joint_rotations_host`` applied
    to ``camera_to_world_host`` of the call with the ``Camera`` minus extrinsics and ``smooth=None, rotations=None``.  A ``Camera``
    without extrinsics: the same launches, buffers and bits as before.  No accuracy is claimed.

    Steady output -- ``smooth``: None = today's call, the same bits, no further launch or buffer.  True (the defaults), a ``OneEuro`` or a
    pair (pose_filter, root_filter), either of which may be None (``check_smooth``; a root filter without ``camera``: ValueError): the
    returned poses -- and, with ``camera``, the returned roots -- go once through the One-Euro filter, an exponential smoother whose
    cut-off rises with the speed of the signal (uu3d_one_euro_tracks, one launch each; ``one_euro`` is the launch alone; the rule in numpy:
    ``one_euro_host``, and the result equals it on the output of the call without ``smooth``, bit for bit).  A channel is one coordinate of
    one joint (C = 3 J) or of the root (C = 3); the sample rate is that of the RETURNED frames: ``model_fps`` for the plain call and with
    ``keyframes_only``, the track's ``fps`` with ``fps``, ``out_fps`` with ``out_fps``.  The roots are solved from the UNFILTERED poses,
    exactly as without ``smooth``; a root row of state 0 (zeros) is passed through and takes no sample; ``root_state`` and the flags are
    unchanged, and the root joint of a root-relative pose stays exactly 0.  A plain ``OneEuro`` is CAUSAL: frame i depends on the frames
    up to i only, so the result lags behind the motion exactly as the live one (``StreamSession(smooth=...)``) does.
    ``OneEuro(..., zero_lag=True)`` -- offline only, for either member of the pair independently, at every returned rate -- filters a
    track in two passes (uu3d_one_euro_tracks_two_pass, still one launch each): pass 1 is the causal walk, pass 2 the same walk over pass
    1's float32 rows taken last to first, with the same rate, parameters and ``root_state`` bytes and fresh filter state, each pass
    taking its first usable sample as given; per track the result is reverse(one_euro_host(reverse(one_euro_host(x)))) with the causal
    filter, bit for bit, which is what ``one_euro_host`` computes for such a filter.  On a ramp the forward and the backward lag are one
    constant and cancel.  A live session cannot do this and refuses such a filter.  No accuracy or jitter figure is claimed.

    Constant bone lengths -- ``bones``: None = today's call, the same bits, no further launch or buffer.  The network predicts every
    frame's skeleton on its own, so a person's bone lengths breathe from frame to frame, and under ``camera`` the depth with them.
    "track": every track's bones get the track's own mean lengths (uu3d_bone_lengths over the returned frames); a (J,) array of lengths in
    the poses' units, indexed by CHILD joint (the root's entry is ignored), or a list of such arrays, one per track: a subject whose
    lengths are known -- calibrated once with ``bone_lengths`` on a recording --, which also takes the model's scale error out of the
    depth; ``Bones(lengths, skeleton=...)``: the same for a tree of your own (``Skeleton``).  The default tree is ``SKELETONS["h36m17"]``
    (another joint count: ValueError naming ``Skeleton``), and with ``root_relative`` its root must be ROOT_KEYTPOINT.  Directly behind
    uu3d_assemble_tracks every pose is rebuilt from the root outwards, each bone scaled to its length and its direction kept
    (uu3d_fix_bones; ``fix_bones`` is the launch alone; the rule in numpy: ``bone_lengths_host`` / ``fix_bones_host``, and the poses equal
    ``fix_bones_host`` on the call without ``bones``, bit for bit).  Everything behind reads the fixed poses: the pose filter of
    ``smooth`` and the root solve of ``camera`` -- with ``out_fps`` its re-assembled poses at the given frames' times are fixed with the
    same lengths table.  A length that is not finite or <= 0 (a track without a usable frame) leaves that bone as it is; a NaN frame stays
    NaN; the root joint of a root-relative pose stays exactly 0.  No accuracy figure is claimed.

    Joint rotations -- ``rotations``: None = today's call, the same bits, no further launch or buffer.  True (``Rotations("h36m17")``) or
    a ``Rotations(rest, skeleton=..., primary=..., secondary=..., return_global=...)``: the call appends ``rotations``, a list of
    (T_i, J, 4) float32 device tensors, behind whatever it returns otherwise -- per returned frame and joint the unit quaternion
    (w, x, y, z) of the joint relative to its parent's frame, the root's relative to the pose's space -- and with ``return_global`` the
    list ``global_rotations`` behind that.  They are computed from the RETURNED poses (behind ``bones``, behind ``smooth``, at the returned
    frame times) in one launch over all tracks' rows (uu3d_joint_rotations; ``joint_rotations`` is the launch alone; the rule in numpy:
    ``joint_rotations_host``, and the result equals it on the returned poses bit for bit).  A model whose joint count is not the
    skeleton's: ValueError.  Positions do not show the twist about a bone with a single child: it is zero relative to the parent.  No
    accuracy figure is claimed (``rotations.py``).

    C1 motion between keyframes -- ``interpolation``: "linear" = today's call, the same launches, buffers and bits: a returned frame
    between two predicted ones lies on the line through them (the evaluation's protocol), so the velocity jumps at every predicted frame.
    "cubic": it lies on the C1 cubic through the same predictions instead -- the Hermite segment between the two with Catmull-Rom
    tangents, which reads the predicted frame in front of the left one and the one behind the right one as well (at a track's first and
    last segment the segment's own difference stands in).  uu3d_assemble_tracks_cubic replaces uu3d_assemble_tracks, one launch for one
    launch, no further forward (``assemble_tracks_cubic`` is the launch alone; the plan: ``evaluation.keyframe_plan_cubic`` /
    ``keyframe_plan_cubic_at``; the rule in numpy: ``evaluation.interpolate_cubic_host``, and the poses equal it on the raw window
    predictions bit for bit).  A predicted frame, a frame behind a track's last predicted one and the root joint of a root-relative pose
    keep the linear call's bits; a model that predicts every frame returns the linear call's bits everywhere.  It holds in every form of
    the call -- ``keyframes_only``, ``fps``, ``out_fps``, ``valid`` / ``repair_joints``, ``keypoints`` -- and everything behind reads the
    cubic poses: ``bones``, ``smooth``, ``rotations``, and the root solve of ``camera`` (with ``out_fps`` its poses at the given frames'
    times are read from the same cubic); the root trajectory itself stays piecewise linear through the solved frames, which lie at every
    given frame, not at keyframes.  Anything else: ValueError.  Offline only: a live session would need one more predicted frame of
    lookahead, and ``run_eval``'s report keeps the reference's protocol.  No accuracy figure is claimed."""
    import torch
    front = _assembled_tracks(model, config, tracks, resolutions, mask_stride, flip, keyframes_only, reuse_frames, batch_size, root_relative, depth,
                              lengths, graph, valid, fps, out_fps, model_fps, repair_joints, keypoints, camera, min_root_joints, smooth, bones,
                              rotations, interpolation)
    opts, table, given, lens, model_lens, rates, mask_stride = front.opts, front.table, front.given, front.lens, front.model_lens, front.rates, front.mask_stride
    assemble, plan_at, frame_idx, rows, stride, out = front.assemble, front.plan_at, front.frame_idx, front.rows, front.stride, front.out
    # bones: constant bone lengths -- everything behind reads the fixed poses
    if opts.rigid is not None:
        skeleton, known = opts.rigid
        bone_table = bone_lengths(out, lens, skeleton) if known is None else _upload(known, np.float64, out.device)
        out = fix_bones(out, lens, bone_table, skeleton)
    shown = out
    if opts.pose_filter is not None or opts.root_filter is not None:
        out_rate = model_fps if fps is None else (rates if out_fps is None else frame_rates(out_fps, len(tracks)))
    sizes = [int(n) for n in lens]
    # roots: solved at the given frames, joined to a trajectory that is read at the returned frames -- in camera space, from the unfiltered poses
    roots = root_state = None
    if camera is not None:
        def reread(at):                                               # the same motion at the given frames' times (``out_fps``)
            again = assemble(plan_at(frame_idx, 1 if stride is None else stride, at, rows=rows))
            return again if opts.rigid is None else fix_bones(again, given, bone_table, skeleton)
        at_given, where = poses_at_given_frames(out, lens, given, int(mask_stride) if keyframes_only else 0, rates if fps is not None else None,
                                                out_fps, model_fps, reread)
        solved_roots, solved = solve_roots(at_given, table.source[0], opts.cameras, table.source[1], opts.min_root_joints, lens=given)
        roots, root_state = root_trajectory(solved_roots, solved, given, where)
    # world space: poses and roots to world axes, one launch over all tracks' returned rows -- everything behind reads the world scene
    if opts.world is not None:
        shown, roots = camera_to_world_rows(out, roots, root_state, opts.world, lens)
    # filters: what is returned is the poses and roots, or the same filtered
    if opts.pose_filter is not None:
        shown = one_euro(shown, lens, out_rate, opts.pose_filter)
    poses = list(torch.split(shown, sizes, 0))
    placed = ()
    if camera is not None:
        if opts.root_filter is not None:
            roots = one_euro(roots, lens, out_rate, opts.root_filter, state=root_state)
        placed = (list(torch.split(roots, sizes, 0)), list(torch.split(root_state, sizes, 0)))
    result = _returned(poses, placed, table, model_lens, given, return_valid, repair_joints is not None)
    # rotations: the quaternions of the RETURNED poses, one launch over all tracks' rows, appended behind whatever the call returns
    if opts.rotations is not None:
        turned = joint_rotations(shown, opts.rotations)
        more = (list(torch.split(turned[0], sizes, 0)),) + ((list(torch.split(turned[2], sizes, 0)),) if opts.rotations.return_global else ())
        result = (result if isinstance(result, tuple) else (result,)) + more
    return result


def _assembled_tracks(model, config, tracks, resolutions, mask_stride, flip, keyframes_only, reuse_frames, batch_size, root_relative, depth, lengths,
                      graph, valid, fps, out_fps, model_fps, repair_joints, keypoints, camera, min_root_joints, smooth, bones, rotations, interpolation):
    """The part of ``predict_tracks`` up to the assembly, shared with ``views.predict_views``: the options' checks, the front (undistort,
    keypoint map, repair, normalise or resample), the windows, the forwards and uu3d_assemble_tracks -- the arguments as ``predict_tracks``
    takes them -> a namespace: ``opts`` (``options.StageOptions``), ``table`` (``table.source``: the undistorted, mapped raw points and
    the per-joint used flags, with ``camera``), ``given`` / ``lens`` / ``model_lens`` (frames given, returned and on the model's grid, per
    track), ``rates`` (None without ``fps``), ``mask_stride``, ``out`` (the assembled poses of all tracks, (sum(lens), J, 3)) and what a
    second assembly at other frame times needs (``assemble``, ``plan_at``, ``frame_idx``, ``rows``, ``stride``)."""
    # options: the refusals shared with a live session (``options.stage_options``), then the ones only this call has
    opts = stage_options(config, len(tracks), "track", root_relative, keypoints, camera, min_root_joints, smooth, bones, repair_joints, fps, out_fps,
                         interpolation=interpolation, rotations=rotations)
    if opts.keypoints is not None:
        check_keypoint_inputs(opts.keypoints, [_shape(t)[1] if len(_shape(t)) == 3 else -1 for t in tracks])
    if fps is not None and keyframes_only:
        raise ValueError("fps and keyframes_only exclude each other: for a detector that ran on every k-th frame pass the given frames with "
                         "fps=video_rate / k and out_fps=video_rate")
    if valid is not None and not model.has_strided_input:
        raise ValueError("valid needs a model with strided input: a missing frame becomes the learned masked token, which this model does not have")
    check_repair_joints(repair_joints, valid)
    check_valid(valid, [len(t) for t in tracks], joints=_shape(tracks[0])[1] if len(tracks) and len(_shape(tracks[0])) == 3 else None)
    cfg = config.copy()
    if mask_stride is None:
        mask_stride = default_mask_stride(cfg)
    cfg.MASK_STRIDE = mask_stride
    flip = bool(cfg.EVAL_FLIP) if flip is None else bool(flip)
    if keyframes_only and mask_stride is None:
        raise ValueError("keyframes_only needs a mask stride")
    # table: the given frames -> the pose table on the model's time grid; ``lens``: returned frames per track
    given = np.array([len(t) for t in tracks], np.int64)
    front = dict(valid=valid, repair_joints=repair_joints, keypoints=opts.keypoints, model=model, keep_source=camera is not None,
                 distortion=opts.lens)
    rates = None
    if fps is None:
        table, lens = pose_table(tracks, model.device, resolutions, int(mask_stride) if keyframes_only else 0, lengths, **front)
        model_lens = lens
    else:
        rates = frame_rates(fps, len(tracks))
        table, model_lens, _ = resampled_pose_table(tracks, model.device, rates, resolutions, model_fps=model_fps, **front)
        lens, positions = output_positions(given, rates, rates if out_fps is None else out_fps, model_fps)
    # windows + forward: the raw predictions of the windows that are run, and the row of each frame's window among them (-1: not run)
    raw, frame_idx, rows = _predicted_windows(model, cfg, table, mask_stride, flip, batch_size, depth, graph, reuse_frames)
    # assemble plan: which two predicted frames every returned frame is read from, and how
    stride = ev.prediction_stride(cfg)
    cubic = opts.interpolation == "cubic" and stride is not None and stride > 1      # (every frame predicted: nothing lies between keyframes)
    plan_at = evaluation.keyframe_plan_cubic_at if cubic else evaluation.keyframe_plan_at
    if fps is not None:
        plan = plan_at(frame_idx, 1 if stride is None else stride, positions, rows=rows)
    elif cubic:
        plan = evaluation.keyframe_plan_cubic(frame_idx, stride, rows=rows)
    elif stride is None:
        plan = rows, rows, np.zeros(len(rows), np.float64)
    else:
        plan = evaluation.keyframe_plan(frame_idx, stride, rows=rows)[:3]

    def assemble(plan):                                               # (a cubic plan has five arrays, a linear one three)
        return (assemble_tracks_cubic if cubic else assemble_tracks)(raw[0], raw[1] if flip else None, *plan, flip_order=cfg.AUGM_FLIP_KEYPOINT_ORDER,
                                                                     root=int(cfg.ROOT_KEYTPOINT) if root_relative else -1)
    out = assemble(plan)
    return types.SimpleNamespace(opts=opts, table=table, given=given, lens=lens, model_lens=model_lens, rates=rates, mask_stride=mask_stride,
                                 out=out, assemble=assemble, plan_at=plan_at, frame_idx=frame_idx, rows=rows, stride=stride)


def _predicted_windows(model, cfg, table, mask_stride, flip, batch_size, depth, graph, reuse_frames):
    """One window per frame of ``table``, in table order (position p is table row p); the ones ``eval.needed_windows`` keeps go through
    ``eval.predict_windows``' pipeline -> (raw predictions (plain, flipped), the frame index of every window, its row among the raw
    predictions or -1)."""
    gen = SequenceGenerator(table, seq_len=cfg.SEQUENCE_LENGTH, target_frame_rate=50, subsample=1, stride=cfg.SEQUENCE_STRIDE,
                            padding_type=cfg.PADDING_TYPE, flip_augment=False, flip_lr_indices=cfg.AUGM_FLIP_KEYPOINT_ORDER,
                            mask_stride=mask_stride, stride_mask_align_global=True, rand_shift_stride_mask=False, shuffle=False)
    desc = gen.descriptors()
    run = np.flatnonzero(ev.needed_windows(desc[:, 1], cfg))
    raw = ev._predict_windows_raw(model, gen, desc[run], int(batch_size or cfg.BATCH_SIZE), flip, depth, graph,
                                  bool(reuse_frames) and bool(model.arch.compiled_dims))
    rows = np.full(len(desc), -1, np.int64)
    rows[run] = np.arange(len(run))
    return raw, desc[:, 1], rows


def _returned(poses, placed, table, model_lens, given, return_valid, joint_state):
    """The return value of ``predict_tracks``: ``poses``; with ``return_valid`` (poses, flags) -- the table's per-frame flags on the model's
    grid, all True where it has none -- or, with ``repair_joints``, (poses, flags, joint_state); with ``camera`` the two lists of
    ``placed`` (roots, root_state) are appended to whichever it is."""
    import torch
    if not return_valid:
        return (poses,) + placed if placed else poses
    flags = table.valid.view(torch.bool) if table.valid is not None else torch.ones((int(model_lens.sum()),), dtype=torch.bool, device=poses[0].device)
    flags = list(torch.split(flags, [int(n) for n in model_lens], 0))
    if not joint_state:
        return (poses, flags) + placed
    return (poses, flags, list(torch.split(table.joint_state, [int(n) for n in given], 0))) + placed


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
    add_track_options(p, False, "resolution")
    p.add_argument("--mask_stride", type=int, default=None, help="input stride s_in (default: the config's first MASK_STRIDE)")
    p.add_argument("--keyframes_only", action="store_true",
                   help="the arrays hold frames 0, s_in, 2 s_in, ... only; a track of K keyframes is taken to have (K - 1) * s_in + 1 frames")
    add_track_options(p, False, "mask_missing", "repair_joints", "min_score", "fps", "out_fps", "keypoints", "camera", "min_root_joints", "smooth",
                      "smooth_root", "bones")
    args = p.parse_args(argv)
    if args.smooth_root is not None and args.camera is None:
        p.error("--smooth_root needs --camera: without it no roots are written")
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
    ms = default_mask_stride(config) if args.mask_stride is None else args.mask_stride
    lengths = None
    if args.keyframes_only:
        if ms is None:
            raise SystemExit("--keyframes_only needs a mask stride")
        lengths = [(len(t) - 1) * int(ms) + 1 for t in tracks]
    options = track_keywords(args, config, names, joint_flags, live=False)
    model = _load_model(config, args.weights)
    poses = predict_tracks(model, config, tracks, resolutions=None if args.resolution is None else tuple(args.resolution), mask_stride=ms,
                           keyframes_only=args.keyframes_only, lengths=lengths, **options)
    arrays = {}
    if "camera" in options:
        poses, roots, root_state = poses
        arrays.update({k + "__root": r.detach().cpu().numpy() for k, r in zip(names, roots)})
        arrays.update({k + "__root_state": r.detach().cpu().numpy() for k, r in zip(names, root_state)})
    arrays.update({k: np.asarray(p.detach().cpu().numpy(), np.float32) for k, p in zip(names, poses)})
    np.savez(args.output, **arrays)
    print(f"wrote {args.output}: {len(names)} tracks, {sum(int(p.shape[0]) for p in poses)} frames", flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
