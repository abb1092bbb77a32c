"""The options of the track stages, checked once for ``predict.predict_tracks`` (``per="track"``) and ``stream.StreamSession``
(``per="slot"``): ``stage_options`` runs the refusals the two share -- none of them touches a model or a device -- and returns what the
stages take.  A refusal only one of the two has stays with it (``fps`` with ``keyframes_only`` offline; the "together with out_fps"
family, ``MAX_LIVE_REPAIR`` and the one camera of ``detections`` live).  Wraps no library call."""
import collections

from .bones import check_bones
from .camera import split_cameras, world_rows
from .keypoints import keypoint_map
from .rotations import check_rotations
from .roots import DEFAULT_MIN_ROOT_JOINTS, MAX_ROOT_JOINTS, check_cameras, check_min_root_joints
from .smooth import check_causal, check_smooth
from .validity import check_repair_joints

# cameras: (count, 4) float64 or None; min_root_joints: the checked int (a session without a camera: None); pose_filter / root_filter: a
# ``OneEuro`` or None each; rigid: None or (skeleton, (count, J) lengths or None for "track"); keypoints: a ``KeypointMap`` or None;
# rotations: a ``Rotations`` or None; interpolation: "linear" or "cubic" (of the offline call; a session checks its own with ``check_interpolation``);
# lens: None or the (count, 10) float64 rows of uu3d_undistort_points -- ``camera`` was a ``Camera`` with distortion, or one per track / slot;
# world: None or the (count, 7) float64 rows of uu3d_camera_to_world -- ``camera`` was a ``Camera`` with extrinsics, or one per track / slot
StageOptions = collections.namedtuple("StageOptions", "cameras min_root_joints pose_filter root_filter rigid keypoints rotations interpolation lens world")
INTERPOLATIONS = ("linear", "cubic")

OUT_FPS_NEEDS_FPS = {"track": "out_fps needs fps: the rate the tracks were filmed at", "slot": "out_fps needs fps: the rate of the pushed frames"}


def check_interpolation(interpolation):
    """``predict_tracks(interpolation=...)`` / ``StreamSession(interpolation=...)``: how a returned frame between two predicted ones is
    read -> the checked name."""
    if not isinstance(interpolation, str) or interpolation not in INTERPOLATIONS:
        raise ValueError(f"interpolation must be one of {', '.join(repr(n) for n in INTERPOLATIONS)}, got {interpolation!r}")
    return interpolation


def stage_options(config, count, per, root_relative, keypoints, camera, min_root_joints, smooth, bones, repair_joints, fps, out_fps,
                  interpolation="linear", rotations=None):
    """``count`` tracks (``per="track"``) or slots (``per="slot"``) of a model of ``config``; the other arguments as ``predict_tracks`` and
    ``StreamSession`` take them -> a ``StageOptions``.  Every refusal is a ValueError in the words of the stage's own check.
    ``min_root_joints``: a session passes None for "not given" -- the default with a camera, and anything else without one is refused (it
    is a parameter of the root solve); the offline call has the default in its signature and passes what it got.
    ``repair_joints`` is checked for its type only: whether it has the ``valid`` it needs is the caller's to say.
    ``interpolation``: the offline call's (``check_interpolation``); a session does not pass it here and checks its own.
    ``camera`` may be a ``camera.Camera`` or a list of them: ``split_cameras`` takes it apart before ``check_cameras`` sees it, and
    ``world_rows`` reads its extrinsics once both have passed it."""
    interpolation = check_interpolation(interpolation)
    pose_filter, root_filter = check_smooth(smooth, camera is not None)
    if per == "slot":
        check_causal(pose_filter, root_filter)                       # (a zero-lag filter needs the whole track: offline only)
    rigid = check_bones(bones, count, config.NUM_KEYPOINTS, int(config.ROOT_KEYTPOINT) if root_relative else None, per=per)
    cameras = lens = world = None
    if camera is not None:
        given = camera
        camera, lens = split_cameras(camera, count, per=per)
        cameras = check_cameras(camera, count, per=per)
        world = world_rows(given, count)
        min_root_joints = check_min_root_joints(DEFAULT_MIN_ROOT_JOINTS if min_root_joints is None and per == "slot" else min_root_joints)
        if int(config.NUM_KEYPOINTS) > MAX_ROOT_JOINTS:
            raise ValueError(f"camera needs a model of at most {MAX_ROOT_JOINTS} joints, this one has {int(config.NUM_KEYPOINTS)}")
    elif per == "slot" and min_root_joints is not None:
        raise ValueError("min_root_joints needs camera=(fx, fy, cx, cy): it is a parameter of the root solve")
    if keypoints is not None:
        keypoints = keypoint_map(keypoints, config.NUM_KEYPOINTS)
    if fps is None and out_fps is not None:
        raise ValueError(OUT_FPS_NEEDS_FPS[per])
    check_repair_joints(repair_joints, "finite")
    return StageOptions(cameras, min_root_joints, pose_filter, root_filter, rigid, keypoints, check_rotations(rotations, config.NUM_KEYPOINTS),
                        interpolation, lens, world)
