"""The command-line options that ``python -m uplift_upsample_3dhpe_amd.predict`` and ``... .stream`` share: declared once
(``add_track_options``; where the two programs word a help text differently, both wordings stand in ``TRACK_OPTIONS``), and turned into the
keywords of ``predict_tracks`` / ``replay_tracks`` once (``track_keywords``).  Wraps no library call."""
import numpy as np

from .keypoints import KEYPOINT_PRESETS, keypoint_map
from .rates import _rate_argument
from .roots import DEFAULT_MIN_ROOT_JOINTS, check_cameras, check_min_root_joints
from .smooth import OneEuro
from .validity import MAX_LIVE_REPAIR

_FILTER = dict(type=float, nargs=3, metavar=("MIN_CUTOFF", "BETA", "D_CUTOFF"), default=None)
# --NAME -> (what both programs declare, what only ``predict`` says, what only ``stream`` says): the keywords of ``add_argument``
TRACK_OPTIONS = {
    "resolution": (dict(type=float, nargs=2, metavar=("W", "H"), default=None,
                        help="image size in pixels of all tracks; without it the coordinates are taken as normalised already"), {}, {}),
    "mask_missing": (dict(action="store_true"),
                     dict(help="a frame with a NaN or Inf coordinate is a missed detection: never shown to the network, its pose is still predicted"),
                     dict(help="a frame with a NaN or Inf coordinate is a missed detection: the track grows by it, the network never sees it")),
    "repair_joints": (dict(type=int, default=None, metavar="G"),
                      dict(help="fill a joint that is missing for up to G consecutive frames from the nearest frames where it was seen; implies "
                                "--mask_missing"),
                      dict(help="fill a joint that is missing for up to G <= 32 consecutive frames from the nearest frames where it was seen, as "
                                "predict --repair_joints on the track so far; implies --mask_missing; not with --fps")),
    "min_score": (dict(type=float, default=None, metavar="S"),
                  dict(help="the arrays may be (T, J, 3) with the detector's score in the third channel: a joint counts as seen when score >= S"),
                  dict(help="with --repair_joints the arrays may be (T, J, 3) with the detector's score in the third channel: a joint counts as "
                            "seen when score >= S")),
    "fps": (dict(type=_rate_argument, default=None, metavar="F"),
            dict(help="frame rate of the tracks, a float or NUM/DEN (29.97, 30000/1001); without it they are taken at the model's rate"),
            dict(help="frame rate of the tracks, a float or NUM/DEN (29.97, 30000/1001); without it they are taken at the model's rate.  "
                      "--lookahead then counts frames of the tracks")),
    "out_fps": (dict(type=_rate_argument, default=None),
                dict(metavar="F", help="frame rate of the poses written (default: --fps)"),
                dict(metavar="G", help="rate of the poses written, a float or NUM/DEN (needs --fps): NAME then holds every pose the session emitted, "
                                       "in order (n_out, J, 3), and NAME_count the number each tick returned")),
    "keypoints": (dict(default=None, metavar="NAME", choices=sorted(KEYPOINT_PRESETS)),
                  dict(help="the joint layout of the arrays, (T, K, 2): mapped onto the model's joints on the device; --min_score then reads the "
                            "score channel of (T, K, 3) arrays, one score per detector joint"),
                  dict(help="the joint layout of the arrays, (T, K, 2): mapped onto the model's joints on the device; scores are then per detector "
                            "joint")),
    "camera": (dict(type=float, nargs=4, metavar=("FX", "FY", "CX", "CY"), default=None),
               dict(help="the camera's intrinsics in the units of the arrays (pixels with --resolution): the output gains <key>__root (T, 3), the "
                         "position of the skeleton's root in the camera's space, and <key>__root_state (T,) per track"),
               dict(help="the camera's intrinsics in the units of the arrays (pixels with --resolution): the output gains NAME__root (T, 3), the "
                         "position of the skeleton's root in the camera's space at every tick, and NAME__root_state (T,) per track; not with "
                         "--out_fps")),
    "min_root_joints": (dict(type=int, metavar="N"),
                        dict(default=DEFAULT_MIN_ROOT_JOINTS, help="the fewest observed joints a frame's root is solved from (with --camera)"),
                        dict(default=None, help=f"the fewest observed joints a frame's root is solved from (with --camera; default "
                                                f"{DEFAULT_MIN_ROOT_JOINTS})")),
    "smooth": (_FILTER,
               dict(help="pass the written poses through a One-Euro filter (Hz, 1 / unit speed, Hz) at the rate of the written frames; causal, it "
                         "lags"),
               dict(help="pass the poses of every tick through a live One-Euro filter (Hz, 1 / unit speed, Hz); not with --out_fps")),
    "smooth_root": (dict(_FILTER, help="the same for the roots (needs --camera)"), {}, {}),
    "bones": (dict(default=None, metavar="track|FILE.npy"),
              dict(help="constant bone lengths: 'track' gives every track its own mean lengths, FILE.npy holds a (J,) array of known lengths in "
                        "the poses' units, indexed by child joint"),
              dict(help="constant bone lengths: 'track' rebuilds every pose with the running mean lengths of its track so far, FILE.npy holds a "
                        "(J,) array of known lengths in the poses' units, indexed by child joint; not with --out_fps")),
}


def add_track_options(parser, live, *names):
    """Declares the named options of ``TRACK_OPTIONS`` on ``parser``, in the order given (the order of the program's --help): ``live``
    False for ``predict``, True for ``stream``."""
    for name in names:
        shared, offline, session = TRACK_OPTIONS[name]
        parser.add_argument("--" + name, **shared, **(session if live else offline))


def track_keywords(args, config, names, joint_flags, live):
    """The parsed options of ``TRACK_OPTIONS`` -> the keywords of ``predict_tracks`` (``live`` False) or ``replay_tracks`` (True): ``valid``
    / ``repair_joints``, ``keypoints``, ``fps`` / ``out_fps``, ``camera`` / ``min_root_joints``, ``smooth``, ``bones`` -- each only where its
    option was given.  ``names``: the keys of the input arrays; ``joint_flags``: what ``split_scores`` made of --min_score, or None.
    Anything wrong is a SystemExit naming the option."""
    kw = {}
    if joint_flags is not None:
        kw["valid"] = joint_flags
    elif args.mask_missing or args.repair_joints is not None:
        kw["valid"] = "finite"
    if args.repair_joints is not None:
        if live and not 1 <= args.repair_joints <= MAX_LIVE_REPAIR:
            raise SystemExit(f"--repair_joints must be in [1, {MAX_LIVE_REPAIR}]")
        kw["repair_joints"] = args.repair_joints
    if args.keypoints is not None:
        kw["keypoints"] = args.keypoints
    if args.out_fps is not None and args.fps is None:
        raise SystemExit("--out_fps needs --fps")
    kw.update({k: v for k, v in (("fps", args.fps), ("out_fps", args.out_fps)) if v is not None})
    if args.camera is not None:
        try:
            check_cameras(tuple(args.camera), 1)
            kw.update(camera=tuple(args.camera),
                      min_root_joints=check_min_root_joints(DEFAULT_MIN_ROOT_JOINTS if args.min_root_joints is None else args.min_root_joints))
        except ValueError as e:
            raise SystemExit(f"--camera: {e}") from None
        if any(k.endswith(("__root", "__root_state")) for k in names):
            raise SystemExit(f"{args.input}: a key ending in __root or __root_state would collide with the arrays --camera writes")
    kw.update(smooth_option(args))
    kw.update(bones_option(args, config.NUM_KEYPOINTS))
    return kw


def bones_option(args, J):
    """--bones of a command line -> the ``bones`` keyword ({} when it is not given): "track", or the (J,) array of an .npy file."""
    if getattr(args, "bones", None) is None:
        return {}
    if args.bones == "track":
        return {"bones": "track"}
    try:
        lengths = np.asarray(np.load(args.bones), np.float64)
    except (OSError, ValueError) as e:
        raise SystemExit(f"--bones: {args.bones} is neither 'track' nor a readable .npy file ({e})") from None
    if lengths.shape != (int(J),):
        raise SystemExit(f"--bones: {args.bones} holds an array of shape {lengths.shape}, expected ({int(J)},): one length per child joint")
    return {"bones": lengths}


def smooth_option(args):
    """--smooth / --smooth_root of a command line -> the ``smooth`` keyword ({} when neither is given)."""
    if args.smooth is None and args.smooth_root is None:
        return {}
    try:
        return {"smooth": (None if args.smooth is None else OneEuro(*args.smooth), None if args.smooth_root is None else OneEuro(*args.smooth_root))}
    except ValueError as e:
        raise SystemExit(f"--smooth / --smooth_root: {e}") from None


def split_scores(names, tracks, J, min_score, source="input"):
    """The arrays of the command line -> (list of (T, J, 2) tracks, per-joint flags or None).  With ``min_score`` = S an array may be
    (T, J, 3), the detector's score in the third channel: the joint is flagged when score >= S (a NaN score fails) and the score is
    stripped; a (T, J, 2) array next to it has every joint flagged.  Without it only (T, J, 2) passes."""
    for k, t in zip(names, tracks):
        if t.ndim != 3 or t.shape[1] != J or t.shape[2] not in ((2,) if min_score is None else (2, 3)):
            raise SystemExit(f"{source}[{k}] has shape {t.shape}, expected (T, {J}, 2)" + ("" if min_score is None else f" or (T, {J}, 3)"))
    if min_score is None:
        return tracks, None
    flags = [t[:, :, 2] >= min_score if t.shape[2] == 3 else np.ones(t.shape[:2], bool) for t in tracks]
    return [np.ascontiguousarray(t[:, :, :2]) for t in tracks], flags


def input_joints(config, keypoints):
    """The joint count of the command line's arrays -> (K, the keyword for ``predict_tracks`` / ``replay_tracks``)."""
    if keypoints is None:
        return config.NUM_KEYPOINTS, {}
    try:
        return keypoint_map(keypoints, config.NUM_KEYPOINTS).inputs, {"keypoints": keypoints}
    except ValueError as e:
        raise SystemExit(f"--keypoints: {e}") from None
