"""GPU: the launch tables of a StreamSession per option set, by name and in order, with h36m_81 at mask stride 4, slots = 2, lookahead = 2.
No session pushes anything: each is built, read, finished once with no slot chosen (the sessions without ``fps``) and closed.  Pinned per
option set: the library functions of ``_push_before``, ``_tick_steps`` (a Python step shows as "forward"), ``_push_after``,
``[_reset_call] + _reset_more`` and, after one ``finish([])``, ``_drain_steps`` and the resets again; how many buffers a push returns;
``captures`` (1, then 2); and which of the public buffers are one and the same tensor ("same": the names that share an object, one group
per shared object): a stage that moves, drops or doubles a launch, or re-points a property, fails here by name."""
import pytest

from tests.tracks_util import _model

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
MS, T, A = 4, 2, 2
INTRINSICS = (1150.0, 1148.5, 500.25, 499.0)


def _options(name):
    from uplift_upsample_3dhpe_amd import predict
    world = predict.Camera(*INTRINSICS, orientation=(0.81, -0.53, 0.2, 0.15), translation=(1.8, 4.9, 1.6))
    pair = (predict.OneEuro(1.0, 0.5, 1.0), predict.OneEuro(0.8, 0.3, 1.0))
    five = dict(bones="track", camera=world, smooth=pair, rotations=True)
    return {"none": {}, "bones": dict(bones="track"), "camera": dict(camera=INTRINSICS), "world": dict(camera=world),
            "smooth_camera": dict(smooth=pair, camera=INTRINSICS), "rotations": dict(rotations=True), "five": five,
            "fps_five": dict(fps=30, **five), "detections_camera_smooth": dict(detections=2, camera=INTRINSICS, smooth=pair)}[name]


CASES = ("none", "bones", "camera", "world", "smooth_camera", "rotations", "five", "fps_five", "detections_camera_smooth")


def _names(steps):
    return ["forward" if args is None else fn.__name__ for fn, args in steps]


def _same(s):
    """The public buffers that are one tensor object: sorted groups of names (a name whose property raises AttributeError is left out)."""
    result = s._result
    named = [("push[0]", lambda: result[0]), ("push[2]", lambda: result[2] if s.cameras is not None else None)]
    named += [(p, lambda p=p: getattr(s, p)) for p in ("raw_poses", "camera_poses", "fixed_poses", "raw_roots", "camera_roots")]
    groups = {}
    for name, get in named:
        try:
            t = get()
        except AttributeError:
            continue
        if t is not None:
            groups.setdefault(id(t), []).append(name)
    return sorted(sorted(g) for g in groups.values() if len(g) > 1)


def _observe(name):
    from uplift_upsample_3dhpe_amd import stream
    cfg, arch, w, model = _model("h36m_81")
    options = _options(name)
    s = stream.StreamSession(model, cfg, slots=T, resolutions=(1000, 1002), mask_stride=MS, flip=True, lookahead=A, **options)
    try:
        seen = {"result": len(s._result), "captures": [s.captures], "push_before": _names(s._push_before), "tick": _names(s._tick_steps),
                "push_after": _names(s._push_after), "reset": _names([s._reset_call] + s._reset_more), "same": _same(s)}
        if s.cameras is not None and s.world is None:
            assert s.raw_poses is s.camera_poses and s.raw_roots is s.camera_roots
        if s.bones is None and s.pose_filter is None and s.world is None:
            assert s._result[0] is s.raw_poses
        if "fps" not in options:
            rows = s.finish([])
            assert len(rows) == len(s._result) and all(tuple(r.shape[:2]) == (T, A) for r in rows)
            seen["captures"].append(s.captures)
            seen["drain"] = _names(s._drain_steps)
            seen["reset_after_finish"] = _names([s._reset_call] + s._reset_more)
            seen["same_after_finish"] = _same(s)
        assert s.check_range() is False
    finally:
        s.close()
    return seen


# per option set what _observe returns: the tables by name, the length of a push's result, captures, the shared buffers
EXPECTED = {
    "none": {
        "result": 2,
        "captures": [1, 2],
        "push_before": [],
        "tick": ["uu3d_stream_stage", "uu3d_frame_features", "uu3d_stream_commit", "forward", "uu3d_stream_emit"],
        "push_after": [],
        "reset": ["uu3d_stream_reset"],
        "same": [["push[0]", "raw_poses"]],
        "drain": ["uu3d_stream_drain_commit", "forward", "uu3d_stream_emit", "uu3d_stream_drain_file"],
        "reset_after_finish": ["uu3d_stream_reset", "uu3d_stream_drain_reset"],
        "same_after_finish": [["push[0]", "raw_poses"]],
    },
    "bones": {
        "result": 2,
        "captures": [1, 2],
        "push_before": [],
        "tick": ["uu3d_stream_stage", "uu3d_frame_features", "uu3d_stream_commit", "forward", "uu3d_stream_emit", "uu3d_stream_bones"],
        "push_after": [],
        "reset": ["uu3d_stream_reset", "uu3d_stream_bones_reset"],
        "same": [["fixed_poses", "push[0]"]],
        "drain": ["uu3d_stream_drain_commit", "forward", "uu3d_stream_emit", "uu3d_stream_bones", "uu3d_stream_drain_file"],
        "reset_after_finish": ["uu3d_stream_reset", "uu3d_stream_bones_reset", "uu3d_stream_drain_reset"],
        "same_after_finish": [["fixed_poses", "push[0]"]],
    },
    "camera": {
        "result": 4,
        "captures": [1, 2],
        "push_before": [],
        "tick": ["uu3d_stream_stage", "uu3d_frame_features", "uu3d_stream_commit", "forward", "uu3d_stream_emit", "uu3d_stream_root"],
        "push_after": [],
        "reset": ["uu3d_stream_reset", "uu3d_stream_root_reset"],
        "same": [["camera_poses", "push[0]", "raw_poses"], ["camera_roots", "push[2]", "raw_roots"]],
        "drain": ["uu3d_stream_drain_commit", "forward", "uu3d_stream_emit", "uu3d_stream_root_drain", "uu3d_stream_drain_file"],
        "reset_after_finish": ["uu3d_stream_reset", "uu3d_stream_root_reset", "uu3d_stream_drain_reset"],
        "same_after_finish": [["camera_poses", "push[0]", "raw_poses"], ["camera_roots", "push[2]", "raw_roots"]],
    },
    "world": {
        "result": 4,
        "captures": [1, 2],
        "push_before": [],
        "tick": ["uu3d_stream_stage", "uu3d_frame_features", "uu3d_stream_commit", "forward", "uu3d_stream_emit", "uu3d_stream_root",
                 "uu3d_camera_to_world"],
        "push_after": [],
        "reset": ["uu3d_stream_reset", "uu3d_stream_root_reset"],
        "same": [["push[0]", "raw_poses"], ["push[2]", "raw_roots"]],
        "drain": ["uu3d_stream_drain_commit", "forward", "uu3d_stream_emit", "uu3d_stream_root_drain", "uu3d_camera_to_world",
                  "uu3d_stream_drain_file"],
        "reset_after_finish": ["uu3d_stream_reset", "uu3d_stream_root_reset", "uu3d_stream_drain_reset"],
        "same_after_finish": [["push[0]", "raw_poses"], ["push[2]", "raw_roots"]],
    },
    "smooth_camera": {
        "result": 4,
        "captures": [1, 2],
        "push_before": [],
        "tick": ["uu3d_stream_stage", "uu3d_frame_features", "uu3d_stream_commit", "forward", "uu3d_stream_emit", "uu3d_stream_root",
                 "uu3d_stream_one_euro", "uu3d_stream_one_euro"],
        "push_after": [],
        "reset": ["uu3d_stream_reset", "uu3d_stream_root_reset", "uu3d_stream_one_euro_reset", "uu3d_stream_one_euro_reset"],
        "same": [["camera_poses", "raw_poses"], ["camera_roots", "raw_roots"]],
        "drain": ["uu3d_stream_drain_commit", "forward", "uu3d_stream_emit", "uu3d_stream_root_drain", "uu3d_stream_one_euro", "uu3d_stream_one_euro",
                  "uu3d_stream_drain_file"],
        "reset_after_finish": ["uu3d_stream_reset", "uu3d_stream_root_reset", "uu3d_stream_one_euro_reset", "uu3d_stream_one_euro_reset",
                               "uu3d_stream_drain_reset"],
        "same_after_finish": [["camera_poses", "raw_poses"], ["camera_roots", "raw_roots"]],
    },
    "rotations": {
        "result": 3,
        "captures": [1, 2],
        "push_before": [],
        "tick": ["uu3d_stream_stage", "uu3d_frame_features", "uu3d_stream_commit", "forward", "uu3d_stream_emit", "uu3d_joint_rotations"],
        "push_after": [],
        "reset": ["uu3d_stream_reset", "uu3d_joint_rotations_reset"],
        "same": [["push[0]", "raw_poses"]],
        "drain": ["uu3d_stream_drain_commit", "forward", "uu3d_stream_emit", "uu3d_joint_rotations", "uu3d_stream_drain_file"],
        "reset_after_finish": ["uu3d_stream_reset", "uu3d_joint_rotations_reset", "uu3d_stream_drain_reset"],
        "same_after_finish": [["push[0]", "raw_poses"]],
    },
    "five": {
        "result": 5,
        "captures": [1, 2],
        "push_before": [],
        "tick": ["uu3d_stream_stage", "uu3d_frame_features", "uu3d_stream_commit", "forward", "uu3d_stream_emit", "uu3d_stream_bones",
                 "uu3d_stream_root", "uu3d_camera_to_world", "uu3d_stream_one_euro", "uu3d_stream_one_euro", "uu3d_joint_rotations"],
        "push_after": [],
        "reset": ["uu3d_stream_reset", "uu3d_stream_root_reset", "uu3d_stream_one_euro_reset", "uu3d_stream_one_euro_reset",
                  "uu3d_stream_bones_reset", "uu3d_joint_rotations_reset"],
        "same": [["camera_poses", "fixed_poses"]],
        "drain": ["uu3d_stream_drain_commit", "forward", "uu3d_stream_emit", "uu3d_stream_bones", "uu3d_stream_root_drain", "uu3d_camera_to_world",
                  "uu3d_stream_one_euro", "uu3d_stream_one_euro", "uu3d_joint_rotations", "uu3d_stream_drain_file", "uu3d_stream_drain_file"],
        "reset_after_finish": ["uu3d_stream_reset", "uu3d_stream_root_reset", "uu3d_stream_one_euro_reset", "uu3d_stream_one_euro_reset",
                               "uu3d_stream_bones_reset", "uu3d_joint_rotations_reset", "uu3d_stream_drain_reset"],
        "same_after_finish": [["camera_poses", "fixed_poses"]],
    },
    "fps_five": {
        "result": 5,
        "captures": [1],
        "push_before": ["uu3d_stream_source_push"],
        "tick": ["uu3d_stream_resample_stage", "uu3d_frame_features", "uu3d_stream_commit", "forward", "uu3d_stream_emit",
                 "uu3d_stream_file_keyframe"],
        "push_after": ["uu3d_stream_timed_emit", "uu3d_stream_bones", "uu3d_stream_root", "uu3d_camera_to_world", "uu3d_stream_one_euro",
                       "uu3d_stream_one_euro", "uu3d_joint_rotations"],
        "reset": ["uu3d_stream_rate_reset", "uu3d_stream_root_reset", "uu3d_stream_one_euro_reset", "uu3d_stream_one_euro_reset",
                  "uu3d_stream_bones_reset", "uu3d_joint_rotations_reset"],
        "same": [["camera_poses", "fixed_poses"]],
    },
    "detections_camera_smooth": {
        "result": 4,
        "captures": [1, 2],
        "push_before": [],
        "tick": ["uu3d_stream_associate", "uu3d_stream_reset", "uu3d_stream_root_reset", "uu3d_stream_one_euro_reset", "uu3d_stream_one_euro_reset",
                 "uu3d_stream_stage_valid", "uu3d_frame_features", "uu3d_stream_commit_valid", "forward", "uu3d_stream_emit", "uu3d_stream_root",
                 "uu3d_stream_one_euro", "uu3d_stream_one_euro"],
        "push_after": [],
        "reset": ["uu3d_stream_reset", "uu3d_stream_root_reset", "uu3d_stream_one_euro_reset", "uu3d_stream_one_euro_reset", "uu3d_associate_reset"],
        "same": [["camera_poses", "raw_poses"], ["camera_roots", "raw_roots"]],
        "drain": ["uu3d_stream_drain_commit", "forward", "uu3d_stream_emit", "uu3d_stream_root_drain", "uu3d_stream_one_euro", "uu3d_stream_one_euro",
                  "uu3d_stream_drain_file"],
        "reset_after_finish": ["uu3d_stream_reset", "uu3d_stream_root_reset", "uu3d_stream_one_euro_reset", "uu3d_stream_one_euro_reset",
                               "uu3d_associate_reset", "uu3d_stream_drain_reset"],
        "same_after_finish": [["camera_poses", "raw_poses"], ["camera_roots", "raw_roots"]],
    },
}


@pytest.mark.parametrize("name", CASES)
def test_launch_tables_by_name(name):
    seen, want = _observe(name), EXPECTED[name]
    for key in sorted(set(seen) | set(want)):
        assert seen.get(key) == want.get(key), (name, key, seen.get(key), want.get(key))
