"""Host side of the device evaluation report: the gather plan that replaces interpolate_between_keyframes (evaluation.keyframe_plan)
and the assembly of the report from a sums table (evaluation.report_from_sums), against the host functions and the fixtures generated
from the reference's own metrics.py / action_wise_eval.py."""
import os

import numpy as np
import pytest

from uplift_upsample_3dhpe_amd import evaluation as E
from tests import util

G = os.path.join(util.ROOT, "tests", "golden")


def _apply(pred, plan):
    left, right, w, _ = plan
    w = w.reshape((-1,) + (1,) * (pred.ndim - 1))
    return np.where(w == 0, pred[left], pred[left] * (1.0 - w) + pred[right] * w)


def test_plan_reproduces_the_reference_interpolation():
    g = np.load(os.path.join(G, "metrics_expected.npz"))
    for stride in (5, 10):
        plan = E.keyframe_plan(g[f"frame_indices_{stride}"], stride)
        assert np.array_equal(plan[3], g[f"keyframes_{stride}"])
        assert np.abs(_apply(g["pred"], plan) - g[f"interp_{stride}"]).max() < 1e-12


def _random_indices(rng, videos, step):
    parts = []
    for _ in range(videos):
        n = int(rng.integers(1, 60))
        if rng.random() < 0.25:
            n = 1                                                    # single-frame videos
        first = int(rng.integers(0, 12)) * step if rng.random() < 0.5 else int(rng.integers(0, 40))
        parts.append(first + step * np.arange(n))
    return np.concatenate(parts)


@pytest.mark.parametrize("step", [1, 2, 3])
@pytest.mark.parametrize("stride", [5, 10])
def test_plan_equals_the_host_loop_on_random_videos(step, stride):
    """A subsampled frame step, videos that end between keyframes, single-frame videos, videos that start off-keyframe; the video
    boundary is a drop (or repeat) of the frame index."""
    rng = np.random.default_rng(100 * step + stride)
    for trial in range(20):
        idx = _random_indices(rng, int(rng.integers(1, 12)), step)
        pred = rng.normal(size=(len(idx), 4, 3))
        want, key = E.interpolate_between_keyframes(pred, idx, stride)
        plan = E.keyframe_plan(idx, stride)
        assert np.array_equal(plan[3], key)
        assert np.array_equal(_apply(pred, plan), want), trial       # the same formula on the same numbers
        assert np.all(plan[2][plan[0] == plan[1]] == 0) and np.all((plan[2] >= 0) & (plan[2] < 1))
        per_frame = E.keyframe_plan(idx, np.full(len(idx), stride))  # per-frame stride array, as evaluate_predictions passes
        assert all(np.array_equal(a, b) for a, b in zip(plan, per_frame))


def test_plan_in_rows_of_the_forwarded_predictions():
    idx = np.concatenate([np.arange(0, 23), np.arange(0, 11)])
    key = idx % 5 == 0
    rows = np.full(len(idx), -1)
    rows[key] = np.arange(key.sum())
    pred = np.random.default_rng(0).normal(size=(len(idx), 3, 3))
    left, right, w, k = E.keyframe_plan(idx, 5, rows=rows)
    assert np.array_equal(k, key) and left.min() >= 0 and right.max() < key.sum()
    want, _ = E.interpolate_between_keyframes(pred, idx, 5)
    assert np.array_equal(_apply(pred[key], (left, right, w, k)), want)
    # a video that starts in front of its first keyframe keeps its own prediction there: that row must have been forwarded
    idx2 = np.concatenate([np.arange(0, 12), np.arange(3, 14)])
    key2 = idx2 % 5 == 0
    rows2 = np.full(len(idx2), -1)
    rows2[key2] = np.arange(key2.sum())
    with pytest.raises(ValueError):
        E.keyframe_plan(idx2, 5, rows=rows2)
    rows2[12:14] = key2.sum() + np.arange(2)                        # frames 3 and 4 of the second video forwarded as well
    left, right, w, _ = E.keyframe_plan(idx2, 5, rows=rows2)
    assert left[12] == right[12] == key2.sum() and w[12] == 0
    assert E.keyframe_plan(np.zeros(0, int), 5)[0].shape == (0,)


def _sums_table(per_joint, actions, num_actions, select=None):
    """What uu3d_error_sums computes: per (action | all, metric) the sum of the entries >= 0 and their count, in metres."""
    t = np.zeros((num_actions + 1, 3, 2))
    sel = np.ones(len(actions), bool) if select is None else select
    for a in range(num_actions + 1):
        rows = sel & ((actions == a) if a < num_actions else True)
        for m in range(3):
            e = per_joint[m][rows]
            t[a, m] = e[e >= 0].sum(), (e >= 0).sum()
    return t


def test_report_from_sums_matches_the_reference_reports():
    g = np.load(os.path.join(G, "metrics_expected.npz"))
    pred, gt, root, actions = g["pred"], g["gt"], int(g["root"]), g["actions"]
    per_joint = [g["mpjpe_jp"], g["nmpjpe_root_jp"], g["pmpjpe_jp"]]
    keys = ("mpjpe", "nmpjpe", "pampjpe")
    frame, avg, per = E.report_from_sums(_sums_table(per_joint, actions, 15))
    assert np.abs(np.array([frame[k] for k in keys]) - g["aw_frame"]).max() < 1e-5          # millimetres
    assert np.abs(np.array([avg[k] for k in keys]) - g["aw_average"]).max() < 1e-5
    assert list(per.keys()) == [str(a) for a in g["aw_actions"]] == E.H36M_ACTIONS
    assert np.abs(np.array([[d[k] for k in keys] for d in per.values()]) - g["aw_per_action"]).max() < 1e-5
    fr = E.report_from_sums(_sums_table(per_joint, actions, 0), action_wise=False)
    assert list(fr) == list(E.METRICS)
    assert np.abs(np.array([fr[k] for k in keys]) - g["frame_wise"]).max() < 1e-5
    # against the host functions, with a row selection (the KEYFRAMES report) and an action without poses
    sel = (np.arange(len(actions)) // 15) % 2 == 0                  # every other pose of each action
    sel &= actions != 4
    want = E.h36_action_wise_eval(pred[sel], gt[sel], actions[sel], root)
    got = E.report_from_sums(_sums_table(per_joint, actions, 15, sel))
    for k in keys:
        assert abs(got[0][k] - want[0][k]) < 1e-5
        assert np.isnan(got[1][k]) and np.isnan(want[1][k])          # the mean over actions of a report with an empty action
        for name in E.H36M_ACTIONS:
            assert (name == "Phoning") == bool(np.isnan(got[2][name][k]))
            if name != "Phoning":
                assert abs(got[2][name][k] - want[2][name][k]) < 1e-5


def test_device_metrics_flag_of_the_command_line():
    from uplift_upsample_3dhpe_amd import train as T
    assert T.parse_args(["--out_dir", "o"]).device_metrics is False
    assert T.parse_args(["--out_dir", "o", "--device_metrics"]).device_metrics is True
    assert "device_metrics" not in {a.dest for a in T.build_parser()._actions}          # the reference's own flags stay as they are
    import inspect
    for f in (T.run_train, T.Validation.__init__):
        assert inspect.signature(f).parameters["device_metrics"].default is False
