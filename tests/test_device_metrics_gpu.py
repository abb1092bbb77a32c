"""The evaluation report on the device (csrc/uu3d_metrics.h: uu3d_pose_errors / uu3d_error_sums, evaluation_device.py) against the
reference's own numbers (tests/golden/metrics_expected.npz, generated from its metrics.py / action_wise_eval.py) and against the host
restatement evaluation.py: per-joint MPJPE / N-MPJPE within 1e-9 m, P-MPJPE within 1e-8 m, every report entry within 1e-5 mm."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import uplift_upsample_3dhpe_amd as pkg
from tests import util

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
G = os.path.join(util.ROOT, "tests", "golden")
TOL_M = np.array([1e-9, 1e-9, 1e-8])          # metres: mpjpe, nmpjpe, pmpjpe per joint
TOL_MM = 1e-5                                 # millimetres: every entry of a report
KEYS = ("mpjpe", "nmpjpe", "pampjpe")


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host_errors(pred, gt, root):
    from uplift_upsample_3dhpe_amd import evaluation as E
    pred, gt = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    if gt.shape[-1] == 3:
        gt = np.concatenate([gt, np.ones(gt.shape[:-1] + (1,))], -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.stack([E.mpjpe(pred, gt, root, normalize=False), E.nmpjpe(pred, gt, root, alignment="root", normalize=False),
                         E.pmpjpe(pred, gt, normalize=False)], -1)


def _dev_errors(pred, gt, root, **kw):
    from uplift_upsample_3dhpe_amd import evaluation_device as ED
    err, sums = ED.pose_errors(_cuda(pred), _cuda(gt), root, **kw)
    torch.cuda.synchronize()
    return (None if err is None else err.cpu().numpy()), (None if sums is None else sums.cpu().numpy())


def _check_errors(got, want, label=""):
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.array_equal(got == -1.0, want == -1.0), label
    diff = np.abs(got - want).reshape(-1, 3).max(0)
    print(f"{label} per-joint max |device - host| (m): mpjpe {diff[0]:.3e} nmpjpe {diff[1]:.3e} pmpjpe {diff[2]:.3e}")
    assert np.all(diff < TOL_M), (label, diff)


def _sums_table(err, actions, num_actions, select=None):
    t = np.zeros((num_actions + 1, 3, 2))
    sel = np.ones(len(err), bool) if select is None else np.asarray(select, bool)
    for a in range(num_actions + 1):
        rows = sel & ((np.asarray(actions) == a) if a < num_actions else True)
        for m in range(3):
            e = err[rows][..., m]
            t[a, m] = e[e >= 0].sum(), (e >= 0).sum()
    return t


def _flatten(rep, prefix=""):
    if rep is None:
        return {prefix: None}
    if isinstance(rep, dict):
        out = {}
        for k, v in rep.items():
            out.update(_flatten(v, f"{prefix}/{k}"))
        return out
    if isinstance(rep, (tuple, list)):
        out = {}
        for i, v in enumerate(rep):
            out.update(_flatten(v, f"{prefix}[{i}]"))
        return out
    return {prefix: float(rep)}


def _check_reports(got, want, label="", skip=("seconds",)):
    a, b = _flatten(got), _flatten(want)
    assert list(a) == list(b), label                                 # same keys, same order of actions
    worst = 0.0
    for k in a:
        if k.endswith(skip):
            continue
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (label, k)
        elif np.isnan(b[k]):
            assert np.isnan(a[k]), (label, k)
        else:
            worst = max(worst, abs(a[k] - b[k]))
            assert abs(a[k] - b[k]) <= TOL_MM, (label, k, a[k], b[k])
    print(f"{label} report max |device - host| (mm): {worst:.3e}")


def _fixture_like(rng, gt3, invalid=0.1, root=6):
    """Predictions drawn as tests/golden/make_metrics_golden.py draws them: ground truth times a random scale, plus noise, plus a shift."""
    B, J = gt3.shape[:2]
    pred = gt3 * rng.uniform(0.8, 1.25, size=(B, 1, 1)) + rng.normal(0, 0.04, size=(B, J, 3)) + rng.normal(0, 0.5, size=(B, 1, 3))
    valid = (rng.uniform(size=(B, J)) > invalid).astype(np.float64)
    valid[:, root] = 1.0
    return pred, np.concatenate([gt3, valid[..., None]], -1)


def _smooth_videos(rng, lengths, J, first_frames=None):
    """Ground truth that moves smoothly inside each video (blends between anchor poses 20 frames apart), so that a prediction
    interpolated between keyframes stays a prediction of its frame.  -> gt3 (P, J, 3), frame_indices (P,)."""
    gts, idx = [], []
    for v, n in enumerate(lengths):
        knots = n // 20 + 2
        anchors = rng.normal(0, 0.35, size=(1, J, 3)) + np.cumsum(rng.normal(0, 0.08, size=(knots, J, 3)), 0)
        t = np.arange(n) / 20.0
        k = t.astype(int)
        w = (t - k)[:, None, None]
        gts.append(anchors[k] * (1 - w) + anchors[k + 1] * w)
        idx.append((0 if first_frames is None else first_frames[v]) + np.arange(n))
    return np.concatenate(gts), np.concatenate(idx)


def _fit_condition(pred, gt3):
    """min over the poses of (s2 + s3) / s1 of the cross-covariance of the similarity fit."""
    X0, Y0 = gt3 - gt3.mean(1, keepdims=True), pred - pred.mean(1, keepdims=True)
    X0 = X0 / np.sqrt((X0 ** 2).sum((1, 2)))[:, None, None]
    Y0 = Y0 / np.sqrt((Y0 ** 2).sum((1, 2)))[:, None, None]
    s = np.linalg.svd(np.einsum("bki,bkj->bij", X0, Y0), compute_uv=False)
    return float(((s[:, 1] + s[:, 2]) / s[:, 0]).min())


def test_against_the_reference_fixture():
    """The reference's own per-joint errors and reports.  The fixture's poses are float64, so they go in as float64 (inputs_f64)."""
    from uplift_upsample_3dhpe_amd import evaluation as E, evaluation_device as ED
    g = np.load(os.path.join(G, "metrics_expected.npz"))
    pred, gt, root, actions = g["pred"], g["gt"], int(g["root"]), g["actions"]
    want = np.stack([g["mpjpe_jp"], g["nmpjpe_root_jp"], g["pmpjpe_jp"]], -1)
    err, sums = _dev_errors(pred, gt, root, actions=actions.astype(np.int32), num_actions=15, want_sums=True)
    _check_errors(err, want, "reference fixture")
    assert np.array_equal(err[..., 0] == -1.0, gt[..., 3] <= 0)
    frame, avg, per = E.report_from_sums(sums)
    diffs = [np.abs(np.array([frame[k] for k in KEYS]) - g["aw_frame"]).max(), np.abs(np.array([avg[k] for k in KEYS]) - g["aw_average"]).max(),
             np.abs(np.array([[d[k] for k in KEYS] for d in per.values()]) - g["aw_per_action"]).max()]
    assert list(per.keys()) == [str(a) for a in g["aw_actions"]]
    _, sums0 = _dev_errors(pred, gt, root, want_errors=False, want_sums=True)
    fr = E.report_from_sums(sums0, action_wise=False)
    diffs.append(np.abs(np.array([fr[k] for k in KEYS]) - g["frame_wise"]).max())
    print("reference fixture reports max |device - reference| (mm): frame %.3e average %.3e per action %.3e frame-wise %.3e" % tuple(diffs))
    assert max(diffs) < TOL_MM
    # uu3d_error_sums on the error array gives the table of the fused call: to rounding here (float64 poses of 17 joints are tiled 60 to
    # a workgroup in the fused call, 64 in uu3d_error_sums, so the partial sums are cut differently) ...
    again = ED.error_sums(_cuda(err), actions=actions.astype(np.int32), num_actions=15).cpu().numpy()
    assert np.array_equal(again[..., 1], sums[..., 1]) and np.abs(again[..., 0] - sums[..., 0]).max() < 1e-12
    # ... and the same poses rounded to float32 (the product path: 64-pose tiles in both): agreement with the reference to the input
    # rounding, and the two tables bit for bit (the same sums in the same order; specific to 64-pose tiles, see include/uu3d.h)
    err32, sums32 = _dev_errors(pred.astype(np.float32), gt.astype(np.float32), root, actions=actions.astype(np.int32), num_actions=15, want_sums=True)
    assert np.abs(err32 - want).max() < 5e-7
    assert np.array_equal(ED.error_sums(_cuda(err32), actions=actions.astype(np.int32), num_actions=15).cpu().numpy(), sums32)


@pytest.mark.parametrize("stride", [5, 10])
def test_synthetic_run_against_the_host(stride):
    """Several videos, 15 actions, invalid joints, 20 011 poses (more than one workgroup per compute unit's worth of tiles, ragged tail),
    the interpolation fused into the load; float32 inputs as in the product."""
    from uplift_upsample_3dhpe_amd import evaluation as E, evaluation_device as ED
    rng = np.random.default_rng(7 + stride)
    lengths = [3001, 1, 4520, 777, 2999, 5003, 12, 3698]
    firsts = [0, 0, 0, 3, 0, stride * 3, 0, 0]                      # the fourth video starts in front of its first keyframe
    assert sum(lengths) == 20011
    gt3, idx = _smooth_videos(rng, lengths, 17, firsts)
    pred, gt = _fixture_like(rng, gt3)
    pred, gt = pred.astype(np.float32), gt.astype(np.float32)
    actions = np.repeat(np.arange(len(lengths)) % 15, lengths)
    actions = ((actions + np.arange(len(idx)) // 500) % 15).astype(np.int32)
    root = 6
    interp, key = E.interpolate_between_keyframes(pred.astype(np.float64), idx, stride)
    cond = _fit_condition(interp, gt[..., :3].astype(np.float64))
    print(f"stride {stride}: min (s2 + s3) / s1 = {cond:.3f}")
    assert cond > 0.1
    left, right, weight, k = E.keyframe_plan(idx, stride)
    assert np.array_equal(k, key)
    want = _host_errors(interp, gt, root)
    err, sums = _dev_errors(pred, gt, root, left=left, right=right, weight=weight, actions=actions, num_actions=15, want_sums=True)
    _check_errors(err, want, f"stride {stride}, all frames")
    _check_reports(E.report_from_sums(sums), E.h36_action_wise_eval(interp, gt.astype(np.float64), actions, root), f"stride {stride} ALL FRAMES")
    # KEYFRAMES: the raw predictions of the selected rows
    errk, sumsk = _dev_errors(pred, gt, root, select=key.astype(np.uint8), actions=actions, num_actions=15, want_sums=True)
    assert np.all(errk[~key] == -1.0)
    _check_errors(errk[key], _host_errors(pred[key], gt[key], root), f"stride {stride}, keyframes")
    _check_reports(E.report_from_sums(sumsk), E.h36_action_wise_eval(pred[key].astype(np.float64), gt[key].astype(np.float64), actions[key], root),
                   f"stride {stride} KEYFRAMES")
    # the Python layer: the dict of evaluate_predictions, from the forwarded rows only
    cfg = util.load_config("h36m_351")
    cfg.SEQUENCE_STRIDE, cfg.MASK_STRIDE, cfg.TEST_STRIDED_EVAL = stride, stride, True
    fwd = key.copy()
    fwd[np.flatnonzero(~key & (E.keyframe_plan(idx, stride)[0] == np.arange(len(idx))))] = True     # frames in front of a first keyframe
    rows = np.full(len(idx), -1)
    rows[fwd] = np.arange(fwd.sum())
    full = np.where(fwd[:, None, None], pred, 0).astype(np.float32)
    for aw in (True, False):
        want_rep = E.evaluate_predictions(full, gt[..., :3], actions, idx, cfg, action_wise=aw)
        got_rep = ED.evaluate_predictions_device(_cuda(pred[fwd]), _cuda(gt[..., :3]), actions, idx, cfg, action_wise=aw, rows=rows)
        assert got_rep["keyframes"] is not None
        _check_reports(got_rep, want_rep, f"stride {stride} evaluate_predictions action_wise={aw}")
    rows[np.flatnonzero(key)[3]] = -1
    with pytest.raises(ValueError):
        ED.evaluate_predictions_device(_cuda(pred[fwd]), _cuda(gt[..., :3]), actions, idx, cfg, rows=rows)
    cfg.TEST_STRIDED_EVAL = False
    plain = ED.evaluate_predictions_device(_cuda(pred), _cuda(gt[..., :3]), actions, idx, cfg)
    assert plain["keyframes"] is None
    _check_reports(plain, E.evaluate_predictions(pred, gt[..., :3], actions, idx, cfg), "unstrided")
    cfg.TEST_STRIDED_EVAL, cfg.EVAL_DISABLE_LEARNED_UPSAMPLING, cfg.SEQUENCE_STRIDE, cfg.MASK_STRIDE = True, True, 1, stride
    _check_reports(ED.evaluate_predictions_device(_cuda(pred), _cuda(gt[..., :3]), actions, idx, cfg),
                   E.evaluate_predictions(pred, gt[..., :3], actions, idx, cfg), "mask stride only")


def test_degenerate_poses():
    """Conditions only: collinear or all-zero poses give finite values or the raw-prediction fallback of evaluation.pmpjpe; a pose whose
    optimal scale is 0 / 0 has NaN N-MPJPE and is left out of the sums, as on the host."""
    from uplift_upsample_3dhpe_amd import evaluation as E
    rng = np.random.default_rng(3)
    B, J, root = 70, 17, 6
    gt3 = rng.normal(0, 0.35, size=(B, J, 3))
    pred, gt = _fixture_like(rng, gt3, invalid=0.0)
    line = rng.normal(size=(J, 1)) * np.array([[0.3, -0.2, 0.5]])
    pred[0] = line                                   # collinear prediction
    pred[1] = 0.0                                    # all-zero prediction: zero extent, and p - p[root] = 0 (N-MPJPE scale 0 / 0)
    gt[2, :, :3] = 0.0                               # all-zero ground truth
    gt[3, :, :3] = line + 0.1                        # collinear ground truth
    pred[4] = pred[4, root]                          # every joint at the root
    gt[5, :, 3] = 0.0; gt[5, root, 3] = 1.0          # only the root is valid: masked sums 0 / 0
    pred, gt = pred.astype(np.float32), gt.astype(np.float32)
    err, sums = _dev_errors(pred, gt, root, want_sums=True)
    want = np.full(err.shape, np.nan)                # (the host's batched SVD raises on a NaN matrix: its P-MPJPE for the regular poses only)
    want[6:] = _host_errors(pred[6:], gt[6:], root)
    with np.errstate(invalid="ignore", divide="ignore"):
        want[:6, :, 0] = E.mpjpe(pred[:6].astype(np.float64), gt[:6].astype(np.float64), root, normalize=False)
        want[:6, :, 1] = E.nmpjpe(pred[:6].astype(np.float64), gt[:6].astype(np.float64), root, normalize=False)
    raw = np.linalg.norm(pred.astype(np.float64) - gt[..., :3], axis=-1)
    for b in range(6):
        p = err[b, :, 2][gt[b, :, 3] > 0]
        r = raw[b][gt[b, :, 3] > 0]
        assert np.all(np.isfinite(p)) or np.allclose(p, r, atol=1e-12), (b, p)
    for b in (1, 4, 5):
        assert np.all(np.isnan(err[b, :, 1][gt[b, :, 3] > 0])) and np.all(np.isnan(want[b, :, 1][gt[b, :, 3] > 0]))
    assert np.array_equal(err[..., :2] == -1.0, want[..., :2] == -1.0) and np.array_equal(err[..., 2] == -1.0, err[..., 0] == -1.0)
    _check_errors(err[6:], want[6:], "regular poses next to degenerate ones")
    assert np.array_equal(np.isnan(err[..., :2]), np.isnan(want[..., :2]))
    fin = np.isfinite(want[..., :2])
    assert np.abs(err[..., :2][fin] - want[..., :2][fin]).max() < 1e-9
    host = _sums_table(want, np.zeros(B, int), 0)
    assert np.array_equal(sums[0, :2, 1], host[0, :2, 1]) and sums[0, 1, 1] < sums[0, 0, 1]      # NaN is not >= 0: not counted
    assert np.abs(sums[0, :2, 0] - host[0, :2, 0]).max() < 1e-9 * B * J


def test_reflected_predictions():
    rng = np.random.default_rng(4)
    gt3 = rng.normal(0, 0.3, size=(300, 17, 3))
    pred = (gt3 + rng.normal(0, 0.05, size=gt3.shape)).astype(np.float32)
    gt = np.concatenate([gt3, np.ones((300, 17, 1))], -1).astype(np.float32)
    refl = pred * np.array([-1.0, 1.0, 1.0], np.float32)
    base, _ = _dev_errors(pred, gt, 6)
    err, _ = _dev_errors(refl, gt, 6)
    _check_errors(err, _host_errors(refl, gt, 6), "reflected")
    _check_errors(base, _host_errors(pred, gt, 6), "unreflected")
    assert err[..., 2].mean() > 2 * base[..., 2].mean()                   # a rotation cannot undo a reflection


def test_invariances():
    """Float64 inputs: the transformed poses are not representable in float32."""
    rng = np.random.default_rng(5)
    gt3 = rng.normal(0, 0.3, size=(400, 17, 3))
    pred = gt3 + rng.normal(0, 0.05, size=gt3.shape)
    base, _ = _dev_errors(pred, gt3, 6)

    def rot():
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        return q * np.sign(np.linalg.det(q))
    moved = np.stack([2.5 * p @ rot() + rng.normal(size=3) for p in pred])
    assert np.abs(_dev_errors(moved, gt3, 6)[0][..., 2] - base[..., 2]).max() < 1e-10
    assert np.abs(_dev_errors(pred * 3.0, gt3, 6)[0][..., 1] - base[..., 1]).max() < 1e-10
    assert np.abs(_dev_errors(pred + 0.7, gt3, 6)[0][..., 1] - base[..., 1]).max() < 1e-10
    assert np.abs(_dev_errors(pred + 0.7, gt3, 6)[0][..., 0] - base[..., 0]).max() < 1e-10
    copy = np.stack([(g @ rot()) * 1.7 + rng.normal(size=3) for g in gt3])
    exact = _dev_errors(copy, gt3, 6)[0]
    assert exact[..., 2].max() < 1e-12
    same = _dev_errors(gt3 * 1.7, gt3, 6)[0]
    assert same[..., 1].max() < 1e-12 and _dev_errors(gt3 + 0.3, gt3, 6)[0][..., 0].max() < 1e-12


def test_two_launches_give_the_same_bits():
    from uplift_upsample_3dhpe_amd import evaluation as E, evaluation_device as ED
    rng = np.random.default_rng(6)
    gt3, idx = _smooth_videos(rng, [9000, 8000, 8037], 17)
    pred, gt = _fixture_like(rng, gt3)
    pred, gt = _cuda(pred.astype(np.float32)), _cuda(gt.astype(np.float32))
    left, right, weight, _ = E.keyframe_plan(idx, 5)
    actions = (np.arange(len(idx)) % 15).astype(np.int32)
    runs = [ED.pose_errors(pred, gt, 6, left=left, right=right, weight=weight, actions=actions, num_actions=15, want_sums=True) for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    only = ED.pose_errors(pred, gt, 6, left=left, right=right, weight=weight, actions=actions, num_actions=15, want_errors=False, want_sums=True)[1]
    assert torch.equal(only, runs[0][1])                                  # with or without the error array
    assert torch.equal(ED.error_sums(runs[0][0], actions=actions, num_actions=15), runs[0][1])


@pytest.mark.parametrize("J", [24, 32, 1])
def test_other_joint_counts_without_valid_flags(J):
    rng = np.random.default_rng(J)
    gt3 = rng.normal(0, 0.35, size=(3000, J, 3))
    pred, _ = _fixture_like(rng, gt3, root=0)
    pred, gt3 = pred.astype(np.float32), gt3.astype(np.float32)
    err, _ = _dev_errors(pred, gt3, 0)
    if J == 1:                                                            # one joint: zero extent, every metric of the root
        assert np.all(err[..., 0] == 0) and np.all(np.isnan(err[..., 1]))
        return
    _check_errors(err, _host_errors(pred, gt3, 0), f"J = {J}, C = 3")


def test_argument_checks_do_not_launch():
    from uplift_upsample_3dhpe_amd import _capi
    lib = _capi.load_library()
    bad = _capi.UU3D_ERR_INVALID_ARGUMENT
    x = torch.zeros((4, 17, 3), device="cuda")
    out = torch.zeros((4, 17, 3), dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda **k: lib.uu3d_pose_errors(*[k.get(n, d) for n, d in (
        ("pred", p(x)), ("R", 4), ("left", None), ("right", None), ("weight", None), ("gt", p(x)), ("P", 4), ("J", 17), ("C", 3), ("root", 6),
        ("f64", 0), ("errors", p(out)), ("actions", None), ("A", 0), ("select", None), ("sums", None), ("scratch", None), ("nbytes", 0), ("stream", None))])
    assert call() == _capi.UU3D_OK
    for k in (dict(pred=None), dict(gt=None), dict(J=33), dict(J=0), dict(C=2), dict(root=17), dict(root=-1), dict(errors=None), dict(P=0),
              dict(P=5), dict(weight=p(out)), dict(f64=2), dict(sums=p(out)), dict(sums=p(out), scratch=p(out), nbytes=8),
              dict(sums=p(out), scratch=p(out), nbytes=1 << 20, A=64), dict(sums=p(out), scratch=p(out), nbytes=1 << 20, A=2)):
        assert call(**k) == bad, k
    assert lib.uu3d_error_sums(None, 4, 17, None, 0, None, p(out), p(out), 1 << 20, None) == bad
    assert lib.uu3d_error_sums(p(out), 4, 17, None, 0, None, p(out), p(out), 8, None) == bad
    assert lib.uu3d_error_sums_scratch_bytes(4, 64) == 0 and lib.uu3d_error_sums_scratch_bytes(0, 1) == 0
    assert lib.uu3d_error_sums_scratch_bytes(4, 15) > 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("reuse", [False, True])
def test_run_eval_with_device_metrics(reuse):
    from uplift_upsample_3dhpe_amd import eval as ev
    cfg = util.load_config("h36m_351")
    cfg.BATCH_SIZE = 16
    arch = pkg.arch_from_config(cfg)
    model = pkg.build_uplift_upsample_transformer(cfg, weights=pkg.init_weights(arch, seed=2, perturb=0.1))
    args = (cfg, "h36m", os.path.join(G, "h36m_tiny_3d.npz"), os.path.join(G, "h36m_tiny_2d.npz"), "S9")
    for aw in (True, False):
        lines = [[], []]
        host = ev.run_eval_multi_mask_stride(*args, model=model, action_wise=aw, reuse_frames=reuse, log=lambda *a: lines[0].append(" ".join(map(str, a))))
        dev = ev.run_eval_multi_mask_stride(*args, model=model, action_wise=aw, reuse_frames=reuse, device_metrics=True,
                                            log=lambda *a: lines[1].append(" ".join(map(str, a))))
        assert sorted(dev) == sorted(host)
        for msv in host:
            assert dev[msv]["keyframes"] is not None and set(dev[msv]) == set(host[msv])
            _check_reports(dev[msv], host[msv], f"run_eval reuse_frames={reuse} action_wise={aw} mask stride {msv}")
        strip = lambda ls: [l for l in ls if not l.startswith("Finished evaluation")]
        assert len(lines[0]) == len(lines[1]) and any("KEYFRAMES" in l for l in lines[1])
        assert [l.split(":")[0] for l in strip(lines[0])] == [l.split(":")[0] for l in strip(lines[1])]


def test_run_train_with_device_metrics(tmp_path):
    """Two epochs with and without the flag: the same metric history within 1e-5 mm, the same weights bit for bit."""
    from tests.test_train_loop_gpu import _config, _h36m_copy, _quiet
    from uplift_upsample_3dhpe_amd.train import run_train
    p3, p2 = _h36m_copy(tmp_path)
    cfg = _config(tmp_path)
    kw = dict(h36m_path=p3, dataset_2d_path=p2, train_subset="S8", val_subset="S9", test_subset="S9", log=_quiet)
    a = run_train(cfg, out_dir=str(tmp_path / "host"), **kw)
    b = run_train(cfg, out_dir=str(tmp_path / "dev"), device_metrics=True, **kw)
    assert list(a["history"]) == list(b["history"])
    worst = 0.0
    for m in a["history"]:
        assert len(a["history"][m]) == len(b["history"][m]) == 2
        for (ea, va), (eb, vb) in zip(a["history"][m], b["history"][m]):
            assert ea == eb
            if m == "loss":
                assert va == vb
            elif np.isnan(va):
                assert np.isnan(vb)
            else:
                worst = max(worst, abs(va - vb))
                assert abs(va - vb) <= TOL_MM, (m, ea, va, vb)
    print(f"run_train metric history max |device - host| (mm): {worst:.3e}")
    za, zb = np.load(str(tmp_path / "host/checkpoints/cp_0002.npz")), np.load(str(tmp_path / "dev/checkpoints/cp_0002.npz"))
    for k in ("params", "ema", "adam_m", "adam_v", "rng_state", "global_step"):
        assert np.array_equal(za[k], zb[k]), k
    assert os.path.basename(a["best_weights"]) == os.path.basename(b["best_weights"])
    _check_reports(b["test_report"], a["test_report"], "run_train test report")


def test_two_ranks_on_one_gpu(tmp_path):
    """Each rank evaluates a shard of the poses, the sums tables are added in rank order: both ranks return the one-rank report -- from
    run_eval, from a pass of report_sums without a plan (rank 1's shard starts at its own rows), and in run_train's validation."""
    from tests.test_train_loop_gpu import _config, _h36m_copy
    from uplift_upsample_3dhpe_amd import evaluation as E, evaluation_device as ED
    p3, p2 = _h36m_copy(tmp_path)
    cfg = _config(tmp_path, DROP_PATH_RATE=0.0, DROP_RATE=0.0, ATTENTION_DROP_RATE=0.0, BATCH_SIZE=12)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, PYTHONPATH=util.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(util.ROOT, "tests", "device_metrics_dist2_worker.py"), str(r), "2", str(port), str(tmp_path),
                               cfg, p3, p2], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o)
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-3000:] for l in logs)
    res = [json.load(open(os.path.join(tmp_path, f"rank{r}.json"))) for r in range(2)]
    from tests.device_metrics_dist2_worker import plain_pass_inputs, reports
    one = reports()
    assert res[0]["shards"] != res[1]["shards"] and min(res[0]["shards"] + res[1]["shards"]) > 0
    for r in res:
        assert r["num_forwarded"] == one["num_forwarded"]
        for mode in ("host", "device"):
            _check_reports(r["device"], one[mode], f"rank {r['rank']} against one rank ({mode})")
    assert json.dumps(res[0]["device"]) == json.dumps(res[1]["device"])
    # the plan-less pass: against one rank on the device and against the host
    pred, gt, actions = plain_pass_inputs()
    one_sums = ED.report_sums(_cuda(pred), _cuda(gt), 6, [{}], num_actions=15, actions=actions)
    host_rep = E.h36_action_wise_eval(pred.astype(np.float64), np.concatenate([gt, np.ones(gt.shape[:2] + (1,), np.float32)], -1).astype(np.float64),
                                      actions, 6)
    for r in res:
        two = np.asarray(r["plain_sums"])
        assert np.array_equal(two[..., 1], one_sums[..., 1])
        _check_reports(E.report_from_sums(two[0]), E.report_from_sums(one_sums[0]), f"rank {r['rank']} plan-less pass against one rank")
        _check_reports(E.report_from_sums(two[0]), host_rep, f"rank {r['rank']} plan-less pass against the host")
    # run_train over the two ranks: the metric history with the flag equals the history without (the same training, the same predictions)
    for r in res:
        a, b = r["history_host"], r["history_device"]
        assert list(a) == list(b) and json.dumps(b) == json.dumps(res[0]["history_device"])
        worst = 0.0
        for m in a:
            assert len(a[m]) == len(b[m]) == 2
            for (ea, va), (eb, vb) in zip(a[m], b[m]):
                assert ea == eb
                if m == "loss":
                    assert va == vb
                elif np.isnan(va):
                    assert np.isnan(vb)
                else:
                    worst = max(worst, abs(va - vb))
                    assert abs(va - vb) <= TOL_MM, (m, ea, va, vb)
        print(f"rank {r['rank']} two-rank run_train metric history max |device - host| (mm): {worst:.3e}")
    za, zb = (np.load(str(tmp_path / f"{mode}_rank0" / "checkpoints" / "cp_0002.npz")) for mode in ("host", "device"))
    for k in ("params", "ema"):
        assert np.array_equal(za[k], zb[k]), k
