"""The evaluation report computed on the device: ``evaluation.evaluate_predictions`` with the predictions and the
ground truth left in HBM.  csrc/uu3d_metrics.h computes MPJPE / N-MPJPE / P-MPJPE per joint in float64 with the keyframe interpolation fused
into its load (``evaluation.keyframe_plan``) and the per-action sums of the report; the host only divides the
``(actions + 1, 3, 2)`` table (``evaluation.report_from_sums``).  ``evaluation.py`` stays the yardstick (tests/test_device_metrics_gpu.py).

With torch.distributed initialised every rank evaluates a contiguous shard of the poses; the tables are gathered and added in rank order,
so every rank returns the same report."""
import ctypes as C

import numpy as np

from . import _capi
from . import dist as udist
from . import evaluation
from ._capi import ptr as _ptr


def _dev(a, dtype, device):
    import torch
    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)


def pose_errors(pred, gt, root, left=None, right=None, weight=None, actions=None, num_actions=0, select=None, want_errors=True,
                want_sums=False):
    """uu3d_pose_errors on the current stream.  pred (R, J, 3), gt (P, J, 3 | 4): device tensors, both float32 or both float64; left / right
    (int32), weight (float64), actions (int32), select (uint8): host arrays or device tensors of P entries, or None.
    -> (errors (P, J, 3) float64 or None, sums (num_actions + 1, 3, 2) float64 or None), device tensors."""
    import torch
    lib = _capi.load_library()
    if not (pred.is_cuda and gt.is_cuda and pred.dtype == gt.dtype and pred.dtype in (torch.float32, torch.float64)):
        raise ValueError("pred and gt must be device tensors of one dtype, float32 or float64")
    if pred.dim() != 3 or gt.dim() != 3 or pred.shape[2] != 3 or gt.shape[1] != pred.shape[1] or gt.shape[2] not in (3, 4):
        raise ValueError(f"pred {tuple(pred.shape)} / gt {tuple(gt.shape)}: expected (R, J, 3) and (P, J, 3 | 4)")
    dev = pred.device
    pred, gt = pred.contiguous(), gt.contiguous()
    P, J = int(gt.shape[0]), int(gt.shape[1])
    left, right = _dev(left, torch.int32, dev), _dev(right, torch.int32, dev)
    weight, actions, select = _dev(weight, torch.float64, dev), _dev(actions, torch.int32, dev), _dev(select, torch.uint8, dev)
    for name, a in (("left", left), ("right", right), ("weight", weight), ("actions", actions), ("select", select)):
        if a is not None and tuple(a.shape) != (P,):
            raise ValueError(f"{name} has shape {tuple(a.shape)}, expected ({P},)")
    errors = torch.empty((P, J, 3), dtype=torch.float64, device=dev) if want_errors else None
    sums = scratch = None
    nbytes = 0
    if want_sums:
        sums = torch.empty((num_actions + 1, 3, 2), dtype=torch.float64, device=dev)
        nbytes = int(lib.uu3d_error_sums_scratch_bytes(P, num_actions))
        scratch = torch.empty((max(nbytes, 8) // 8,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(lib, lib.uu3d_pose_errors(_ptr(pred), int(pred.shape[0]), _ptr(left), _ptr(right), _ptr(weight), _ptr(gt), P, J,
                                              int(gt.shape[2]), int(root), int(pred.dtype == torch.float64), _ptr(errors), _ptr(actions),
                                              int(num_actions), _ptr(select), _ptr(sums), _ptr(scratch), C.c_size_t(nbytes),
                                              C.c_void_p(stream)), None)
    return errors, sums


def error_sums(errors, actions=None, num_actions=0, select=None):
    """uu3d_error_sums on the current stream: errors (P, J, 3) float64 on the device -> sums (num_actions + 1, 3, 2) on the device."""
    import torch
    lib = _capi.load_library()
    if not (errors.is_cuda and errors.dtype == torch.float64 and errors.dim() == 3 and errors.shape[2] == 3):
        raise ValueError("errors must be a (P, J, 3) float64 device tensor")
    dev = errors.device
    errors = errors.contiguous()
    P, J = int(errors.shape[0]), int(errors.shape[1])
    actions, select = _dev(actions, torch.int32, dev), _dev(select, torch.uint8, dev)
    sums = torch.empty((num_actions + 1, 3, 2), dtype=torch.float64, device=dev)
    nbytes = int(lib.uu3d_error_sums_scratch_bytes(P, num_actions))
    scratch = torch.empty((max(nbytes, 8) // 8,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _capi.check(lib, lib.uu3d_error_sums(_ptr(errors), P, J, _ptr(actions), int(num_actions), _ptr(select), _ptr(sums), _ptr(scratch),
                                             C.c_size_t(nbytes), C.c_void_p(stream)), None)
    return sums


def _rank_world():
    import torch.distributed as tdist
    if tdist.is_available() and tdist.is_initialized():
        return tdist.get_rank(), tdist.get_world_size()
    return 0, 1


def report_sums(pred_dev, gt_dev, root, passes, num_actions=0, actions=None):
    """One sums table per entry of ``passes`` (dicts of the optional host arrays left / right / weight / select of P entries; without
    ``left`` pose i is row i of ``pred_dev``), as numpy
    (len(passes), num_actions + 1, 3, 2): this rank's contiguous shard of the poses through uu3d_pose_errors (no error array is
    written), ONE copy to the host, and with several ranks one gather of the tables, added in rank order."""
    import torch
    rank, world = _rank_world()
    P = int(gt_dev.shape[0])
    lo, hi = udist.shard_bounds(P, rank, world)
    cut = lambda a: None if a is None else a[lo:hi]
    tables = []
    for ps in passes:
        if hi == lo:
            tables.append(torch.zeros((num_actions + 1, 3, 2), dtype=torch.float64, device=gt_dev.device))
            continue
        left = ps.get("left")
        if left is None:                                             # "pose i is row i" counts from the shard's first pose, not from row 0
            left = np.arange(P, dtype=np.int32)
        _, sums = pose_errors(pred_dev, gt_dev[lo:hi], root, left=cut(left), right=cut(ps.get("right")),
                              weight=cut(ps.get("weight")), actions=cut(actions), num_actions=num_actions, select=cut(ps.get("select")),
                              want_errors=False, want_sums=True)
        tables.append(sums)
    local = torch.stack(tables, 0)[None]                             # (1, passes, A + 1, 3, 2)
    every = udist.allgather_errors(local) if world > 1 else local    # (world, ...) in rank order
    every = every.cpu().numpy()
    total = np.zeros(every.shape[1:], np.float64)
    for r in range(every.shape[0]):
        total += every[r]
    return total


def evaluate_predictions_device(pred_dev, gt_dev, actions, frame_indices, config, action_wise=True, rows=None):
    """``evaluation.evaluate_predictions`` on the device: the same dict (same keys, same order of actions, "keyframes" None under the same
    conditions).  pred_dev (R, J, 3) float32: the forwarded predictions; ``rows`` (P,): the row of ``pred_dev`` that holds each position's
    prediction, -1 where it was not forwarded (None: row i is position i); gt_dev (P, J, 3 | 4) float32 on the device (root-shifted or
    not: every metric aligns it itself); actions, frame_indices: host arrays of P entries."""
    frame_indices = np.asarray(frame_indices)
    P = len(frame_indices)
    if int(gt_dev.shape[0]) != P:
        raise ValueError(f"gt_dev has {int(gt_dev.shape[0])} poses, frame_indices {P}")
    if rows is None:
        if int(pred_dev.shape[0]) != P:
            raise ValueError(f"pred_dev has {int(pred_dev.shape[0])} rows for {P} positions and no `rows`")
        rows = np.arange(P, dtype=np.int64)
    rows = np.asarray(rows).astype(np.int64)
    mask_stride = config.MASK_STRIDE[0] if isinstance(config.MASK_STRIDE, (list, tuple)) else config.MASK_STRIDE
    strided = config.TEST_STRIDED_EVAL is True
    if config.SEQUENCE_STRIDE > 1 and strided:
        strides = np.tile([config.SEQUENCE_STRIDE], reps=(P))
        if getattr(config, "EVAL_DISABLE_LEARNED_UPSAMPLING", False) and mask_stride is not None:
            strides[:] = mask_stride
        left, right, weight, _ = evaluation.keyframe_plan(frame_indices, strides, rows=rows)
        passes = [{"left": left, "right": right, "weight": weight}]
    else:
        if (rows < 0).any():
            raise ValueError("every position is evaluated, but some were not forwarded")
        passes = [{"left": rows}]
    if (config.SEQUENCE_STRIDE > 1 or (mask_stride is not None and mask_stride > 1)) and strided:
        input_stride = config.SEQUENCE_STRIDE if mask_stride is None else mask_stride
        key = np.equal(np.mod(frame_indices, input_stride), 0)
        if (rows[key] < 0).any():
            raise ValueError("a keyframe of the KEYFRAMES report was not forwarded")
        passes.append({"left": rows, "select": key.astype(np.uint8)})
    A = len(evaluation.H36M_ACTIONS) if action_wise else 0
    tables = report_sums(pred_dev, gt_dev, config.ROOT_KEYTPOINT, passes, num_actions=A,
                         actions=np.asarray(actions).astype(np.int32) if action_wise else None)
    out = {"all_frames": evaluation.report_from_sums(tables[0], action_wise), "keyframes": None}
    if len(passes) > 1:
        out["keyframes"] = evaluation.report_from_sums(tables[1], action_wise)
    return out
