"""Training driver -- the reference's ``train.py`` (dataset set-up :44-191, epoch loop :386-749) over this package's pieces:

    .npz / AMASS ingestion (h36m.py, amass.py)  ->  videos resident in HBM (data.PoseTable)  ->  the training stream as host
    descriptors (data.DescriptorStream = ``repeat().batch(B)``: batches may straddle generator epochs)  ->  uu3d_gather_windows
    (+ uu3d_world_to_cam_2d for AMASS) builds each batch on the device  ->  Trainer.train_step (forward, loss, backward, bucketed
    all-reduce, guarded AdamW, EMA)  ->  per epoch: validation (flip, batch wrap), metric history, best / last ``.h5``, checkpoint.

    from uplift_upsample_3dhpe_amd.train import run_train
    result = run_train("config/h36m_81.json", h36m_path=..., dataset_2d_path=..., out_dir="out")
    python -m uplift_upsample_3dhpe_amd.train --config config/h36m_81.json --out_dir out      # the reference's flags

The step loop never waits for the device: descriptors are sliced on the host and uploaded from pinned memory, the epoch loss and
the count of skipped steps accumulate on the device, the 10-step log line reads a copy started at an earlier log line.  The host
synchronises once per epoch (validation, checkpoint, weight files).

Deliberate differences from the reference ("run_train"): the checkpoint ``cp_XXXX.npz`` also holds the stream
position and the metric history, so a resumed run is bit-identical to an uninterrupted one; it is written at the END of the epoch
(after validation and the weight files); scalars go to ``history.jsonl`` instead of TensorBoard.
"""
import argparse
import datetime
import glob
import json
import os
import re
import sys
import time

import numpy as np

from . import amass as uamass
from . import dist as udist
from . import evaluation, h36m
from .data import AmassSequenceGenerator, DescriptorStream, PoseTable, SequenceGenerator, validation_descriptors, world_to_cam_and_2d
from .net.uplift_upsample_transformer_config import UpliftUpsampleConfig
from .utils.metric_history import MetricHistory
from .utils.weight_io import resolve_weight_selector

LOG_EVERY = 10                    # train.py:567
TIMING_KEYS = ("train/step_duration", "epoch_seconds", "val_seconds")


def _log(*args):
    print(*args, flush=True)


def _format_time(seconds):
    return str(datetime.timedelta(seconds=int(round(max(0.0, seconds)))))


def _rank_world():
    import torch.distributed as tdist
    if tdist.is_available() and tdist.is_initialized():
        return tdist.get_rank(), tdist.get_world_size()
    return 0, 1


# ---------------------------------------------------------------------------------------------------------------------------------
# data sets (train.py:44-191)
# ---------------------------------------------------------------------------------------------------------------------------------
def _split_options(config, split):
    train = split == "train"
    return dict(subsample=config.DATASET_TRAIN_3D_SUBSAMPLE_STEP if train else config.DATASET_VAL_3D_SUBSAMPLE_STEP,
                stride=config.SEQUENCE_STRIDE, padding_type=config.PADDING_TYPE,
                flip_augment=train and config.AUGM_FLIP_PROB > 0, in_batch_augment=config.IN_BATCH_AUGMENT,
                mask_stride=config.MASK_STRIDE, stride_mask_align_global=False,
                rand_shift_stride_mask=bool(config.STRIDE_MASK_RAND_SHIFT) and train, shuffle=train, seed=config.SHUFFLE_SEED)


def h36m_generator(config, h36m_data, subset, split, device=None, log=_log):
    """create_h36m_datasets (train.py:44-91) for one split: ``h36m_data`` = load_dataset_and_2d_poses(...)."""
    dataset_3d, poses_2d = h36m_data
    _, poses_3d, p2d, _, subjects, actions, rates = h36m.filter_and_subsample_dataset(
        dataset_3d, poses_2d, h36m.subjects_of_split(subset), "*", downsample=1, image_base_path=None, verbose=False)
    table = h36m.pose_table(p2d, poses_3d, subjects, actions, rates, device=device)
    gen = SequenceGenerator(table, seq_len=config.SEQUENCE_LENGTH, target_frame_rate=50,
                            flip_lr_indices=config.AUGM_FLIP_KEYPOINT_ORDER, **_split_options(config, split))
    log(f"Sequences: {len(gen)}")
    return gen


def amass_generator(config, amass_path, h36m_path, subset, split, target_frame_rate, cameras=None, device=None, log=_log):
    """create_amass_datasets (train.py:125-160) for one split -> (generator, the Human3.6M cameras for the next split)."""
    log(f"Loading AMASS dataset for split {subset}")
    ds = uamass.AMASSDataset(amass_path, h36m_path, subset, h36m_cameras=cameras)
    seqs, rates = uamass.sequences(ds)
    table = PoseTable(None, seqs, frame_rates=rates, device=device)
    gen = AmassSequenceGenerator(table, uamass.camera_table(ds), seq_len=config.SEQUENCE_LENGTH, target_frame_rate=int(target_frame_rate),
                                 flip_lr_indices=h36m.FLIP_LR_INDICES, **_split_options(config, split))
    log(f"Sequences: {len(gen)}")
    return gen, ds.cameras()


def gather_batch(generator, desc, cams=None):
    """One batch on the device -> (2D windows (B, N, J, 2), 3D targets (B, N, J, 3), stride masks (B, N) uint8).  H36M: the generator's
    gather (2D already multiplied by the stride mask); AMASS: world-frame windows + camera draws through world_to_cam_and_2d."""
    if isinstance(generator, AmassSequenceGenerator):
        b = generator.gather(desc, cams)
        cam3d, kp2d = world_to_cam_and_2d(b["kp3d"], b["cams"])
        return kp2d, cam3d, b["stride_mask"]
    b = generator.gather(desc, zero_masked=True, with_3d=True)
    return b["kp2d"], b["kp3d"], b["stride_mask"]


def _flip(x, order):
    """train.py:609-618: negate x, swap left / right joints (axis 2 of (B, N, J, C), axis 1 of (B, J, 3))."""
    import torch
    axis = 2 if x.dim() == 4 else 1
    return torch.cat([x[..., :1] * -1.0, x[..., 1:]], dim=-1).index_select(axis, order)


# ---------------------------------------------------------------------------------------------------------------------------------
# validation (train.py:592-700)
# ---------------------------------------------------------------------------------------------------------------------------------
class Validation(object):
    """The validation set of a run: descriptors of ``ceil(VE / B)`` full batches (the last one wraps), each rank's contiguous shard of
    every batch, and the eval-mode forwards of val_step (train.py:509-538) with EVAL_FLIP."""

    def __init__(self, config, generator, is_h36m, device_metrics=False):
        import torch
        self.config, self.gen, self.is_h36m = config, generator, is_h36m
        self.device_metrics = bool(device_metrics)
        self.B = int(config.BATCH_SIZE)
        self.desc, self.cams, self.n_batches, self.examples = validation_descriptors(generator, self.B, config.VALIDATION_EXAMPLES)
        self.order = torch.as_tensor(np.asarray(config.AUGM_FLIP_KEYPOINT_ORDER), dtype=torch.long, device=generator.table.device)
        self.loss_config = config.copy()                   # val_step's loss: central + sequence, unweighted, over BATCH_SIZE (:522-535)
        self.loss_config.LOSS_WEIGHT_CENTER, self.loss_config.LOSS_WEIGHT_SEQUENCE = 1.0, 1.0

    def _loss(self, full, central, kp3d):
        from .optim import train_loss
        loss, _, _ = train_loss(full, central, kp3d, self.loss_config, want_grads=False)
        return loss[0] if full is not None else loss[1]

    def _forward(self, model, kp2d, smask):
        if model.has_strided_input:
            return model([kp2d, smask], training=False)
        return model(kp2d, training=False)

    def run(self, model):
        """-> (val loss, metrics dict of the reference's names, per-window predictions (examples, J, 3) float64).  ``model`` holds the
        weights to validate (val_model: the EMA weights when EMA_ENABLED).  With ``device_metrics`` the metrics come from
        csrc/uu3d_metrics.h; the returned predictions are the same host array either way."""
        import torch
        rank, world = _rank_world()
        cfg = self.config
        dev = self.gen.table.device
        flip = cfg.EVAL_FLIP is True
        loss_sum = torch.zeros((), dtype=torch.float64, device=dev)
        local = []                                           # per batch: (rows, J, 6) = prediction | root-shifted centre ground truth
        mid = cfg.SEQUENCE_LENGTH // 2
        root = cfg.ROOT_KEYTPOINT
        for b in range(self.n_batches):
            r0 = b * self.B
            n = min(self.B, len(self.desc) - r0)
            lo, hi = udist.shard_bounds(n, rank, world)
            if hi == lo:
                continue
            d = self.desc[r0 + lo:r0 + hi]
            c = None if self.cams is None else self.cams[r0 + lo:r0 + hi]
            kp2d, kp3d, smask = gather_batch(self.gen, d, c)
            full, pred = self._forward(model, kp2d, smask)
            loss_sum += self._loss(full, pred, kp3d)
            if flip:
                if self.is_h36m:                             # the generator's flip bit = negate x + swap joints of the 2D and 3D windows
                    df = d.copy()
                    df[:, 5] = 1 - df[:, 5]
                    fk2d, fk3d, _ = gather_batch(self.gen, df, c)
                else:                                        # AMASS: the projected windows are mirrored, as train.py:609-618 does
                    fk2d, fk3d = _flip(kp2d, self.order), _flip(kp3d, self.order)
                ffull, fpred = self._forward(model, fk2d, smask)
                loss_sum += self._loss(ffull, fpred, fk3d)
                pred = (pred + _flip(fpred, self.order)) / 2.0
            gt = kp3d[:, mid] - kp3d[:, mid, root:root + 1]
            local.append(torch.cat([pred, gt], dim=-1))
        J = self.gen.table.J
        local = torch.cat(local, 0) if local else torch.zeros((0, J, 6), dtype=torch.float32, device=dev)
        if world > 1:
            import torch.distributed as tdist
            tdist.all_reduce(loss_sum)
            allp = udist.allgather_errors(local)             # rank order: rank 0's rows of every batch, then rank 1's, ...
            sizes = [min(self.B, len(self.desc) - b * self.B) for b in range(self.n_batches)]
            bounds = [[udist.shard_bounds(n, r, world) for n in sizes] for r in range(world)]
            at = np.cumsum([0] + [sum(hi - lo for lo, hi in bounds[r]) for r in range(world)])[:-1]
            parts = []
            for b in range(self.n_batches):                  # back to batch order
                for r in range(world):
                    lo, hi = bounds[r][b]
                    parts.append(allp[at[r]:at[r] + hi - lo])
                    at[r] += hi - lo
            local = torch.cat(parts, 0)
        n_calls = self.n_batches * (2 if flip else 1)
        loss = float(loss_sum.item()) / n_calls
        metrics = {"loss": loss}
        if self.device_metrics:
            # the metrics where the predictions lie (csrc/uu3d_metrics.h); with several ranks each evaluates a shard of the examples
            from . import evaluation_device
            dpred, dgt = local[:self.examples, :, :3].contiguous(), local[:self.examples, :, 3:].contiguous()
            A = len(evaluation.H36M_ACTIONS) if self.is_h36m else 0
            actions = self.gen.table.actions[self.desc[:self.examples, 0]].astype(np.int32) if self.is_h36m else None
            sums = evaluation_device.report_sums(dpred, dgt, root, [{}], num_actions=A, actions=actions)[0]
            rep = evaluation.report_from_sums(sums, action_wise=self.is_h36m)
            frame, aw = rep[:2] if self.is_h36m else (rep, None)
            metrics.update({"MPJPE": float(frame["mpjpe"]), "NMPJPE": float(frame["nmpjpe"]), "PAMPJPE": float(frame["pampjpe"])})
            if aw is not None:
                metrics.update({"AW-MPJPE": float(aw["mpjpe"]), "AW-NMPJPE": float(aw["nmpjpe"]), "AW-PAMPJPE": float(aw["pampjpe"])})
            return loss, metrics, dpred.cpu().numpy().astype(np.float64)
        res = local[:self.examples].cpu().numpy().astype(np.float64)               # predictions trimmed to VALIDATION_EXAMPLES (:629-639)
        pred, gt = res[..., :3], res[..., 3:]
        gt = np.concatenate([gt, np.ones(gt.shape[:-1] + (1,))], axis=-1)         # dummy valid flag (:643-644)
        if self.is_h36m:
            actions = self.gen.table.actions[self.desc[:self.examples, 0]]
            frame, aw, _ = evaluation.h36_action_wise_eval(pred, gt, actions, root)
            metrics.update({"MPJPE": float(frame["mpjpe"]), "NMPJPE": float(frame["nmpjpe"]), "PAMPJPE": float(frame["pampjpe"]),
                            "AW-MPJPE": float(aw["mpjpe"]), "AW-NMPJPE": float(aw["nmpjpe"]), "AW-PAMPJPE": float(aw["pampjpe"])})
        else:
            frame = evaluation.frame_wise_eval(pred, gt, root)
            metrics.update({"MPJPE": float(frame["mpjpe"]), "NMPJPE": float(frame["nmpjpe"]), "PAMPJPE": float(frame["pampjpe"])})
        return loss, metrics, pred


# ---------------------------------------------------------------------------------------------------------------------------------
# checkpoints and weight files
# ---------------------------------------------------------------------------------------------------------------------------------
def latest_checkpoint(checkpoint_dir):
    """The ``cp_XXXX.npz`` of the highest epoch in ``checkpoint_dir`` -> (path, epoch), or (None, 0)."""
    best = (None, 0)
    for p in glob.glob(os.path.join(checkpoint_dir, "cp_*.npz")):
        m = re.fullmatch(r"cp_(\d+)\.npz", os.path.basename(p))
        if m and int(m.group(1)) > best[1]:
            best = (p, int(m.group(1)))
    return best


def replace_weight_file(model, checkpoint_dir, kind, epoch, previous):
    """Write ``<kind>_weights_{epoch:04d}.h5`` and delete ``previous`` (train.py:704-719) -> the new path."""
    path = os.path.join(checkpoint_dir, f"{kind}_weights_{epoch:04d}.h5")
    model.save_weights(path)
    if previous is not None and os.path.abspath(previous) != os.path.abspath(path) and os.path.exists(previous):
        os.remove(previous)
    return path


def validation_metrics(val_is_h36m):
    """train.py:450-458: the tracked metrics (all lower-is-better); the AW- ones for an H36M validation set only."""
    names = ["loss", "MPJPE", "NMPJPE", "PAMPJPE"]
    if val_is_h36m:
        names += ["AW-MPJPE", "AW-NMPJPE", "AW-PAMPJPE"]
    return names


def best_checkpoint_metric(config_metric, val_dataset_name):
    """train.py:319-320: BEST_CHECKPOINT_METRIC loses its ``AW-`` prefix when the validation set is not H36M."""
    if val_dataset_name != "h36m" and config_metric is not None:
        return config_metric.replace("AW-", "")
    return config_metric


# ---------------------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------------------
def run_epoch(trainer, stream, generator, steps, shard, loss_sum, skipped, snaps, epoch=1, log=_log):
    """The step loop of one epoch (train.py:552-574): ``steps`` batches of ``stream``, this rank's rows ``shard`` of each gathered on the
    device and trained on.  Never waits for the device: the per-step loss is added into ``loss_sum`` and the skip decision into
    ``skipped`` (device tensors); every LOG_EVERY steps the line reports the newest of the pinned copies ``snaps`` of ``loss_sum`` that
    has landed (labelled with its step) and starts the next copy."""
    import torch
    pending = []                                                             # (pinned buffer, event, step) of started copies
    epoch_start = time.time()
    lo, hi = shard
    for it in range(steps):
        tick = time.time()
        desc, cams = stream.next()
        kp2d, kp3d, smask = gather_batch(generator, desc[lo:hi], None if cams is None else cams[lo:hi])
        trainer.train_step(kp2d, kp3d, smask)
        loss_sum += trainer.loss[0]
        trainer.count_skipped(skipped)
        tock = time.time()
        if it % LOG_EVERY == 0:
            shown = ""
            while pending and pending[0][1].query():                         # (query() does not wait)
                buf, _, at = pending.pop(0)
                shown = f"Mean loss {float(buf[0]) / (at + 1):.6f} (after step {at})"
            eta = (steps - it - 1) / (it + 1) * (tock - epoch_start)
            log(f"{it}/{steps} @ Epoch {epoch} (Step {tock - tick:.3f}s, ETA {_format_time(eta)}): {shown or 'Mean loss pending'}")
            if len(pending) < len(snaps):
                buf = next(b for b in snaps if all(b is not p[0] for p in pending))
                buf.copy_(loss_sum, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                pending.append((buf, ev, it))


def run_train(config, dataset="h36m", dataset_val=None, h36m_path="./data/data_3d_h36m.npz",
              dataset_2d_path="./data/data_2d_h36m_cpn_ft_h36m_dbb.npz", amass_path=None, amass_frame_rate=50, train_subset="train",
              val_subset="val", test_subset=None, weights=None, continue_training=False, out_dir="out", log=_log, config_file=None,
              device_metrics=False):
    """train.py:264-749.  ``config``: a config object or the path of a config file (``config_file``: the file an object came from,
    which names the dumped ``<stem>_complete.json``).  Returns {"history": {metric: [(epoch, value), ...]},
    "best_weights": path or None, "last_weights": path, "test_report": eval.run_eval_multi_mask_stride(...) or None}.
    ``device_metrics``: the validation metrics and the test report are computed on the device (evaluation_device.py) instead of in numpy
    on the host: the same history within 1e-5 mm, the same weights and checkpoints.

    With torch.distributed initialised: every rank builds the same descriptor stream and trains on its contiguous shard of each global
    batch (gradients summed over the ranks, normalised by the global BATCH_SIZE: the one-rank step), validates its shard of each val
    batch (loss sums all-reduced, predictions all-gathered: every rank computes the same metrics); only rank 0 writes files."""
    import torch
    rank, world = _rank_world()
    config_path = config_file
    if isinstance(config, str):
        config_path = config
        config = UpliftUpsampleConfig(config_file=config)
    else:
        config = config.copy()
    if config.ARCH != "UpliftUpsampleTransformer":
        raise ValueError(f"ARCH {config.ARCH} is not the uplift / upsample transformer")
    dataset = dataset.lower()
    dataset_val = dataset_val.lower() if dataset_val is not None else None
    if dataset not in ("h36m", "amass") or dataset_val not in (None, "h36m", "amass"):
        raise ValueError(f"datasets must be h36m or amass, got {dataset} / {dataset_val}")
    val_dataset_name = dataset if dataset_val is None else dataset_val
    if "amass" in (dataset, dataset_val) and amass_path is None:
        raise ValueError("AMASS needs amass_path")
    if "h36m" in (dataset, dataset_val) and dataset_2d_path is None:
        raise ValueError("H36M needs dataset_2d_path")
    weights = resolve_weight_selector(weights)
    config.BEST_CHECKPOINT_METRIC = best_checkpoint_metric(config.BEST_CHECKPOINT_METRIC, val_dataset_name)
    config.AUGM_FLIP_KEYPOINT_ORDER = list(h36m.FLIP_LR_INDICES)                   # train.py:323
    checkpoint_dir = os.path.join(out_dir, "checkpoints")
    if rank == 0:
        os.makedirs(checkpoint_dir, exist_ok=True)
        stem = os.path.splitext(os.path.basename(config_path))[0] if config_path else "config"
        config.dump(os.path.join(out_dir, stem + "_complete.json"))              # train.py:326-333
    device = torch.device("cuda", torch.cuda.current_device())
    B = int(config.BATCH_SIZE)

    # ---- data (train.py:351-385) ----
    h36m_data = None
    if "h36m" in (dataset, dataset_val):
        h36m_data = h36m.load_dataset_and_2d_poses(h36m_path, dataset_2d_path, "h36m", verbose=False)
    train_val_subset = None if dataset_val is not None else val_subset
    cameras = None
    if dataset == "h36m":
        train_gen = h36m_generator(config, h36m_data, train_subset, "train", device, log)
        val_gen = h36m_generator(config, h36m_data, train_val_subset, "val", device, log) if train_val_subset is not None else None
    else:
        train_gen, cameras = amass_generator(config, amass_path, h36m_path, train_subset, "train", amass_frame_rate, cameras, device, log)
        val_gen = None
        if train_val_subset is not None:
            val_gen, cameras = amass_generator(config, amass_path, h36m_path, train_val_subset, "val", amass_frame_rate, cameras, device, log)
    if dataset_val == "h36m" and val_subset is not None:
        val_gen = h36m_generator(config, h36m_data, val_subset, "val", device, log)
    elif dataset_val == "amass" and val_subset is not None:
        val_gen, cameras = amass_generator(config, amass_path, h36m_path, val_subset, "val", amass_frame_rate, cameras, device, log)
    validation = Validation(config, val_gen, val_dataset_name == "h36m", device_metrics=device_metrics) if val_gen is not None else None
    if validation is not None:
        log(f"val batches {validation.n_batches}")
    stream = DescriptorStream(train_gen, B)
    shard = udist.shard_bounds(B, rank, world)

    # ---- model, optimizer, EMA (train.py:386-436) ----
    from .net.uplift_upsample_transformer_constructor import build_uplift_upsample_transformer
    from .trainer import Trainer
    model = build_uplift_upsample_transformer(config, device=device)
    if weights is not None:
        log(f"Loading weights from {weights}")
        model.load_weights(weights, skip_mismatch=False)
    trainer = Trainer(model, config, seed=rank)                                   # DropPath / Dropout draws: one seed per rank
    metrics = validation_metrics(val_dataset_name == "h36m")
    hist = MetricHistory()
    for m in metrics:
        hist.add_metric(m, higher_is_better=False)
    if config.BEST_CHECKPOINT_METRIC is not None and config.BEST_CHECKPOINT_METRIC not in metrics:
        raise ValueError(f"BEST_CHECKPOINT_METRIC {config.BEST_CHECKPOINT_METRIC} is not one of {metrics}")
    best_path = last_path = None
    initial_epoch = 1
    if continue_training:
        ckp, ep = latest_checkpoint(checkpoint_dir)
        if ckp is None:
            raise FileNotFoundError(f"Cant find checkpoint to continue training in {checkpoint_dir}")
        log(f"Restoring checkpoint from {ckp}")
        with np.load(ckp) as z:
            trainer.load_state_dict({k: z[k] for k in z.files if not k.startswith("run/")})
            run_state = json.loads(str(z["run/state"]))
        stream.load_state_dict(run_state["stream"])
        hist = MetricHistory.from_state_dict(run_state["history"])
        best_path, last_path = run_state["best_weights"], run_state["last_weights"]
        initial_epoch = ep + 1
        log(f"Will continue training from epoch {initial_epoch}")

    # device-side accumulators of an epoch; the 10-step log line reads pinned copies started at earlier log lines
    loss_sum = torch.zeros(1, dtype=torch.float64, device=device)
    skipped = torch.zeros(1, dtype=torch.int32, device=device)
    snaps = [torch.zeros(1, dtype=torch.float64).pin_memory() for _ in range(2)]
    history_path = os.path.join(out_dir, "history.jsonl")
    steps = int(config.STEPS_PER_EPOCH)
    for epoch in range(initial_epoch, int(config.EPOCHS) + 1):
        loss_sum.zero_()
        skipped.zero_()
        epoch_start = time.time()
        log(f"## EPOCH {epoch} / {config.EPOCHS}")
        run_epoch(trainer, stream, train_gen, steps, shard, loss_sum, skipped, snaps, epoch=epoch, log=log)
        torch.cuda.synchronize()
        epoch_duration = time.time() - epoch_start
        if world > 1:
            import torch.distributed as tdist
            tdist.all_reduce(loss_sum)                                           # shard losses are over the GLOBAL batch size: they add
        record = {"epoch": epoch}
        if steps > 0:
            train_loss = float(loss_sum.cpu()[0]) / steps
            log(f"Finished epoch {epoch} in {_format_time(epoch_duration)}, {epoch_duration / steps:.3f}s/step")
            record.update({"train/loss": train_loss, "train/LR": trainer.optimizer._value(trainer.optimizer.learning_rate),
                           "train/step_duration": epoch_duration / steps, "train/skipped_steps": int(skipped.cpu()[0])})
            if config.OPTIMIZER == "AdamW":
                record["train/WD"] = trainer.optimizer._value(trainer.optimizer.weight_decay)
            if record["train/skipped_steps"]:
                log(f"WARNING: {record['train/skipped_steps']} of {steps} steps skipped for non-finite gradients")
        trainer.export_to_model(use_ema=bool(config.EMA_ENABLED))                 # val_model (train.py:393-401)
        if validation is not None and epoch % int(config.VALIDATION_INTERVAL) == 0:
            log(f"Running validation on {validation.examples} examples")
            val_start = time.time()
            _, res, _ = validation.run(model)
            record["val_seconds"] = time.time() - val_start
            log(f"Finished validation in {_format_time(record['val_seconds'])}, loss: {res['loss']:.6f}, MPJPE: {res['MPJPE']:.2f}, "
                f"NMPJPE: {res['NMPJPE']:.2f}, PAMPJPE: {res['PAMPJPE']:.2f}, ")
            if "AW-MPJPE" in res:
                log(f"AW-MPJPE: {res['AW-MPJPE']:.2f}, AW-NMPJPE: {res['AW-NMPJPE']:.2f}, AW-PAMPJPE: {res['AW-PAMPJPE']:.2f}, ")
            for m in metrics:
                hist.add_data(m, value=res[m], step=epoch)
                record["val/" + m] = res[m]
            if config.BEST_CHECKPOINT_METRIC is not None:
                best_value, best_epoch = hist.best_value(config.BEST_CHECKPOINT_METRIC)
                if best_epoch == epoch:
                    log(f"Saving currently best checkpoint @ epoch {epoch} ({config.BEST_CHECKPOINT_METRIC}: {best_value}) as .h5")
                    new = os.path.join(checkpoint_dir, f"best_weights_{epoch:04d}.h5")
                    if rank == 0:
                        new = replace_weight_file(model, checkpoint_dir, "best", epoch, best_path)
                    best_path = new
        new = os.path.join(checkpoint_dir, f"last_weights_{epoch:04d}.h5")
        if rank == 0:
            new = replace_weight_file(model, checkpoint_dir, "last", epoch, last_path)
        last_path = new
        record["epoch_seconds"] = time.time() - epoch_start
        if epoch % int(config.CHECKPOINT_INTERVAL) == 0:
            # after validation and the weight files: the checkpoint holds everything the next epoch starts from
            state = {"stream": stream.state_dict(), "history": hist.state_dict(), "best_weights": best_path, "last_weights": last_path}
            sd = trainer.state_dict()
            if rank == 0:
                path = os.path.join(checkpoint_dir, f"cp_{epoch:04d}.npz")
                np.savez(path, **sd, **{"run/state": np.array(json.dumps(state))})
                log("Saving checkpoint to ", path)
        if rank == 0:
            with open(history_path, "a") as fh:
                fh.write(json.dumps(record, sort_keys=True) + "\n")

    if validation is not None:
        log("Best checkpoint results:")
        if config.BEST_CHECKPOINT_METRIC is not None:
            hist.print_all_for_best_metric(config.BEST_CHECKPOINT_METRIC, log=log)
        else:
            hist.print_best(log=log)
    test_report = None
    if test_subset is not None and val_dataset_name == "h36m":
        from .eval import run_eval_multi_mask_stride
        if config.BEST_CHECKPOINT_METRIC is not None and validation is not None:
            log("Eval best weights")
            eval_path = best_path
        else:
            log("Eval last weights")
            eval_path = last_path
        if world > 1:
            import torch.distributed as tdist
            tdist.barrier()                                                      # rank 0 wrote the file
        test_report = run_eval_multi_mask_stride(config, "h36m", h36m_path, dataset_2d_path, test_subset, weights_path=eval_path,
                                                 model=None, action_wise=True, log=log, device_metrics=device_metrics)
    log("Done.")
    return {"history": {m: list(hist.history[m]) for m in hist.metrics}, "best_weights": best_path, "last_weights": last_path,
            "test_report": test_report}


# ---------------------------------------------------------------------------------------------------------------------------------
# command line (train.py:194-305)
# ---------------------------------------------------------------------------------------------------------------------------------
def build_parser(extensions=False):
    """The reference's flags (train.py:200-263); ``extensions``: plus the flags this package adds (``--device_metrics``)."""
    p = argparse.ArgumentParser(description="2D-to-3D uplifting training for strided poseformer.")
    p.add_argument("--config", required=False, default=None, metavar="/path/to/config.json",
                   help="Path to the config file. Overwrites the default configs in the code.")
    p.add_argument("--gpu_id", required=False, default=None, metavar="gpu_id", help="Overwrites the GPU_ID from the config", type=str)
    p.add_argument("--dataset", required=False, default="h36m", metavar="{h36m, amass}", help="Dataset used for training")
    p.add_argument("--dataset_val", required=False, default=None, metavar="{h36m, amass}", help="Dataset used for validation")
    p.add_argument("--h36m_path", required=False, default="./data/data_3d_h36m.npz", metavar="/path/to/h36m/",
                   help="Directory of the H36m dataset")
    p.add_argument("--amass_path", required=False, default=None, metavar="/path/to/amass/", help="Directory of the AMASS dataset")
    p.add_argument("--amass_frame_rate", required=False, default="50", metavar="<r>", help="Target frame rate for amass training")
    p.add_argument("--dataset_2d_path", required=False, default="./data/data_2d_h36m_cpn_ft_h36m_dbb.npz", metavar="/path/to/2d poses/",
                   help="2D pose dataset")
    p.add_argument("--train_subset", required=False, default="train", metavar="<name of train subset>",
                   help="Name of the dataset subset to train on")
    p.add_argument("--val_subset", required=False, default="val", metavar="<name of val subset>",
                   help="Name of the dataset subset to validate on; an empty string or \"none\" disables validation.")
    p.add_argument("--test_subset", required=False, default=None, metavar="<name of test subset>",
                   help="Name of the dataset subset to test on; an empty string or \"none\" disables test evaluation.")
    p.add_argument("--weights", required=False, default=None, metavar="/path/to/weights.h5",
                   help="Path to weights .h5 file (or a file name prefix) for model weight initialization.")
    p.add_argument("--continue_training", required=False, default=False, metavar="<True|False>",
                   help="Continue a previously started training from its latest checkpoint in out_dir.")
    p.add_argument("--out_dir", required=True, metavar="/path/to/output_directory",
                   help="Logs and checkpoint directory. Also used to search for checkpoints if continue_training is set.")
    if extensions:
        p.add_argument("--device_metrics", required=False, default=False, action="store_true",
                       help="Compute the validation and test metrics on the GPU instead of in numpy on the host (same numbers within 1e-5 mm).")
    return p


def parse_args(argv=None):
    """The reference's argument clean-up (train.py:261-265, 291)."""
    args = build_parser(extensions=True).parse_args(argv)
    args.continue_training = args.continue_training not in [False, "False", "false", "f", "n", "0"]
    args.val_subset = None if args.val_subset in ["none", "None", "", 0] else args.val_subset
    args.test_subset = None if args.test_subset in ["none", "None", "", 0] else args.test_subset
    args.dataset = args.dataset.lower()
    args.dataset_val = args.dataset_val.lower() if args.dataset_val is not None else None
    args.amass_frame_rate = int(args.amass_frame_rate)
    return args


def main(argv=None):
    import torch
    args = parse_args(argv)
    expand = lambda p: None if p is None else os.path.abspath(os.path.expanduser(os.path.expandvars(p)))
    config = UpliftUpsampleConfig(config_file=expand(args.config)) if args.config else UpliftUpsampleConfig()
    if args.gpu_id is not None:
        if not args.gpu_id.isalnum():
            raise ValueError("--gpu_id must be a device number")
        config.GPU_ID = int(args.gpu_id)
    torch.cuda.set_device(int(config.GPU_ID))
    run_train(config, dataset=args.dataset, dataset_val=args.dataset_val, h36m_path=expand(args.h36m_path),
              dataset_2d_path=expand(args.dataset_2d_path), amass_path=expand(args.amass_path), amass_frame_rate=args.amass_frame_rate,
              train_subset=args.train_subset, val_subset=args.val_subset, test_subset=args.test_subset, weights=expand(args.weights),
              continue_training=args.continue_training, out_dir=expand(args.out_dir), config_file=expand(args.config),
              device_metrics=args.device_metrics)
    return 0


if __name__ == "__main__":
    sys.exit(main())
