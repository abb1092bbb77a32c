"""Trainer.train_step over long sequences (the tiled exact-f32 attention pair, csrc/uu3d_attn_long.h): dense_351 (351 tokens) and
dense_351 with SEQUENCE_STRIDE 2 (176 tokens), batch 32, timed with device events after a warm-up.  One JSON line per config.

    python tools/train_long_bench.py [--batch 32] [--steps 10] [--warmup 3]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import uplift_upsample_3dhpe_amd as pkg  # noqa: E402
from uplift_upsample_3dhpe_amd import synthetic  # noqa: E402
from uplift_upsample_3dhpe_amd.trainer import Trainer  # noqa: E402


def config(stride):
    cfg = synthetic.load_config("dense_351")
    if stride != 1:
        cfg.SEQUENCE_STRIDE = stride
        cfg.SEQUENCE_LENGTH = (351 - 1) // stride + 1            # 176 tokens at stride 2, 351-frame receptive field
        cfg.STRIDES, cfg.PADDINGS = [4, 4, 11], [[0, 0], [0, 0], [0, 0]]
    return cfg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    for stride in (1, 2):
        cfg = config(stride)
        arch = pkg.arch_from_config(cfg)
        w = pkg.init_weights(arch, seed=0, perturb=0.05)
        tr = Trainer(pkg.build_uplift_upsample_transformer(cfg, weights=w), cfg, seed=0)
        x, m = synthetic.synthetic_batch(cfg, a.batch, seed=1)
        gt = np.random.default_rng(2).normal(0, 0.3, size=(a.batch, arch.num_frames, 17, 3)).astype(np.float32)
        args = (torch.from_numpy(x).cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(m).cuda())
        for _ in range(a.warmup):
            tr.train_step(*args)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            loss = tr.train_step(*args)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.steps
        print(json.dumps({"config": "dense_351" if stride == 1 else "dense_351_stride2", "tokens": arch.num_frames, "batch": a.batch,
                          "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(ms, 3),
                          "sequences_per_s": round(a.batch / ms * 1e3, 1), "loss_finite": bool(torch.isfinite(loss).all())}), flush=True)
        del tr


if __name__ == "__main__":
    main()
