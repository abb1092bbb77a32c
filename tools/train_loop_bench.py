"""run_train's step loop against a bare loop of Trainer.train_step, steady state, on seeded synthetic pose tracks (no dataset).

  run_train : train.run_epoch -- what run_train runs between two validations: the descriptor stream (repeat().batch(B)), the on-device
              window gather from a resident pose table, Trainer.train_step, the device-side loss sum and skip count, the 10-step log line
  bare      : Trainer.train_step on ONE resident batch, nothing else

The two loops alternate in one process (``--rounds`` times) on one model; each timed run is ``--steps`` steps after ``--warmup``.
Reports sequences/s of both and their ratio per case, plus the projected time of a full epoch of the config (STEPS_PER_EPOCH x BATCH).
   python tools/train_loop_bench.py [--cases h36m_351_pt:64,h36m_351_pt:512,h36m_81:256] [--steps 200] [--rounds 3]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="h36m_351_pt:64,h36m_351_pt:512,h36m_81:256")
    ap.add_argument("--videos", type=int, default=40)
    ap.add_argument("--frames", type=int, default=2500)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    from uplift_upsample_3dhpe_amd import synthetic as util
    from uplift_upsample_3dhpe_amd import train as T
    from uplift_upsample_3dhpe_amd.data import DescriptorStream, PoseTable, SequenceGenerator
    from uplift_upsample_3dhpe_amd.trainer import Trainer
    import uplift_upsample_3dhpe_amd as pkg
    rng = np.random.default_rng(0)
    # smooth tracks: a random walk per joint (2D input and 3D target; the values do not change the cost)
    p2 = [np.cumsum(rng.normal(0, 0.01, size=(args.frames, 17, 2)), 0).astype(np.float32) + rng.uniform(-0.5, 0.5, size=(1, 17, 2)).astype(np.float32)
          for _ in range(args.videos)]
    p3 = [np.cumsum(rng.normal(0, 0.005, size=(args.frames, 17, 3)), 0).astype(np.float32) + rng.normal(0, 0.3, size=(1, 17, 3)).astype(np.float32)
          for _ in range(args.videos)]
    out = []
    quiet = lambda *a: None
    for case in args.cases.split(","):
        name, batch = case.split(":")
        cfg = util.load_config(name)
        full_epoch_steps = int(cfg.STEPS_PER_EPOCH)
        cfg.BATCH_SIZE = int(batch)
        arch = pkg.arch_from_config(cfg)
        model = pkg.build_uplift_upsample_transformer(cfg, weights=pkg.init_weights(arch, seed=0, perturb=0.05))
        tr = Trainer(model, cfg)
        table = PoseTable(p2, p3, device=model.device)
        gen = SequenceGenerator(table, seq_len=cfg.SEQUENCE_LENGTH, **T._split_options(cfg, "train"), flip_lr_indices=cfg.AUGM_FLIP_KEYPOINT_ORDER)
        stream = DescriptorStream(gen, cfg.BATCH_SIZE)
        stream.next()                                      # (the first generator epoch's descriptors: built once, outside the timing)
        loss_sum = torch.zeros(1, dtype=torch.float64, device=model.device)
        skipped = torch.zeros(1, dtype=torch.int32, device=model.device)
        snaps = [torch.zeros(1, dtype=torch.float64).pin_memory() for _ in range(2)]
        kp2d, kp3d, sm = T.gather_batch(gen, stream.next()[0])
        kp2d, kp3d, sm = kp2d.clone(), kp3d.clone(), sm.clone()

        def loop(steps):
            T.run_epoch(tr, stream, gen, steps, (0, cfg.BATCH_SIZE), loss_sum, skipped, snaps, log=quiet)

        def bare(steps):
            for _ in range(steps):
                tr.train_step(kp2d, kp3d, sm)
        res = {"loop": [], "bare": []}
        for r in range(args.rounds):
            for key, fn in (("loop", loop), ("bare", bare)) if r % 2 == 0 else (("bare", bare), ("loop", loop)):
                fn(args.warmup)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(args.steps)
                torch.cuda.synchronize()
                res[key].append(cfg.BATCH_SIZE * args.steps / (time.perf_counter() - t0))
        loop_rate, bare_rate = float(np.median(res["loop"])), float(np.median(res["bare"]))
        row = {"config": name, "batch": cfg.BATCH_SIZE, "steps": args.steps, "rounds": args.rounds,
               "run_train_seq_per_s": round(loop_rate, 1), "bare_seq_per_s": round(bare_rate, 1),
               "ratio": round(loop_rate / bare_rate, 4), "per_round_ratio": [round(a / b, 4) for a, b in zip(res["loop"], res["bare"])],
               "full_epoch_s": round(full_epoch_steps * cfg.BATCH_SIZE / loop_rate, 1), "full_epoch_steps": full_epoch_steps,
               "skipped_steps": int(skipped.cpu()[0])}
        print(json.dumps(row), flush=True)
        out.append(row)
        del tr, model
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    main()
