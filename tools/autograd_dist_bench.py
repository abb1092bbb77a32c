"""Custom-loss training steps (zero_grad, model(..., training=True), a torch MPJPE, loss.backward(), apply_gradients) against
Trainer.train_step on h36m_351, timed with device events after a warm-up; one JSON line per measurement.

    python tools/autograd_dist_bench.py [--batch 64] [--steps 20] [--warmup 5]          # one rank
    python tools/autograd_dist_bench.py --world 8                                       # 8 ranks over RCCL (needs 8 GPUs)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/autograd_dist_bench.py --kernel
    python tools/autograd_dist_bench.py --summarize DIR                                  # scale_accumulate_kernel from that trace
                                                                                        # (same --steps / --warmup as the --kernel run)

With one rank the custom-loss step runs the plain tape backward.  With N > 1 it runs the accumulating backward whose ranges are
all-reduced while it runs.  --kernel runs only the accumulating tape backward (uu3d_train_backward_tape_accumulate, one rank, no
collectives), for a kernel trace of its unscale-and-add kernel in a profiling run of its own.
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def setup(batch, global_batch, rank=0):
    import numpy as np
    import torch
    import uplift_upsample_3dhpe_amd as pkg
    from uplift_upsample_3dhpe_amd import synthetic
    cfg = synthetic.load_config("h36m_351")
    cfg.BATCH_SIZE = global_batch
    arch = pkg.arch_from_config(cfg)
    model = pkg.build_uplift_upsample_transformer(cfg, weights=pkg.init_weights(arch, seed=0, perturb=0.05))
    x, m = synthetic.synthetic_batch(cfg, batch, seed=1 + rank)
    x = x * m[:, :, None, None].astype(np.float32)
    gt = np.random.default_rng(2 + rank).normal(0, 0.3, size=(batch, arch.num_frames, 17, 3)).astype(np.float32)
    return cfg, model, tuple(torch.from_numpy(a).cuda() for a in (x, gt, m))


def mpjpe(full, central, gt, cfg):
    import torch
    r, N, J = int(cfg.ROOT_KEYTPOINT), full.shape[1], full.shape[2]
    rel = lambda p: p - p[..., r:r + 1, :]                                    # noqa: E731
    seq = torch.linalg.vector_norm(rel(full) - rel(gt), dim=-1).sum() / (cfg.BATCH_SIZE * N * J)
    cen = torch.linalg.vector_norm(rel(central) - rel(gt[:, N // 2]), dim=-1).sum() / (cfg.BATCH_SIZE * J)
    return cfg.LOSS_WEIGHT_SEQUENCE * seq + cfg.LOSS_WEIGHT_CENTER * cen


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def steps(a, world, rank):
    import torch
    from uplift_upsample_3dhpe_amd.trainer import Trainer
    cfg, model, (x, gt, m) = setup(a.batch, a.batch * world, rank)
    tr = Trainer(model, cfg)
    ms_builtin = timed(lambda: tr.train_step(x, gt, m), a.steps, a.warmup)
    model.requires_grad_()

    def custom():
        tr.zero_grad()
        full, central = model([x, m], training=True)
        mpjpe(full, central, gt, cfg).backward()
        tr.apply_gradients()
    ms_custom = timed(custom, a.steps, a.warmup)
    if rank == 0:
        print(json.dumps({"config": "h36m_351", "world": world, "batch_per_rank": a.batch, "steps": a.steps, "warmup": a.warmup,
                          "train_step_ms": round(ms_builtin, 3), "custom_loss_step_ms": round(ms_custom, 3),
                          "custom_over_builtin": round(ms_custom / ms_builtin, 3),
                          "path": "accumulating tape backward, bucketed all-reduce" if world > 1 else "plain tape backward"}), flush=True)
    del tr, model
    torch.cuda.empty_cache()


def kernel_only(a):
    """Tape forward once, then accumulating backward passes: the trace holds scale_accumulate_kernel once per finished range."""
    import torch
    cfg, model, (x, gt, m) = setup(a.batch, a.batch)
    model.requires_grad_()
    lib = model._lib
    full, central, tape = model._tape_forward(x, model._mask_u8(m))
    gF, gC = torch.randn_like(full) * 1e-3, torch.randn_like(central) * 1e-2
    n = int(lib.uu3d_num_params(model._h))
    scratch, acc = torch.empty(n, device="cuda"), torch.zeros(n, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())                                    # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    run = lambda: lib.uu3d_train_backward_tape_accumulate(model._h, tape.handle, p(gF), p(gC), p(scratch), p(acc), None, 0, stream)  # noqa: E731
    ms = timed(run, a.steps, a.warmup)
    print(json.dumps({"config": "h36m_351", "batch": a.batch, "params": n, "accumulating_tape_backward_ms": round(ms, 3)}), flush=True)


def summarize(d, passes):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            rows += [r for r in csv.DictReader(fh) if "scale_accumulate_kernel" in r.get("Name", "")]
    if not rows:
        raise SystemExit(f"no scale_accumulate_kernel in the kernel statistics under {d}")
    calls = sum(int(r["Calls"]) for r in rows)
    total_ns = sum(float(r["TotalDurationNs"]) for r in rows)
    print(json.dumps({"kernel": "scale_accumulate_kernel", "calls": calls, "mean_us_per_call": round(total_ns / calls / 1e3, 2),
                      "us_per_backward": round(total_ns / passes / 1e3, 2), "total_us": round(total_ns / 1e3, 1),
                      "min_us": round(min(float(r["MinNs"]) for r in rows) / 1e3, 2),
                      "max_us": round(max(float(r["MaxNs"]) for r in rows) / 1e3, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--world", type=int, default=1)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--summarize", default=None)
    ap.add_argument("--rank", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--port", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize, a.steps + a.warmup)       # (the --steps / --warmup of the --kernel run)
    if a.kernel:
        return kernel_only(a)
    if a.rank is not None:                                                    # one rank of --world N
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(a.rank)
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{a.port}", rank=a.rank, world_size=a.world)
        steps(a, a.world, a.rank)
        dist.destroy_process_group()
        return
    if a.world == 1:
        return steps(a, 1, 0)
    import torch
    if torch.cuda.device_count() < a.world:
        print(json.dumps({"world": a.world, "skipped": f"{torch.cuda.device_count()} GPU(s) visible"}), flush=True)
        return
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    base = [sys.executable, os.path.abspath(__file__), "--batch", str(a.batch), "--steps", str(a.steps), "--warmup", str(a.warmup),
            "--world", str(a.world), "--port", str(port)]
    procs = [subprocess.Popen(base + ["--rank", str(r)]) for r in range(a.world)]
    codes = [p.wait() for p in procs]
    if any(codes):
        raise SystemExit(f"rank exit codes {codes}")


if __name__ == "__main__":
    main()
