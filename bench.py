"""Throughput of the uplift/upsample transformer forward on synthetic (B, N, 17, 2) windows.

    python bench.py --gpus 1 --steps 50 --warmup 10
    python bench.py --gpus N ...                 # starts its own N ranks (child processes, before the parent touches a GPU)
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...     # or under a launcher
    python bench.py --config dense_351 --batch 32 --full # SURVEY 8(d)'s stress shape: temporal attention over 351 tokens
    python bench.py --full                       # + per-kernel timing / roofline, CPU baseline, parity vs the oracle, secondary workloads
    python bench.py --dump-outputs DIR           # + the last timed step's outputs as DIR/<name>.npy

One step = one forward of `--batch` sequences per rank (inputs resident in HBM) + the
per-joint MPJPE kernel; with N > 1 ranks the batch is sharded (weak scaling: every rank
runs `--batch` sequences) and each step all-gathers the (B_local, 17) f64 error block over
RCCL.  Prints ONE JSON line on rank 0 (see DESIGN.md "Measurement").  A plain run sets up,
warms up, times `--steps` steps and prints the line; everything else it can measure or
check runs only under `--full`.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# The temporal chain's kernel (csrc/uu3d_tchain16.h): token rows and threads per workgroup
TC_ROWS, TC_THREADS, TC_KERNEL = 64, 512, "tchain16_kernel"
PEAK_F32_MFMA_TFLOPS = 157.3   # /opt/skills/guides/MI355X_MICROARCH.md "Peak FP32 (matrix)"
PEAK_F16_MFMA_TFLOPS = 2500.0  # same table, "Peak BF16/FP16 MFMA ~2.5 PF dense"
# What the leave-one-out builds of the dominant kernel say bounds it (profiles/): `bound` above stays the roofline the FLOPs are priced
# against (the contract's "mfma"), this is the measured limiter.
BOUND_MEASURED = ("LDS fragment reads, two lock-step barriers per chunk and the clock the chip holds on its 1400 W power cap (2.15 GHz under the bench loop, profiles/r06_power.txt): leave-one-out builds of the chain (eight waves on "
                  "16-token panels, csrc/uu3d_tchain16.h) with every CU busy / one launch alone (profiles/r06_ab_tchain16.txt) -- complete 253 / 103 us, without the "
                  "ring's LDS-DMA refills 222 / 92, without the epilogues 202 / 84, neither 178 / 72: the bare loop runs at ~1.55 k cycles per chunk for 1.15 k of MFMA; "
                  "no float atomics, no lane-private round trips: 122 MB of counter traffic per launch against 119 MB algorithmic")


def cpu_baseline(cfg, arch, weights, x, m, budget_s=60.0):
    """Oracle ("port": PyTorch-CPU fp32 restatement) timed on the host cores at the BENCH batch (BASELINE.md section 4:
    same synthetic batch, 3 warm-ups, median of >= 10 forwards -- as far as `budget_s` allows; the counts reached are in
    `sample`).  Eager PyTorch on a many-core host is NOT fastest with every core (256 threads: 81 s per forward of 128
    sequences on the GPU box, contention in the many small matmuls), so the thread count is swept first on a 16-sequence
    sample (ascending, stops when it gets slower) and stated in the result."""
    import statistics
    import torch
    from oracle import uplift_oracle as O
    hp = O.hp_from_arch(arch)
    t_start = time.time()
    ncpu = os.cpu_count() or 1
    ns = min(16, x.shape[0])
    sweep, best, best_t = {}, None, None
    for t in ([c for c in (4, 8, 16, 32, 64, 128, 256) if c <= ncpu] or [ncpu]):      # a host with < 4 threads: just all of them
        torch.set_num_threads(t)
        O.forward(hp, weights, x[:ns], m[:ns], torch.float32)                  # thread-pool start / page in
        t0 = time.time(); O.forward(hp, weights, x[:ns], m[:ns], torch.float32); dt = time.time() - t0
        sweep[t] = dt
        if best_t is None or dt < best_t:
            best, best_t = t, dt
        elif dt > 1.5 * best_t or time.time() - t_start > budget_s / 4:
            break
    torch.set_num_threads(best)
    warm, times = 0, []
    while warm < 3 and time.time() - t_start < budget_s * 0.4 and best_t * x.shape[0] / ns < budget_s * 0.2:
        O.forward(hp, weights, x, m, torch.float32); warm += 1
    # the sample shrinks (whole sequences) when one forward of the bench batch would not fit the budget twice: bounded CPU time
    nb = x.shape[0]
    est = best_t * nb / ns
    if 2 * est > budget_s:
        nb = max(ns, int(nb * budget_s / (2 * est)))
    xs, ms_ = x[:nb], m[:nb]
    while len(times) < 10 and (len(times) < 2 or time.time() - t_start < budget_s):
        t0 = time.time(); O.forward(hp, weights, xs, ms_, torch.float32); times.append(time.time() - t0)
    med = statistics.median(times)
    x = xs
    return {"value": round(x.shape[0] / med, 2), "unit": "pose-sequences/s", "cores": int(best), "kind": "port",
            "host_cores": int(ncpu), "thread_sweep_s_per_16_sequences": {str(k): round(v, 3) for k, v in sweep.items()},
            "sample": f"median of {len(times)} forwards of the bench batch ({x.shape[0]} sequences) after {warm} warm-ups, "
                      f"PyTorch-CPU fp32 oracle (oracle/uplift_oracle.py) on {best} of {ncpu} hardware threads (fastest of the sweep)"}


class ErrorGather:
    """The multi-GPU payload of a step: its (B_local, J) float64 per-joint error block, all-gathered over the ranks.

    mode "end" (default): every step's block is kept in a (steps, B, J) buffer (one small device copy per step, enqueued behind the
    step's result) and ONE collective of the whole buffer runs after the loop's last result, inside the timed region -- nothing of the
    data path waits for a collective.  mode "step": one all-gather per step on the caller's stream (the round-4 behaviour, kept for
    A/B runs).  Without a process group both modes only keep the blocks."""

    def __init__(self, mode, steps, B, J, world, device, use_dist):
        import torch
        if mode not in ("end", "step"):
            raise ValueError("gather mode: end | step")
        self.mode, self.world, self.use_dist = mode, int(world), bool(use_dist)
        self.local = torch.empty((max(steps, 1), B, J), dtype=torch.float64, device=device)
        self.gathered = torch.empty((self.world * self.local.shape[0],) + tuple(self.local.shape[1:]), dtype=torch.float64, device=device) if use_dist else None   # rank-major: (world * steps, B, J)
        self.step_out = torch.empty((self.world * B, J), dtype=torch.float64, device=device) if (use_dist and mode == "step") else None
        self.k = 0

    def reset(self):
        self.k = 0

    def step(self, e):
        import torch.distributed as dist
        self.local[self.k % self.local.shape[0]].copy_(e, non_blocking=True)
        self.k += 1
        if self.use_dist and self.mode == "step":
            dist.all_gather_into_tensor(self.step_out, e)

    def finish(self):
        """mode "end": the one collective; returns the (world, steps, B, J) blocks (or None without a process group)."""
        import torch.distributed as dist
        if self.use_dist and self.mode == "end":
            dist.all_gather_into_tensor(self.gathered, self.local)
        return None if self.gathered is None else self.gathered.view((self.world,) + tuple(self.local.shape))


# UU3D_* variables that make the library compute something else than the forward (timing experiments of tools/; they only act in
# a -DUU3D_TIMING_BUILD library, but a bench line must not be produced under them at all)
FORBIDDEN_ENV = ("UU3D_SKIP", "UU3D_TIMING_PARTS")


def env_switches(timing_experiment=False):
    """Every UU3D_* variable present in this process's environment (A/B switches of the library and of this script): recorded in the
    JSON line, so that a number measured under a switch says so; the result-changing ones are refused (except under --timing-experiment,
    whose line is labelled as not a result)."""
    present = {k: v for k, v in sorted(os.environ.items()) if k.startswith("UU3D_")}
    bad = [k for k in present if k in FORBIDDEN_ENV]
    if bad and not timing_experiment:
        raise SystemExit(f"bench.py refuses to run with {', '.join(bad)} set: those switches skip launches (timing experiments, results wrong)")
    return present


def emit_line(out):
    """The ONE JSON line, as the LAST thing on stdout: RCCL prints its version banner through C stdio, which is block-buffered on a pipe and
    would otherwise come out at process exit, behind the line."""
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:  # pragma: no cover
        pass
    print(json.dumps(out), flush=True)


def run_pipelined_steps(pipe, n, depth, gather):
    """n steps with `depth` batches in flight: launch() a slot, take the oldest result when `depth` are out, hand its error block to
    `gather`; the collective of gather mode "end" closes the loop.  (`pipe`: launch() -> ticket, result(ticket) -> (full, central, err),
    after(ticket, fn) -> fn(full, central, err) on the slot's stream, join().)  Gather mode "end" keeps the block with a copy ON THE SLOT'S
    STREAM (pipe.after: no wait on the caller's stream, whose hardware queue a quarter of the slots share); the caller's stream joins the
    slots before the collective.  Mode "step" needs the block on the caller's stream every step (pipe.result).
    Returns (full, central, err) of the last step: the slot's buffers, valid until the pipeline launches again."""
    gather.reset()
    on_slot = gather.mode == "end"

    def keep(full, central, e):
        gather.step(e)
        return full, central, e

    def take(t):
        return pipe.after(t, keep) if on_slot else keep(*pipe.result(t))
    tickets = []
    last = None
    free = on_slot and not os.environ.get("UU3D_BENCH_WAIT_CALLER")      # (inputs resident in the slots, consumer on the slot's stream: nothing on the caller's stream to wait for)
    for _ in range(n):
        tickets.append(pipe.launch(wait_caller=False) if free else pipe.launch())
        if len(tickets) == depth:
            last = take(tickets.pop(0))
    for t in tickets:
        last = take(t)
    pipe.join()
    gather.finish()
    return last


# --dump-outputs: at most this many bytes of .npy files in all
DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, arrays, seed=0):
    """--dump-outputs: every array of `arrays` (name -> numpy array or None) as <path>/<name>.npy in float32 / float64 (other dtypes are
    widened to float64), in order.  An array that would take the total past DUMP_LIMIT_BYTES is replaced by a fixed, seeded sample of its
    flattened elements (same size and seed: same indices), so that two builds run with the same arguments compare output for output.
    Returns {name: shape written}."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    left, header = DUMP_LIMIT_BYTES, 128                     # (np.save writes a header of 128 bytes in front of the data)
    written = {}
    for name, a in arrays.items():
        if a is None:
            continue
        a = np.ascontiguousarray(a)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        if a.nbytes + header > left:
            k = min(a.size, max(0, (left - header) // a.itemsize))
            idx = np.sort(np.random.default_rng(seed).choice(a.size, size=k, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(path, name + ".npy"), a)
        left -= a.nbytes + header
        written[name] = list(a.shape)
    return written


def parity_vs_oracle(cfg, arch, weights, x, m, full, central, gt, n=8, idx=None):
    """BASELINE's metric names "MPJPE vs ref": the HIP outputs of the bench batch (what the timed pipeline produced) against the CPU oracle on
    its first `n` sequences, OUTSIDE the timed region -- max-abs over both outputs and the difference of the two MPJPEs against the synthetic
    ground truth (mm; the north_star's budget is 0.05 mm).  The oracle is the checker here, never the thing measured."""
    import numpy as np
    import torch
    from oracle import uplift_oracle as O
    if idx is None:
        idx = list(range(min(n, x.shape[0])))
    idx = np.asarray(idx, dtype=np.int64)
    f32, c32 = O.forward(O.hp_from_arch(arch), weights, x[idx], m[idx], torch.float32)
    e = float(np.abs(central[idx] - c32).max())
    if full is not None and f32 is not None:
        e = max(e, float(np.abs(full[idx] - f32).max()))
    _, a = O.frame_mpjpe_mm(central[idx], gt[idx][:, :, :3], cfg.ROOT_KEYTPOINT)
    _, b = O.frame_mpjpe_mm(c32, gt[idx][:, :, :3], cfg.ROOT_KEYTPOINT)
    return {"max_abs_vs_oracle": e, "mpjpe_delta_mm": float(abs(a - b)), "n_sequences": int(len(idx)), "sequence_indices": [int(i) for i in idx],
            "tolerance_max_abs": 1e-4, "budget_mpjpe_mm": 0.05,
            "reference": "oracle/uplift_oracle.py (PyTorch-CPU fp32 restatement; parity UNPINNED against TensorFlow, DESIGN.md section 6)"}


def train_bench(args, world, rank, local_rank, use_dist):
    """BASELINE config 5: config/h36m_351_pt.json train step on synthetic AMASS-shaped sequences."""
    import numpy as np
    import torch
    import torch.distributed as dist
    import uplift_upsample_3dhpe_amd as pkg
    from uplift_upsample_3dhpe_amd import synthetic as util
    from uplift_upsample_3dhpe_amd import harness
    from uplift_upsample_3dhpe_amd.trainer import Trainer
    cfgname = args.config if args.config != "h36m_351" else "h36m_351_pt"
    cfg = util.load_config(cfgname)
    B = args.batch if args.batch != 128 else 64            # JSON BATCH_SIZE 512 global = 64 per GPU on 8
    cfg.BATCH_SIZE = B * world                             # loss normaliser = global batch (train.py:482)
    arch = pkg.arch_from_config(cfg)
    model = pkg.build_uplift_upsample_transformer(cfg, weights=pkg.init_weights(arch, seed=0), device=f"cuda:{local_rank}",
                                                   precision=args.precision)
    tr = Trainer(model, cfg, seed=100 + rank)
    rng = np.random.default_rng(3000 + rank)
    N, J = arch.num_frames, arch.num_keypoints
    x = torch.from_numpy(rng.uniform(-1, 1, size=(B, N, J, 2)).astype(np.float32)).cuda()
    gt = torch.from_numpy(rng.normal(0, 0.3, size=(B, N, J, 3)).astype(np.float32)).cuda()
    m = torch.from_numpy(harness.stride_masks_train(N, cfg.SEQUENCE_STRIDE, cfg.MASK_STRIDE, B, rng, cfg.STRIDE_MASK_RAND_SHIFT)).cuda()

    def sync_all():
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
            torch.cuda.synchronize()
    for _ in range(args.warmup):
        tr.train_step(x, gt, m)
    sync_all()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = tr.train_step(x, gt, m)
    enqueue = time.perf_counter() - t0                         # host time to launch the steps (no synchronisation inside a step)
    sync_all()
    elapsed = time.perf_counter() - t0
    if use_dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank == 0 and args.dump_outputs:
        # what the last timed step hands back: its loss and the weights it updated
        dump_outputs(args.dump_outputs, {"loss": loss.double().cpu().numpy(), "params": tr.params.cpu().numpy()})
    if rank == 0:
        fl = pkg.flops_per_sequence(arch)["total"] * 3.0       # forward + backward ~ 3x forward GEMM FLOPs
        seqs = world * B * args.steps
        emit_line({
            "metric": "train-sequences/sec", "value": round(seqs / elapsed, 2), "unit": "pose-sequences/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": ("f16x3 forward / input-gradient / weight-gradient GEMMs (UU3D_TN_F32=1: f32 weight gradients), f32 attention, loss, optimizer"
                      if args.precision == "f16x3" and not os.environ.get("UU3D_TRAIN_F32") else "f32"),
            "data": "synthetic",
            "config": {"workload": f"config/{cfgname}.json train step (fwd+bwd+AdamW), N={N}, J={J}, batch {B}/GPU, "
                                   f"per-sample mask stride from {cfg.MASK_STRIDE}, DropPath {cfg.DROP_PATH_RATE}",
                       "global_batch": world * B, "parallelism": f"data-parallel x{world}, flat f32 gradient all-reduce"},
            "host_enqueue_ms_per_step": round(enqueue / args.steps * 1e3, 3), "model_tflops_3x_fwd": round(fl * seqs / world / elapsed / 1e12, 2), "loss": float(loss[0].item())})
    if use_dist:
        dist.destroy_process_group()




def quick_forward_bench(cfgname, batch, s_in=None, streams=1, graph=True, steps=40, warmup=10, precision="f16x3", attention=False, copy_inputs=False, parity=True):
    """A short timing of another workload for the `secondary` block of the bench line (same process, same GPU): sequences/s and
    ms per step of the forward + error kernel, `streams` batches in flight; attention=True adds the temporal-attention launch's
    HIP-event time and its fraction of the MFMA peak."""
    import numpy as np
    import torch
    import uplift_upsample_3dhpe_amd as pkg
    from uplift_upsample_3dhpe_amd import synthetic as util
    from uplift_upsample_3dhpe_amd.harness import per_joint_error
    cfg = util.load_config(cfgname)
    arch = pkg.arch_from_config(cfg)
    model_weights = pkg.init_weights(arch, seed=0)
    model = pkg.build_uplift_upsample_transformer(cfg, weights=model_weights, precision=precision)
    s_in = s_in or (cfg.MASK_STRIDE[0] if isinstance(cfg.MASK_STRIDE, list) else cfg.MASK_STRIDE)
    x_np, m_np = util.synthetic_batch(cfg, batch, seed=1000, mask_specs=[(s_in, 0)])
    x = torch.from_numpy(x_np * m_np[:, :, None, None].astype(np.float32)).cuda()
    m = torch.from_numpy(m_np).cuda()
    J = arch.num_keypoints
    gt = torch.cat([torch.randn(batch, J, 3, device="cuda") * 0.3, torch.ones(batch, J, 1, device="cuda")], -1)
    errs = [torch.empty((batch, J), dtype=torch.float64, device="cuda") for _ in range(streams)]
    pipe = model.pipeline(batch, depth=streams, graph=graph, post=lambda f, c, i: per_joint_error(c, gt, cfg.ROOT_KEYTPOINT, out=errs[i]))

    pipe.preload(x, m)                                   # the batch is resident in every slot's input buffers: no per-step copy

    # the headline's loop shape: resident inputs -> the slot's stream never waits for the caller's, the (empty) consumer runs on the slot's stream
    take = (lambda t: pipe.result(t)) if copy_inputs else (lambda t: pipe.after(t, lambda *a: None))

    def run(n):
        tickets = []
        for _ in range(n):
            # copy_inputs: the batch is copied into the slot's input buffers every step (pipe.submit: the rounds-1-3 methodology, and what a
            # caller without a device-side producer pays); else it is resident (pipe.launch: the headline's methodology since round 4)
            tickets.append(pipe.submit(x, m) if copy_inputs else pipe.launch(wait_caller=False))
            if len(tickets) == streams:
                take(tickets.pop(0))
        for t in tickets:
            take(t)
        pipe.join()
    run(warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = {"workload": f"config/{cfgname}.json, batch {batch}, s_in {s_in}" if cfgname != "dense_351" else f"synthetic dense-351 (NOT a shipped config), batch {batch}",
           "value": round(batch * steps / dt, 1), "unit": "pose-sequences/s", "ms_per_step": round(1e3 * dt / steps, 4), "steps": steps,
           "batches_in_flight": streams, "hipgraph": bool(graph), "input": "copied into the slot every step (submit)" if copy_inputs else "resident in the slots (preload + launch)"}
    if parity:
        # what THIS timed path produces for its resident batch, against the oracle on sequences of the first, a middle and the last row tile
        try:
            f_, c_, _ = pipe.result(pipe.submit(x, m) if copy_inputs else pipe.launch())
            torch.cuda.synchronize()
            idx = sorted({0, 1, batch // 2, batch - 1} if cfgname == "dense_351" else {0, 1, batch // 2 - 1, batch // 2, batch - 2, batch - 1})
            idx = [i for i in idx if 0 <= i < batch]
            out["parity"] = parity_vs_oracle(cfg, arch, model_weights, x_np * m_np[:, :, None, None].astype(np.float32), m_np,
                                             f_.cpu().numpy() if f_ is not None else None, c_.cpu().numpy(), gt.cpu().numpy(), idx=idx)
        except Exception as e:  # pragma: no cover
            out["parity"] = {"error": f"{type(e).__name__}: {e}"}
    if attention:
        model.set_profiling(True)
        agg = {}
        for _ in range(3):
            model([x, m], training=False)
            for e in model.read_profile():
                nm = e["name"]
                key = ("t." + nm.split(".", 1)[1]) if (nm[0] == "t" and "." in nm) else nm
                a = agg.setdefault(key, dict(ms=0.0, flops=0.0, bytes=0.0, n=0, kernel=e["kernel"]))
                a["ms"] += e["ms"]; a["flops"] += e["flops"]; a["n"] += 1
        model.set_profiling(False)
        out["attention"] = attention_roofline(agg, arch.num_frames, out["workload"])
    del pipe, model
    torch.cuda.empty_cache()
    return out


def quick_model_call_bench(cfgname, batch, steps=40, warmup=5):
    """What a caller that loops over ``model([x, mask])`` pays per call (eager launches, the LATENCY schedule, default range_guard=True:
    one stream synchronisation + a 4-byte device-to-host copy behind every call) -- and the same loop with range_guard=False."""
    import numpy as np
    import torch
    import uplift_upsample_3dhpe_amd as pkg
    from uplift_upsample_3dhpe_amd import synthetic as util
    cfg = util.load_config(cfgname)
    arch = pkg.arch_from_config(cfg)
    w = pkg.init_weights(arch, seed=0)
    s_in = cfg.MASK_STRIDE[0] if isinstance(cfg.MASK_STRIDE, list) else cfg.MASK_STRIDE
    x_np, m_np = util.synthetic_batch(cfg, batch, seed=1000, mask_specs=[(s_in, 0)])
    x = torch.from_numpy(x_np * m_np[:, :, None, None].astype(np.float32)).cuda()
    m = torch.from_numpy(m_np).cuda()
    out = {"workload": f"config/{cfgname}.json, batch {batch}: a Python loop over model([x, mask]) (eager, latency schedule)"}
    for guard in (True, False):
        model = pkg.build_uplift_upsample_transformer(cfg, weights=w, range_guard=guard)
        for _ in range(warmup):
            model([x, m], training=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            model([x, m], training=False)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out["range_guard_on" if guard else "range_guard_off"] = {"value": round(batch * steps / dt, 1), "unit": "pose-sequences/s", "ms_per_call": round(1e3 * dt / steps, 4)}
        del model
    torch.cuda.empty_cache()
    return out


def quick_train_bench(steps=50, warmup=10, batch=64):
    """BASELINE config 5 (config/h36m_351_pt.json train step: fwd + bwd + AdamW) at world size 1, for the `secondary` block."""
    import numpy as np
    import torch
    import uplift_upsample_3dhpe_amd as pkg
    from uplift_upsample_3dhpe_amd import synthetic as util
    from uplift_upsample_3dhpe_amd import harness
    from uplift_upsample_3dhpe_amd.trainer import Trainer
    cfg = util.load_config("h36m_351_pt")
    cfg.BATCH_SIZE = batch
    arch = pkg.arch_from_config(cfg)
    model = pkg.build_uplift_upsample_transformer(cfg, weights=pkg.init_weights(arch, seed=0))
    tr = Trainer(model, cfg, seed=100)
    rng = np.random.default_rng(3000)
    N, J = arch.num_frames, arch.num_keypoints
    x = torch.from_numpy(rng.uniform(-1, 1, size=(batch, N, J, 2)).astype(np.float32)).cuda()
    gt = torch.from_numpy(rng.normal(0, 0.3, size=(batch, N, J, 3)).astype(np.float32)).cuda()
    m = torch.from_numpy(harness.stride_masks_train(N, cfg.SEQUENCE_STRIDE, cfg.MASK_STRIDE, batch, rng, cfg.STRIDE_MASK_RAND_SHIFT)).cuda()
    for _ in range(warmup):
        tr.train_step(x, gt, m)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = tr.train_step(x, gt, m)
    enqueue = time.perf_counter() - t0
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = {"workload": f"config/h36m_351_pt.json train step (fwd + bwd + AdamW), batch {batch}, DropPath {cfg.DROP_PATH_RATE}",
           "value": round(batch * steps / dt, 1), "unit": "pose-sequences/s", "ms_per_step": round(1e3 * dt / steps, 3), "steps": steps,
           "host_enqueue_ms_per_step": round(1e3 * enqueue / steps, 3), "loss": float(loss[0].item())}
    # algorithmic FLOPs of a step = 3 x the forward's (forward + activation-gradient + weight-gradient products), against the f16 MFMA
    # peak the f16x3 GEMMs of the step run on (its attention and small layers run exact f32: the fraction is an upper-level figure)
    fl = 3.0 * pkg.flops_per_sequence(arch)["total"] * batch
    out["achieved_tflops"] = round(fl / (dt / steps) / 1e12, 2)
    out["frac"] = round(fl / (dt / steps) / 1e12 / PEAK_F16_MFMA_TFLOPS, 4)
    del tr, model
    torch.cuda.empty_cache()
    return out


def _with_env(key, value, fn):
    old = os.environ.get(key)
    os.environ[key] = value
    try:
        return fn()
    finally:
        if old is None:
            del os.environ[key]
        else:
            os.environ[key] = old


def secondary_benchmarks(args):
    """The other claims of DESIGN.md in the same driver-run JSON line: ~20 steps each."""
    out = {}
    jobs = [("steady_state_200_steps", lambda: quick_forward_bench(args.config, args.batch, streams=max(1, args.streams_used), graph=True, steps=200, warmup=20)),
            # the reference's own evaluation batch (config BATCH_SIZE 512 windows per forward, eval.py:147-152): launches of 284 row tiles, where the
            # temporal chain (csrc/uu3d_tchain.h) is chosen by size -- against the same batch with the chain switched off
            ("eval_batch_512", lambda: quick_forward_bench(args.config, 512, streams=4, graph=True, steps=24, warmup=6)),      # (above 128 sequences per batch: one slot per hardware queue, pipeline.py)
            ("eval_batch_512_no_tchain", lambda: _with_env("UU3D_TCHAIN", "0", lambda: quick_forward_bench(args.config, 512, streams=4, graph=True, steps=24, warmup=6))),
            ("with_input_copy_per_step", lambda: quick_forward_bench(args.config, args.batch, streams=max(1, args.streams_used), graph=True, copy_inputs=True)),
            ("latency_one_batch_in_flight", lambda: quick_forward_bench(args.config, args.batch, streams=1, graph=True)),
            ("eager_one_batch_in_flight", lambda: quick_forward_bench(args.config, args.batch, streams=1, graph=False)),
            ("model_call_loop", lambda: quick_model_call_bench(args.config, args.batch)),
            ("eager_pipelined", lambda: quick_forward_bench(args.config, args.batch, streams=max(2, args.streams_used), graph=False)),
            ("h36m_81_batch256", lambda: quick_forward_bench("h36m_81", 256, streams=4)),
            ("s_in_10", lambda: quick_forward_bench(args.config, args.batch, s_in=10, streams=max(1, args.streams_used))),
            ("s_in_20", lambda: quick_forward_bench(args.config, args.batch, s_in=20, streams=max(1, args.streams_used))),
            ("dense_351_batch32", lambda: quick_forward_bench("dense_351", 32, streams=1, attention=True)),
            ("train_step", lambda: quick_train_bench())]
    for name, fn in jobs:
        try:
            out[name] = fn()
        except Exception as e:  # pragma: no cover
            out[name] = {"error": f"{type(e).__name__}: {e}"}
    return out


def pmc_summary_for(config, batch):
    """The committed --pmc summary that was collected on THIS workload (config, per-GPU batch), or None: counters of another
    shape say nothing about this one."""
    names = {("h36m_351", 128): ("r06_final_pmc_summary.csv", "r06_mid_pmc_summary.csv", "r05_final_pmc_summary.csv", "r04_final_pmc_summary.csv"), ("h36m_351", 512): ("r06_b512_pmc_summary.csv", "r05_tchain_b512_pmc_summary.csv"),
             ("dense_351", 32): ("r04_final_dense351_pmc_summary.csv",), ("h36m_81", 256): ("r04_final_h36m81_pmc_summary.csv",)}.get((config, batch), ())
    for name in names:                                           # (the newest round's counters of this workload first)
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", name)
        if os.path.exists(path):
            return path
    return None


# profile-record kernel name (csrc: Launcher::begin) -> substrings that pick the kernel SYMBOL out of a rocprofv3 summary
def symbol_filter(symbol):
    if symbol.startswith("gemm_panel8<") or symbol.startswith("gemm_panel<"):
        return ("gemm_h3_panel8_kernel" if symbol.startswith("gemm_panel8<") else "gemm_h3_panel_kernel",
                "PanelEp" + symbol[symbol.index("<") + 1:-1] + "E")
    return {"tchain": (TC_KERNEL,), "mlp_fused": ("mlp_fused_h3_kernel",), "gemm_wt": ("gemm_h3_wt_kernel",), "gemm_f32": ("gemm_f32_kernel",),
            "gemm_h3": ("gemm_h3",)}.get(symbol)


def pmc_traffic(symbol, summary=None, grid=None):
    """HBM-side bytes per launch of a kernel symbol from the committed rocprofv3 --pmc summary of THIS workload (FETCH_SIZE x2 on
    gfx950 + WRITE_SIZE, separate --pmc passes, tools/profile_r04.sh -> tools/rocpd_summary.py; one launch = the whole batch, like
    `achieved`).  None when no summary of this workload is committed or it does not hold that symbol."""
    import csv
    want = symbol_filter(symbol)
    if want is None or summary is None or not os.path.exists(summary):
        return None
    best = None
    for r in csv.DictReader(open(summary)):
        k = r["kernel"]
        if all(w in k for w in want) and r["HBM_read_bytes_avg_x2_gfx950_corrected"] and r["HBM_write_bytes_avg"]:
            t = float(r["HBM_read_bytes_avg_x2_gfx950_corrected"]) + float(r["HBM_write_bytes_avg"])
            if grid is not None and int(r["grid_size"]) != grid:    # (the counter run also holds the `under_load` forward's launches: another grid)
                continue
            key = (int(r["grid_size"]), int(r["launches"]))         # the temporal-block launches: largest grid, then most launches
            if best is None or key > best[0]:
                best = (key, t)
    return None if best is None else round(best[1])


def attention_roofline(agg, n_tokens, label):
    """The temporal-attention kernel (QK^T + PV of all heads) against the MFMA peak of the arithmetic it runs in: the
    north_star's "fraction of the attention roofline".  FLOPs = 4 L^2 d_h per (sequence, head), algorithmic (the f16x3
    kernel issues 3 MFMA passes per product and pads the 48-wide head to 64 rows in P V)."""
    a = agg.get("t.attn")
    if not a or a["ms"] <= 0:
        return None
    h3 = a["kernel"] == "attn_h3"
    peak = PEAK_F16_MFMA_TFLOPS if h3 else PEAK_F32_MFMA_TFLOPS
    ach = a["flops"] / (a["ms"] * 1e-3) / 1e12
    return {"kernel": f"{a['kernel']} [t.attn]", "workload": f"{label}: {n_tokens} tokens", "achieved": round(ach, 2), "peak": peak,
            "unit": "TFLOP/s", "frac": round(ach / peak, 4), "avg_launch_ms": round(a["ms"] / a["n"], 5),
            "arithmetic": "f16x3 (3 f16 MFMA passes, f32 accumulate; frac of pipe = 3 x frac)" if h3 else "exact f32 MFMA"}


def kernel_blocks(args, pkg, arch, agg, reps, prof_schedule, under_load, B, N, seqs, world, elapsed):
    """--full: the `roofline`, `kernel_ms_per_forward`, `kernel_ms_schedule` and `sum_kernel_ms` blocks of the bench line, from the
    per-kernel HIP-event records `agg` of `reps` quiet forwards and the timed region (`seqs` sequences in `elapsed` seconds)."""
    fl = pkg.flops_per_sequence(arch)
    total_ms = sum(a["ms"] for a in agg.values()) / reps
    # GEMM kernels by SYMBOL (the profile records carry the distinguishing part of the symbol: "gemm_panel8<BiasSplitQ>", "mlp_fused", ...):
    # the dominant kernel is the symbol with the most time per forward, whatever labels its launches carry
    is_gemm = (lambda k: k.startswith(("gemm_h3", "gemm_panel", "mlp_fused", "gemm_wt", "tchain"))) if args.precision == "f16x3" else (lambda k: k.startswith("gemm_f32"))
    peak = PEAK_F16_MFMA_TFLOPS if args.precision == "f16x3" else PEAK_F32_MFMA_TFLOPS
    by_sym = {}
    for k, a in agg.items():
        if is_gemm(a["kernel"]):
            bs = by_sym.setdefault(a["kernel"], dict(ms=0.0, flops=0.0, n=0, labels=[]))
            bs["ms"] += a["ms"]; bs["flops"] += a["flops"]; bs["n"] += a["n"]; bs["labels"].append(k)
    gk = max(by_sym, key=lambda k: by_sym[k]["ms"])
    dom = by_sym[gk]
    dom_key = "+".join(sorted(dom["labels"]))
    ach = dom["flops"] / (dom["ms"] * 1e-3) / 1e12
    gemm_fl = sum(bs["flops"] for bs in by_sym.values())
    gemm_ms = sum(bs["ms"] for bs in by_sym.values())
    return {
        "roofline": {"bound": "mfma", "bound_measured": BOUND_MEASURED if gk == "tchain" else None, "kernel": f"{gk} [{dom_key}]",
                     "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s",
                     "frac": round(ach / peak, 4), "traffic": pmc_traffic(gk, pmc_summary_for(args.config, B), grid=((B * N + TC_ROWS - 1) // TC_ROWS) * TC_THREADS if gk == "tchain" else None),
                     "note": ("algorithmic 2*M*N*K FLOPs (tchain: every Dense layer the launch walks -- projection, fc1, fc2, the next block's QKV; mlp_fused: both Dense layers of the MLP, 4*M*d*h); the f16x3 kernels issue 3 f16 "
                              "MFMA passes per product, so the matrix pipe does 3x this work (frac of pipe = 3 * frac)") if args.precision == "f16x3" else
                             "exact f32-input MFMA",
                     "traffic_note": "`traffic` is read from the committed counter run of this workload (profiles/, separate --pmc passes, launched eagerly under the same schedule) -- not measured in this process, which runs several hipGraphs in flight",
                     "avg_launch_ms": round(dom["ms"] / dom["n"], 5),
                     **({"workgroups_per_launch": (B * N + TC_ROWS - 1) // TC_ROWS, "cus": 256,
                         "frac_of_occupied_cus": round(ach / (peak * min(256, (B * N + TC_ROWS - 1) // TC_ROWS) / 256.0), 4),
                         "occupancy_note": f"the temporal chain runs ONE workgroup per {TC_ROWS} token rows and CU (64 rows: eight waves on 16-token panels, 157 KiB of LDS): a launch of this batch occupies "
                                           "that many of the 256 CUs, `achieved` / `frac` are the launch measured ALONE against the whole chip's peak (`under_load`: the same launch with "
                                           "every CU busy); the timed path runs several forwards' launches side by side"}
                        if gk == "tchain" else {}),
                     "attention": attention_roofline(agg, N, "synthetic dense-351 (NOT a shipped config)" if args.config == "dense_351" else f"config/{args.config}.json"),
                     # the four largest GEMM launch classes (the first two are within a microsecond per launch of each
                     # other, so which one is "dominant" changes from box to box)
                     "gemm_symbols": [{"kernel": f"{k} [{'+'.join(sorted(bs['labels']))}]", "ms_per_forward": round(bs["ms"] / reps, 4),
                                       "launches_per_forward": bs["n"] // reps,
                                       "achieved": round(bs["flops"] / (bs["ms"] * 1e-3) / 1e12, 2),
                                       "frac": round(bs["flops"] / (bs["ms"] * 1e-3) / 1e12 / peak, 4)}
                                      for k, bs in sorted(by_sym.items(), key=lambda kv: -kv[1]["ms"])[:4]],
                     "all_gemm_tflops": round(gemm_fl / (gemm_ms * 1e-3) / 1e12, 2),
                     "under_load": under_load,
                     "model_tflops": round(fl["total"] * seqs / world / elapsed / 1e12, 2),
                     "model_frac": round(fl["total"] * seqs / world / elapsed / 1e12 / peak, 4),
                     "model_frac_note": "whole-forward algorithmic FLOPs per second of the TIMED region (driver-clocked) over the dense peak of the arithmetic: the one figure of this block that no solo launch flatters"},
        "kernel_ms_per_forward": {k: round(a["ms"] / reps, 4) for k, a in sorted(agg.items(), key=lambda kv: -kv[1]["ms"])},
        "kernel_ms_schedule": prof_schedule + " (one quiet forward per sample, HIP events around every launch: the launches the timed path ran)",
        "sum_kernel_ms": round(total_ms, 4),
    }


def spawn_ranks(n, argv):
    """One process per GPU under torch.distributed.run on 127.0.0.1 (the container hostname may not resolve)."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=128, help="sequences per GPU per step")
    ap.add_argument("--config", default="h36m_351")
    ap.add_argument("--mask-stride", type=int, default=None, help="s_in; default = first MASK_STRIDE")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline and the parity check against the oracle")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the short secondary workloads (other configs, eager, train step) appended to the JSON line at N = 1")
    ap.add_argument("--full", action="store_true", help="also measure and check what the headline does not need: per-kernel timing and roofline, the CPU baseline, parity against "
                    "the oracle, the secondary workloads and, with N > 1, the other gather mode (a plain run: set-up, warm-up, the timed steps, the result line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the timed path computed in its last step as DIR/<name>.npy "
                    "(float32 / float64, at most 64 MB in all; the inputs are seeded: the same arguments give the same inputs)")
    ap.add_argument("--no-graph", action="store_true", help="launch eagerly instead of replaying a hipGraph")
    ap.add_argument("--streams", type=int, default=0, help="independent batches in flight (pipeline.ForwardPipeline: one HIP stream, workspace and hipGraph each); 1 = one batch after the other; 0 (default) = two per HIP hardware queue (8; pipeline.distinct_queue_streams)")
    ap.add_argument("--precision", default="f16x3", choices=["f16x3", "f32"], help="GEMM arithmetic of the forward (both hold the 1e-4 parity bar)")
    ap.add_argument("--mode", default="infer", choices=["infer", "train"], help="train = fwd + bwd + grad all-reduce + AdamW (BASELINE config 5)")
    ap.add_argument("--halves", action="store_true", help="two concurrent half-batch chains on two streams instead of one chain of kernels per batch")
    ap.add_argument("--no-halves", action="store_true", help="(default since the row-panel GEMM; accepted for older scripts)")
    ap.add_argument("--force-dist", action="store_true", help="initialise the process group even at world size 1 (exercises the RCCL path)")
    ap.add_argument("--gather", default="end", choices=["end", "step"], help="N > 1: all-gather of the per-sequence error blocks -- end = one collective of every step's block behind the loop's last result (default), step = one per step on the caller's stream")
    ap.add_argument("--timing-experiment", action="store_true", help="tools/ only: accept a timing build of the library (UU3D_LIB=.../libuu3d_timing.so) and UU3D_SKIP; the line is labelled INVALID (launches skipped, results wrong)")
    ap.add_argument("--spawn-check", action="store_true", help="ranks print their rank / world size and exit (no GPU): checks the self-spawn path")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")
    switches = env_switches(args.timing_experiment)        # (raises under UU3D_SKIP / UU3D_TIMING_PARTS)

    # `python bench.py --gpus N` without a launcher: start N ranks as CHILD processes here, before this process has
    # touched the GPU (no exec from a GPU-initialised process), and return their exit code.
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(spawn_ranks(args.gpus, sys.argv[1:]))
    if args.spawn_check:
        print(f"rank {os.environ.get('RANK', '0')}/{os.environ.get('WORLD_SIZE', '1')} local {os.environ.get('LOCAL_RANK', '0')}", flush=True)
        return

    import numpy as np
    import torch
    import torch.distributed as dist
    import uplift_upsample_3dhpe_amd as pkg
    from uplift_upsample_3dhpe_amd import synthetic as util

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    torch.cuda.set_device(local_rank)
    use_dist = world > 1 or args.force_dist
    if use_dist:
        if "MASTER_ADDR" not in os.environ:
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", RANK="0", WORLD_SIZE="1")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    rccl = None
    if use_dist:
        # evidence that the collective spans the ranks the line claims: every rank contributes (rank, local device index) to one all-gather
        ids = torch.tensor([rank, local_rank], dtype=torch.int64, device="cuda")
        seen = torch.empty((world, 2), dtype=torch.int64, device="cuda")
        dist.all_gather_into_tensor(seen, ids)
        seen = seen.cpu().tolist()
        rccl = {"backend": dist.get_backend(), "world_size": dist.get_world_size(), "ranks_seen": [int(r[0]) for r in seen],
                "devices_seen": [int(r[1]) for r in seen]}
        if sorted(rccl["ranks_seen"]) != list(range(world)):
            raise SystemExit(f"the all-gather of rank ids returned {rccl['ranks_seen']} for world size {world}")
    if args.mode == "train":
        return train_bench(args, world, rank, local_rank, use_dist)
    if "timing" in pkg.library_version() and not args.timing_experiment:
        raise SystemExit("bench.py refuses a timing build of the library (csrc/libuu3d_timing.so: launches can be skipped)")
    cfg = util.load_config(args.config)
    arch = pkg.arch_from_config(cfg)
    weights = pkg.init_weights(arch, seed=0)                 # replicated: same seed on every rank
    model = pkg.build_uplift_upsample_transformer(cfg, weights=weights, device=f"cuda:{local_rank}", precision=args.precision,
                                                   concurrent_halves=args.halves and not args.no_halves)
    s_in = args.mask_stride or (cfg.MASK_STRIDE[0] if isinstance(cfg.MASK_STRIDE, list) else cfg.MASK_STRIDE)
    B, N, J = args.batch, arch.num_frames, arch.num_keypoints
    x_np, m_np = util.synthetic_batch(cfg, B, seed=1000 + rank, mask_specs=[(s_in, 0)])
    x_np = x_np * m_np[:, :, None, None].astype(np.float32)
    rng = np.random.default_rng(2000 + rank)
    gt_np = np.concatenate([rng.normal(0, 0.3, size=(B, J, 3)), np.ones((B, J, 1))], -1).astype(np.float32)
    x = torch.from_numpy(x_np).cuda()
    m = torch.from_numpy(m_np).cuda()
    gt = torch.from_numpy(gt_np).cuda()
    err = torch.empty((B, J), dtype=torch.float64, device="cuda")
    gather = ErrorGather(args.gather, args.steps, B, J, world, "cuda", use_dist)
    from uplift_upsample_3dhpe_amd.harness import per_joint_error

    def sync_all():
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
            torch.cuda.synchronize()

    # A step = one batch through the forward + the per-joint error kernel (+ the all-gather of its (B, J) block with N > 1).
    # `--streams S` batches are in flight at once (pipeline.ForwardPipeline: each on its own HIP stream with its own workspace,
    # static buffers and hipGraph of forward + error kernel); S = 1 is one batch after the other.  The RCCL all-gather stays
    # outside the graphs, on the caller's stream.
    S = 1 if (args.halves and not args.no_halves) else max(0, args.streams)
    pipe = None
    auto = (S == 0)
    use_graph = not args.no_graph
    errs = {}                                           # one error block per slot (made by the slot's warm-up launch, before its capture)

    def post(full, central, i):
        if i not in errs:
            errs[i] = torch.empty((B, J), dtype=torch.float64, device="cuda")
        return per_joint_error(central, gt, cfg.ROOT_KEYTPOINT, out=errs[i])

    if args.halves and not args.no_halves:             # legacy option: two half-batch chains inside one call (no pipeline object)
        halves_out = {}

        def compute():
            full, central = model([x, m], training=False)
            per_joint_error(central, gt, cfg.ROOT_KEYTPOINT, out=err)
            halves_out["last"] = (full, central, err)   # (under a hipGraph: the graph's own output tensors, rewritten by every replay)
        run_compute = compute
        if use_graph:
            for _ in range(2):
                compute()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                compute()
            run_compute = g.replay

        def run_steps(n):
            gather.reset()
            for _ in range(n):
                run_compute()
                gather.step(err)
            gather.finish()
            return halves_out.get("last")
    else:
        try:
            if auto:                                    # two slots per HIP hardware queue (pipeline.distinct_queue_streams finds which streams share one)
                pipe = model.pipeline(B, depth=None, graph=use_graph, post=post)
                S = pipe.depth
            else:
                pipe = model.pipeline(B, depth=S, graph=use_graph, post=post)
        except Exception as e:  # pragma: no cover
            print(f"[bench] graph capture failed ({e}); running eagerly", file=sys.stderr)
            use_graph = False
            S = S or 2
            pipe = model.pipeline(B, depth=S, graph=False, post=post)

        # the synthetic batch is resident in every slot's static input buffers (the contract's "inputs already resident in HBM"):
        # a step is launch() = graph replay of forward + error kernel; a producer of real data writes into the buffers
        # pipe.acquire() hands out (eval.predict_windows), it does not copy either
        pipe.preload(x, m)

        def run_steps(n):
            return run_pipelined_steps(pipe, n, S, gather)

    run_steps(args.warmup)
    sync_all()
    t0 = time.perf_counter()
    last = run_steps(args.steps)
    sync_all()
    elapsed = time.perf_counter() - t0
    if use_dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    # ---- --dump-outputs: what the timed path handed its caller in the last timed step (read before anything launches again) ----
    if rank == 0 and args.dump_outputs:
        full_l, central_l, err_l = last
        arrays = {"full": full_l.cpu().numpy() if full_l is not None else None, "central": central_l.cpu().numpy(),
                  "per_joint_error": err_l.cpu().numpy()}
        if use_dist:                                     # N > 1: every rank's error block of that step, rank-major
            every = (gather.step_out.view(world, B, J) if gather.mode == "step" else
                     gather.gathered.view((world,) + tuple(gather.local.shape))[:, (gather.k - 1) % gather.local.shape[0]])
            arrays["per_joint_error_all_ranks"] = every.cpu().numpy()
        shapes = dump_outputs(args.dump_outputs, arrays)
        print(f"[bench] outputs of the last timed step in {args.dump_outputs}: {shapes}", file=sys.stderr, flush=True)

    # ---- N > 1: the same loop once more with the OTHER gather mode (one all-gather per step on the caller's stream, what rounds 1-4 timed), so that
    # scaling numbers stay comparable across rounds: reported beside the headline, never instead of it ----
    other_gather = None
    if args.full and use_dist and world > 1 and pipe is not None:
        other_mode = "step" if args.gather == "end" else "end"
        g2 = ErrorGather(other_mode, args.steps, B, J, world, "cuda", use_dist)
        run_pipelined_steps(pipe, args.warmup, S, g2)
        sync_all()
        t1 = time.perf_counter()
        run_pipelined_steps(pipe, args.steps, S, g2)
        sync_all()
        e2 = time.perf_counter() - t1
        t = torch.tensor([e2], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        e2 = float(t.item())
        other_gather = {"mode": other_mode, "value": round(world * B * args.steps / e2, 2), "unit": "pose-sequences/s", "ms_per_step": round(e2 / args.steps * 1e3, 4)}

    # ---- --full: what the timed path produced for the resident batch (parity block of the JSON line; outside the timed region) ----
    hip_full = hip_central = None
    if args.full and pipe is not None and rank == 0:
        f_, c_, _ = pipe.result(pipe.launch())
        torch.cuda.synchronize()
        hip_full, hip_central = (f_.cpu().numpy() if f_ is not None else None), c_.cpu().numpy()

    # ---- --full: per-kernel timing with HIP events on the launch stream (outside the timed region) ----
    agg, reps, under_load = {}, 5, None
    prof_schedule = "throughput" if (pipe is not None and S > 1) else "latency"       # the launches the timed path ran
    if args.full:
        model.set_profiling(True)
        for _ in range(reps):
            model.call_scheduled([x, m], prof_schedule)
            for e in model.read_profile():
                # temporal blocks share one shape class ("t.<op>"); strided blocks keep their index
                nm = e["name"]
                key = ("t." + nm.split(".", 1)[1]) if (nm[0] == "t" and "." in nm) else nm
                a = agg.setdefault(key, dict(ms=0.0, flops=0.0, bytes=0.0, n=0, kernel=e["kernel"]))
                a["ms"] += e["ms"]; a["flops"] += e["flops"]; a["bytes"] += e["bytes"]; a["n"] += 1
        # ---- the temporal chain's launch when it FILLS the chip (what the timed path runs: several forwards' 71-workgroup launches side by side):
        # one quiet forward of the batch that makes 256 row tiles, HIP events around its launches ----
        if rank == 0 and prof_schedule == "throughput" and any(a["kernel"] == "tchain" for a in agg.values()):
            try:
                b_full = (256 * 128) // N
                reps_x = (b_full + B - 1) // B
                xl, ml = x.repeat((reps_x, 1, 1, 1))[:b_full].contiguous(), m.repeat((reps_x, 1))[:b_full].contiguous()
                ms, fls, n = 0.0, 0.0, 0
                for it in range(4):
                    model.call_scheduled([xl, ml], "throughput")
                    for e in model.read_profile():
                        if it > 0 and e["kernel"] == "tchain" and e["name"][0] == "t" and e["name"].endswith(".chain"):
                            ms += e["ms"]; fls += e["flops"]; n += 1
                if n:
                    under_load = {"workgroups": (b_full * N + TC_ROWS - 1) // TC_ROWS, "rows": b_full * N, "batch": b_full, "avg_launch_ms": round(ms / n, 5),
                                  "achieved": round(fls / (ms * 1e-3) / 1e12, 2), "unit": "TFLOP/s",
                                  "frac": round(fls / (ms * 1e-3) / 1e12 / PEAK_F16_MFMA_TFLOPS, 4),
                                  "note": "one temporal-block launch of the chain (projection .. next block's QKV) over 256 x 128 token rows = every CU busy for the whole launch: HIP events around the "
                                          f"launches of a quiet forward of {b_full} sequences, same kernel and schedule as the timed path"}
                del xl, ml
            except Exception as e:  # pragma: no cover
                under_load = {"error": f"{type(e).__name__}: {e}"}
        model.set_profiling(False)

    if use_dist:                                         # every rank's buffered C stdio (RCCL's banner) out BEFORE rank 0's line
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:  # pragma: no cover
            pass
        dist.barrier()
    if rank == 0:
        seqs = world * B * args.steps
        out = {
            "metric": "pose-sequences/sec",
            "value": round(seqs / elapsed, 2),
            "unit": "pose-sequences/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f16x3 (f32 operands split into f16 hi/lo, 3 MFMA passes, f32 accumulate)" if args.precision == "f16x3" else "f32",
            "data": "synthetic",
            "config": {"workload": ("synthetic dense-351 (SURVEY 8(d) stress shape, not a shipped config: h36m_351 with SEQUENCE_LENGTH 351, stride 1, STRIDES [3,9,13])"
                                    if args.config == "dense_351" else f"config/{args.config}.json") + f" forward, N={N} tokens (receptive field "
                                   f"{(N - 1) * cfg.SEQUENCE_STRIDE + 1}), J={J}, batch {B}/GPU, s_in={s_in}, "
                                   f"seeded Keras-default weights", "global_batch": world * B,
                       "parallelism": f"batch-sharded x{world}", "hipgraph": bool(use_graph),
                       "concurrent_half_batches": bool(args.halves and not args.no_halves and B >= 64),
                       "batches_in_flight": S, "env_switches": switches,
                       "pipelining": (f"{S} independent batches in flight on {S} HIP streams" + (" dealt evenly over the HIP hardware queues (probed)" if auto else "") +
                                      ", each replaying its own hipGraph of forward + error "
                                      "kernel with its own workspace (uplift-upsample-3dhpe_amd/pipeline.py; the same path eval.run_eval uses)") if S > 1
                                     else "one batch after the other"},
        }
        if args.full:
            out.update(kernel_blocks(args, pkg, arch, agg, reps, prof_schedule, under_load, B, N, seqs, world, elapsed))
        if args.full and not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(cfg, arch, weights, x_np, m_np)
        else:
            out["cpu_baseline"] = None
        if args.full and not args.no_cpu_baseline and hip_central is not None:
            try:
                out["parity"] = parity_vs_oracle(cfg, arch, weights, x_np, m_np, hip_full, hip_central, gt_np)
            except Exception as e:  # pragma: no cover
                out["parity"] = {"error": f"{type(e).__name__}: {e}"}
        else:
            out["parity"] = None
        out["rccl"] = rccl
        if args.timing_experiment:
            out["metric"] = "TIMING EXPERIMENT, NOT A RESULT (launches may be skipped)"
            out["INVALID_timing_experiment"] = True
        if world > 1:
            out["config"]["gather"] = ("one all-gather of every step's (B_local, J) f64 error block behind the loop's last result, inside the timed region" if args.gather == "end"
                                       else "one all-gather per step on the caller's stream")
            out["other_gather_mode"] = other_gather           # (the same loop with the other mode: rounds 1-4 timed "step")
        if args.full and world == 1 and not args.no_secondary and args.config == "h36m_351":
            pipe = None
            args.streams_used = S
            out["secondary"] = secondary_benchmarks(args)
        emit_line(out)
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
