"""One rank of tests/test_autograd_dist2_gpu.py: custom-loss training (loss.backward() + Trainer.apply_gradients()) with two ranks
sharing cuda:0 over gloo, as in tests/dist2_worker.py.  Each check runs the accumulating, range-reporting backward pass of the
trainer and a reference: the same trainer code held at world size 1 (the one-rank autograd path), one flat dist.all_reduce of its
gradient, and the same optimizer step.

    python tests/autograd_dist2_worker.py <rank> <world> <port> <outdir>
"""
import ctypes as C
import datetime
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import uplift_upsample_3dhpe_amd as pkg                                    # noqa: E402
from uplift_upsample_3dhpe_amd import dist as udist                        # noqa: E402
from uplift_upsample_3dhpe_amd import synthetic as util                    # noqa: E402
from uplift_upsample_3dhpe_amd.trainer import Trainer                      # noqa: E402


def mpjpe(full, central, gt, cfg):
    """The reference's loss written in torch (root-relative MPJPE of the sequence and of the central frame), normalised by the
    GLOBAL batch: the sum over ranks of the rank gradients is then the gradient of the whole batch."""
    r = int(cfg.ROOT_KEYTPOINT)
    B, N, J = full.shape[0], full.shape[1], full.shape[2]
    rel = lambda p: p - p[..., r:r + 1, :]                                    # noqa: E731
    seq = torch.linalg.vector_norm(rel(full) - rel(gt), dim=-1).sum() / (cfg.BATCH_SIZE * N * J)
    cen = torch.linalg.vector_norm(rel(central) - rel(gt[:, N // 2]), dim=-1).sum() / (cfg.BATCH_SIZE * J)
    return cfg.LOSS_WEIGHT_SEQUENCE * seq + cfg.LOSS_WEIGHT_CENTER * cen


def crc(t):
    return int(np.bitwise_xor.reduce(np.frombuffer(t.detach().cpu().numpy().tobytes(), dtype=np.uint32)))


def same_on_all_ranks(t):
    parts = [torch.zeros(1, dtype=torch.int64) for _ in range(dist.get_world_size())]
    dist.all_gather(parts, torch.tensor([crc(t)], dtype=torch.int64))
    return all(int(p) == int(parts[0]) for p in parts)


class CountAllReduce(object):
    """Counts dist.all_reduce calls (the trainer and dist.BucketedAllReduce look the function up at call time)."""

    def __init__(self):
        self.n, self._orig = 0, dist.all_reduce

    def __enter__(self):
        def counted(*a, **k):
            self.n += 1
            return self._orig(*a, **k)
        dist.all_reduce = counted
        return self

    def __exit__(self, *exc):
        dist.all_reduce = self._orig


def main():
    rank, world, port, outdir = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=300))              # a rank that failed does not keep the other waiting
    out = {"rank": rank}

    cfg = util.load_config("h36m_351")
    Bl = 3                                                                    # per rank and micro-batch
    cfg.BATCH_SIZE = 2 * Bl * world                                           # the global batch of a step of two micro-batches
    cfg.DROP_PATH_RATE = [0.0, 0.0, 0.0]
    arch = pkg.arch_from_config(cfg)
    w = pkg.init_weights(arch, seed=5, perturb=0.1)
    xg, mg = util.synthetic_batch(cfg, 2 * Bl * world, seed=6)
    xg = xg * mg[:, :, None, None].astype(np.float32)
    gtg = np.random.default_rng(7).normal(0, 0.3, size=(2 * Bl * world, arch.num_frames, 17, 3)).astype(np.float32)
    T_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()          # noqa: E731
    micro = []
    for k in range(2):                                                        # micro-batch k of this rank
        lo, hi = udist.shard_bounds(Bl * world, rank, world)
        lo, hi = lo + k * Bl * world, hi + k * Bl * world
        micro.append((T_(xg[lo:hi]), T_(mg[lo:hi]), T_(gtg[lo:hi])))

    def trainer(reference=False):
        model = pkg.build_uplift_upsample_transformer(cfg, weights=w)
        tr = Trainer(model, cfg, seed=1)
        model.requires_grad_()
        if reference:
            tr._world = lambda: 1                                             # the one-rank autograd path (and apply_gradients)
        return model, tr

    def backward(model, tr, k, inf=False):
        x, m, gt = micro[k]
        full, central = model([x, m], training=True)
        loss = mpjpe(full, central, gt, cfg)
        if inf:                                                               # an Inf in this rank's cotangent of `full`
            loss = loss + full[0, 0, 0, 0] * float("inf")
        loss.backward()

    def reference_step(ks):
        model, tr = trainer(reference=True)
        tr.zero_grad()
        for k in ks:
            backward(model, tr, k)
        dist.all_reduce(tr.grads)                                             # one flat sum of the rank gradients
        g = tr.grads.clone()
        tr.apply_gradients()
        torch.cuda.synchronize()
        return g, tr.params.detach().clone()

    # ---- (a) one reporting backward pass: buckets started from the library's stream, == one flat all-reduce, bit for bit ----
    model, tr = trainer()
    seen = []
    orig = tr._buckets.ready
    tr._buckets.ready = lambda first, count, stream=None: (seen.append((int(first), int(count), stream)), orig(first, count, stream))[1]
    p0 = tr.params.detach().clone()
    tr.zero_grad()
    backward(model, tr, 0)
    assert tr.params.grad is tr.grads
    grads_a = tr.grads.clone()
    tr.apply_gradients()
    torch.cuda.synchronize()
    ref_g, ref_p = reference_step([0])
    out["a_buckets"] = len(seen)
    out["a_buckets_from_library_stream"] = all(s is not None for _, _, s in seen)
    out["a_grads_equal_flat"] = bool(torch.equal(grads_a, ref_g))
    out["a_params_equal_reference"] = bool(torch.equal(tr.params, ref_p))
    out["a_params_moved"] = bool(not torch.equal(tr.params, p0))
    out["a_not_skipped"] = not tr.nonfinite()
    out["a_replicas_identical"] = same_on_all_ranks(tr.params)
    out["a_crc"] = crc(tr.params)

    # ---- (b) two micro-batches, the first inside no_sync(): == both micro-batches' summed gradients reduced once ----
    model, tr = trainer()
    tr.zero_grad()
    with CountAllReduce() as c1:
        with tr.no_sync():
            backward(model, tr, 0)
    with CountAllReduce() as c2:
        backward(model, tr, 1)
    grads_b = tr.grads.clone()
    tr.apply_gradients()
    torch.cuda.synchronize()
    ref_g, ref_p = reference_step([0, 1])
    out["b_no_sync_collectives"] = c1.n
    out["b_reporting_collectives"] = c2.n
    out["b_grads_equal_flat"] = bool(torch.equal(grads_b, ref_g))
    out["b_params_equal_reference"] = bool(torch.equal(tr.params, ref_p))
    out["b_replicas_identical"] = same_on_all_ranks(tr.params)
    params_b = tr.params.detach().clone()

    # ---- (c) an Inf in ONE rank's cotangent: every rank skips, the replicas stay identical; a finite step afterwards applies ----
    model, tr = trainer()
    before = tr.params.detach().clone()
    tr.zero_grad()
    backward(model, tr, 0, inf=(rank == 1))
    tr.apply_gradients()
    torch.cuda.synchronize()
    out["c_skipped"] = bool(tr.nonfinite())
    out["c_params_unchanged"] = bool(torch.equal(tr.params, before))
    tr.zero_grad()
    backward(model, tr, 0)
    tr.apply_gradients()
    torch.cuda.synchronize()
    out["c_finite_step_applied"] = bool((not tr.nonfinite()) and not torch.equal(tr.params, before))
    out["c_replicas_identical"] = same_on_all_ranks(tr.params)

    # ---- (c2) ONE rank's non-finite word raised while every gradient stays finite: only the MAX over the ranks' words can make
    # the other rank skip.  Rank 1 raises its word with a plain tape backward of an Inf cotangent into the tape's own buffer
    # (uu3d_train_backward_tape, grads NULL), which leaves trainer.grads alone ----
    model, tr = trainer()
    before = tr.params.detach().clone()
    tr.zero_grad()
    backward(model, tr, 0)
    if rank == 1:
        x, m, _ = micro[1]
        with torch.no_grad():
            full, _, tape = model._tape_forward(x, model._mask_u8(m))
        gF = torch.zeros_like(full)
        gF[0, 0, 0, 0] = float("inf")
        st = model._lib.uu3d_train_backward_tape(model._h, tape.handle, C.c_void_p(gF.data_ptr()), None, None, None,
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == 0
        torch.cuda.synchronize()
        del tape
    out["c2_grads_finite"] = bool(torch.isfinite(tr.grads).all())
    tr.apply_gradients()
    torch.cuda.synchronize()
    out["c2_skipped"] = bool(tr.nonfinite())
    out["c2_params_unchanged"] = bool(torch.equal(tr.params, before))
    out["c2_replicas_identical"] = same_on_all_ranks(tr.params)

    # ---- (d) after the reporting pass, another backward pass in the same step -- reporting or inside no_sync() -- raises before it
    # enqueues anything: no collective, grads untouched ----
    model, tr = trainer()
    tr.zero_grad()
    backward(model, tr, 0)
    torch.cuda.synchronize()
    held = tr.grads.clone()
    x, m, gt = micro[1]
    raised = []
    with CountAllReduce() as c3:
        for local in (False, True):
            full, central = model([x, m], training=True)
            loss = mpjpe(full, central, gt, cfg)
            try:
                if local:
                    with tr.no_sync():
                        loss.backward()
                else:
                    loss.backward()
                raised.append(False)
            except RuntimeError as e:
                raised.append("after the reporting one" in str(e))
    torch.cuda.synchronize()
    out["d_raised"] = raised == [True, True]
    out["d_collectives"] = c3.n
    out["d_grads_untouched"] = bool(torch.equal(tr.grads, held))
    tr.zero_grad()                                                            # the next step starts clean
    backward(model, tr, 0)
    tr.apply_gradients()
    torch.cuda.synchronize()
    out["d_next_step_equal_a"] = crc(tr.params) == out["a_crc"]

    # ---- (e) every pass inside no_sync(): apply_gradients all-reduces the whole buffer once; == (b) ----
    model, tr = trainer()
    tr.zero_grad()
    with CountAllReduce() as c4:
        with tr.no_sync():
            backward(model, tr, 0)
            backward(model, tr, 1)
    with CountAllReduce() as c5:
        tr.apply_gradients()
    torch.cuda.synchronize()
    out["e_backward_collectives"] = c4.n
    out["e_apply_collectives"] = c5.n                                         # the flat gradient sum and the MAX of the non-finite words
    out["e_params_equal_b"] = bool(torch.equal(tr.params, params_b))
    out["e_replicas_identical"] = same_on_all_ranks(tr.params)

    # ---- (f) as (e), with .grad replaced after the passes (an average over the micro-batches): the replaced tensor is what is
    # summed over the ranks; == the one-rank path with the same replacement, then one flat all-reduce ----
    model, tr = trainer()
    tr.zero_grad()
    with tr.no_sync():
        backward(model, tr, 0)
        backward(model, tr, 1)
    tr.params.grad = tr.params.grad / 2
    tr.apply_gradients()
    torch.cuda.synchronize()
    model_r, tr_r = trainer(reference=True)
    tr_r.zero_grad()
    backward(model_r, tr_r, 0)
    backward(model_r, tr_r, 1)
    g = tr_r.params.grad / 2
    dist.all_reduce(g)
    tr_r.params.grad = g
    tr_r.apply_gradients()
    torch.cuda.synchronize()
    out["f_params_equal_reference"] = bool(torch.equal(tr.params, tr_r.params))
    out["f_replicas_identical"] = same_on_all_ranks(tr.params)

    with open(os.path.join(outdir, f"rank{rank}.json"), "w") as f:
        json.dump(out, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
