"""One rank of tests/test_structural_training_gpu.py::test_no_temporal_blocks_on_two_ranks: custom-loss training of a model without
temporal blocks (no full-sequence output; loss (LOSS_WEIGHT_CENTER + LOSS_WEIGHT_SEQUENCE) * central, train.py:491-494) with two
ranks sharing cuda:0 over gloo, as in tests/autograd_dist2_worker.py.  The accumulating, range-reporting backward pass of the trainer
plus its step against the same trainer code held at world size 1, one flat dist.all_reduce of its gradient and the same step.

    python tests/structural_dist2_worker.py <rank> <world> <port> <outdir>
"""
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


def central_loss(central, gt, cfg):
    """The reference's fallback loss written in torch, normalised by the GLOBAL batch."""
    r = int(cfg.ROOT_KEYTPOINT)
    N, J = gt.shape[1], gt.shape[2]
    g = gt[:, N // 2] - gt[:, N // 2, r:r + 1, :]
    cen = torch.linalg.vector_norm(central - g, dim=-1).sum() / (cfg.BATCH_SIZE * J)
    return (cfg.LOSS_WEIGHT_CENTER + cfg.LOSS_WEIGHT_SEQUENCE) * cen


def crc(t):
    return int(np.bitwise_xor.reduce(np.frombuffer(t.detach().cpu().numpy().tobytes(), dtype=np.uint32)))


def main():
    rank, world, port, outdir = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=300))              # a rank that failed does not keep the other waiting
    out = {"rank": rank}

    cfg = util.load_config("h36m_81")
    cfg.TEMPORAL_TRANSFORMER_BLOCKS = 0
    Bl = 3                                                                    # per rank
    cfg.BATCH_SIZE = Bl * world
    cfg.DROP_PATH_RATE = [0.0, 0.0, 0.0]
    arch = pkg.arch_from_config(cfg)
    assert arch.temporal_depth == 0 and arch.has_strided_input
    w = pkg.init_weights(arch, seed=5, perturb=0.1)
    xg, mg = util.synthetic_batch(cfg, Bl * world, seed=6)
    xg = xg * mg[:, :, None, None].astype(np.float32)
    gtg = np.random.default_rng(7).normal(0, 0.3, size=(Bl * world, arch.num_frames, 17, 3)).astype(np.float32)
    T_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()          # noqa: E731
    lo, hi = udist.shard_bounds(Bl * world, rank, world)
    x, m, gt = T_(xg[lo:hi]), T_(mg[lo:hi]), T_(gtg[lo:hi])

    def trainer(reference=False):
        model = pkg.build_uplift_upsample_transformer(cfg, weights=w)
        tr = Trainer(model, cfg, seed=1)
        model.requires_grad_()
        if reference:
            tr._world = lambda: 1                                             # the one-rank autograd path (and apply_gradients)
        return model, tr

    def backward(model):
        full, central = model([x, m], training=True)
        central_loss(central, gt, cfg).backward()
        return full

    # the reporting backward pass: its buckets tile the gradient buffer, and it equals one flat all-reduce, bit for bit
    model, tr = trainer()
    seen = []
    orig = tr._buckets.ready
    tr._buckets.ready = lambda first, count, stream=None: (seen.append((int(first), int(count))), orig(first, count, stream))[1]
    p0 = tr.params.detach().clone()
    tr.zero_grad()
    out["full_is_none"] = backward(model) is None
    grads = tr.grads.clone()
    tr.apply_gradients()
    torch.cuda.synchronize()

    model_r, tr_r = trainer(reference=True)
    tr_r.zero_grad()
    backward(model_r)
    dist.all_reduce(tr_r.grads)                                               # one flat sum of the rank gradients
    ref_g = tr_r.grads.clone()
    tr_r.apply_gradients()
    torch.cuda.synchronize()

    spans = sorted(seen)
    out["buckets"] = len(seen)
    out["ranges_tile_the_buffer"] = (spans[0][0] == 0 and sum(c for _, c in spans) == tr.n_params
                                     and all(a + c == b for (a, c), (b, _) in zip(spans, spans[1:])))
    out["grads_equal_flat"] = bool(torch.equal(grads, ref_g))
    out["params_equal_reference"] = bool(torch.equal(tr.params, tr_r.params))
    out["params_moved"] = bool(not torch.equal(tr.params, p0))
    out["not_skipped"] = not tr.nonfinite()
    parts = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(parts, torch.tensor([crc(tr.params)], dtype=torch.int64))
    out["replicas_identical"] = all(int(p) == int(parts[0]) for p in parts)
    out["crc"] = crc(tr.params)
    with open(os.path.join(outdir, f"rank{rank}.json"), "w") as f:
        json.dump(out, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
