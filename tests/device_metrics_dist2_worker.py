"""One rank of tests/test_device_metrics_gpu.py::test_two_ranks_on_one_gpu: two of these processes share cuda:0 and talk over gloo (as
tests/dist2_worker.py).  run_eval(device_metrics=True): the windows are split over the ranks at a batch boundary (so that every batch is
composed as in a one-rank run and the predictions are the same bits), the predictions all-gathered, each rank evaluates its shard of the
poses on the device and the sums tables are added in rank order.

Then evaluation_device.report_sums with a pass that has no plan ("pose i is row i": what train.Validation hands it), and run_train over the
two ranks with the validation metrics on the host and on the device.

    python tests/device_metrics_dist2_worker.py <rank> <world> <port> <outdir> <config> <h36m 3d> <h36m 2d>
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import uplift_upsample_3dhpe_amd as pkg                                    # noqa: E402
from uplift_upsample_3dhpe_amd import dist as udist                        # noqa: E402
from uplift_upsample_3dhpe_amd import eval as ev                           # noqa: E402
from uplift_upsample_3dhpe_amd import synthetic as util                    # noqa: E402

G = os.path.join(ROOT, "tests", "golden")
BATCH = 4


def _setup():
    cfg = util.load_config("h36m_351")
    cfg.BATCH_SIZE = BATCH
    cfg.MASK_STRIDE = cfg.MASK_STRIDE[0] if isinstance(cfg.MASK_STRIDE, list) else cfg.MASK_STRIDE
    arch = pkg.arch_from_config(cfg)
    model = pkg.build_uplift_upsample_transformer(cfg, weights=pkg.init_weights(arch, seed=2, perturb=0.1))
    return cfg, model, (cfg, "h36m", os.path.join(G, "h36m_tiny_3d.npz"), os.path.join(G, "h36m_tiny_2d.npz"), "S9")


def _plain(rep):
    return {"all_frames": rep["all_frames"], "keyframes": rep["keyframes"]}


def reports():
    """The one-rank reports, host and device."""
    cfg, model, args = _setup()
    host = ev.run_eval(*args, model=model, action_wise=True, log=lambda *a: None)
    dev = ev.run_eval(*args, model=model, action_wise=True, log=lambda *a: None, device_metrics=True)
    return {"host": _plain(host), "device": _plain(dev), "num_forwarded": host["num_forwarded"]}


def plain_pass_inputs():
    """Seeded poses for the plan-less pass of report_sums: 1003 poses, every one different, 15 actions."""
    import numpy as np
    rng = np.random.default_rng(11)
    gt = rng.normal(0, 0.35, size=(1003, 17, 3))
    pred = gt * rng.uniform(0.8, 1.25, size=(1003, 1, 1)) + rng.normal(0, 0.04, size=gt.shape)
    return pred.astype(np.float32), gt.astype(np.float32), (np.arange(1003) % 15).astype(np.int32)


def main():
    import torch
    import torch.distributed as dist
    from uplift_upsample_3dhpe_amd import evaluation_device as ED
    from uplift_upsample_3dhpe_amd.train import run_train
    rank, world, port, outdir = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    cfg, model, args = _setup()
    shards = []

    def uneven(n, r, w):
        # rank 0 takes one batch more than half, cut at a batch boundary
        cut = min(n, (n // 2 // BATCH + 1) * BATCH)
        lo, hi = (0, cut) if r == 0 else (cut, n)
        shards.append(hi - lo)
        return lo, hi
    even_split = udist.shard_bounds
    udist.shard_bounds = uneven
    try:
        rep = ev.run_eval(*args, model=model, action_wise=True, log=lambda *a: None, device_metrics=True)
    finally:
        udist.shard_bounds = even_split
    out = {"rank": rank, "shards": shards, "device": _plain(rep), "num_forwarded": rep["num_forwarded"]}
    pred, gt, actions = plain_pass_inputs()
    out["plain_sums"] = ED.report_sums(torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), 6, [{}], num_actions=15, actions=actions).tolist()
    cfg_path, p3, p2 = sys.argv[5:8]
    for mode in ("host", "device"):
        res = run_train(cfg_path, h36m_path=p3, dataset_2d_path=p2, train_subset="S8", val_subset="S9", log=lambda *a: None,
                        out_dir=os.path.join(outdir, f"{mode}_rank{rank}"), device_metrics=mode == "device")
        out["history_" + mode] = res["history"]
    with open(os.path.join(outdir, f"rank{rank}.json"), "w") as f:
        json.dump(out, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
