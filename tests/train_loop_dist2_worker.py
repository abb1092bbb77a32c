"""One rank of tests/test_train_loop_dist2_gpu.py: run_train over two ranks (gloo, both on cuda:0), each with its own out_dir so that
the test can see which rank wrote files.

    python tests/train_loop_dist2_worker.py <rank> <world> <port> <config> <h36m 3d> <h36m 2d> <outdir>
"""
import json
import os
import sys

import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uplift_upsample_3dhpe_amd.train import run_train      # noqa: E402


def main():
    rank, world, port = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
    cfg, p3, p2, outdir = sys.argv[4:8]
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    out = os.path.join(outdir, f"rank{rank}")
    res = run_train(cfg, h36m_path=p3, dataset_2d_path=p2, train_subset="S8", val_subset="S9", out_dir=out, log=lambda *a: None)
    with open(os.path.join(outdir, f"rank{rank}.json"), "w") as fh:
        json.dump({"history": res["history"], "best": res["best_weights"], "last": res["last_weights"]}, fh)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
