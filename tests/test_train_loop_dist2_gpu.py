"""GPU: run_train over two ranks on one GPU (gloo, in the pattern of tests/test_dist2_gpu.py).  Each rank trains on its contiguous
shard of every global batch and validates its shard of every val batch.  Without DropPath / Dropout (whose draws are per rank by
design) the final weights equal the one-rank run's up to the order of the gradient sums; both ranks report the same history; only
rank 0 writes files."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import util
from tests.test_train_loop_gpu import _config, _h36m_copy

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def test_two_ranks_train_like_one(tmp_path):
    from uplift_upsample_3dhpe_amd.train import run_train
    p3, p2 = _h36m_copy(tmp_path)
    cfg = _config(tmp_path, DROP_PATH_RATE=0.0, DROP_RATE=0.0, ATTENTION_DROP_RATE=0.0, BATCH_SIZE=12)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, PYTHONPATH=util.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(util.ROOT, "tests", "train_loop_dist2_worker.py"), str(r), "2", str(port),
                               cfg, p3, p2, str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o)
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-3000:] for l in logs)
    res = [json.load(open(str(tmp_path / f"rank{r}.json"))) for r in range(2)]
    np.testing.assert_equal(res[0]["history"], res[1]["history"])           # (NaN == NaN: tiny S9 lacks most actions)
    assert [os.path.basename(res[r][k]) for r in range(2) for k in ("best", "last")] == ["best_weights_0002.h5", "last_weights_0002.h5"] * 2 \
        or os.path.basename(res[0]["best"]) == os.path.basename(res[1]["best"])
    assert not os.path.exists(str(tmp_path / "rank1")) or not any(files for _, _, files in os.walk(str(tmp_path / "rank1")))
    one = run_train(cfg, h36m_path=p3, dataset_2d_path=p2, train_subset="S8", val_subset="S9", out_dir=str(tmp_path / "one"),
                    log=lambda *a: None)
    w2 = np.load(str(tmp_path / "rank0" / "checkpoints" / "cp_0002.npz"))
    w1 = np.load(str(tmp_path / "one" / "checkpoints" / "cp_0002.npz"))
    for k in ("params", "ema"):
        a, b = w2[k].astype(np.float64), w1[k].astype(np.float64)
        assert np.linalg.norm(a - b) <= 1e-5 * np.linalg.norm(b), k            # (norm-wise: Adam moves a weight whose gradient sum
                                                                                  # sits at zero by up to a whole step either way)
    for m, vals in one["history"].items():
        got = [v for _, v in res[0]["history"][m]]
        assert np.allclose(got, [v for _, v in vals], rtol=1e-3, equal_nan=True), m
    assert sorted(os.listdir(str(tmp_path / "rank0"))) == ["checkpoints", "history.jsonl", "tiny_complete.json"]
