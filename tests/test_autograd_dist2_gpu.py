"""GPU: custom-loss training (a torch MPJPE, loss.backward(), Trainer.apply_gradients()) with two real ranks on one GPU over gloo
(tests/autograd_dist2_worker.py; the pattern and time limits of tests/test_dist2_gpu.py).  Checked on both ranks:

  (a) one reporting backward pass: its gradient buckets start from the library's stream while the pass runs; gradients and the
      parameters after the step equal, bit for bit, the one-rank autograd backward + one flat dist.all_reduce + the same step;
  (b) two micro-batches, the first inside no_sync() (no collective), equal one flat all-reduce of both micro-batches' gradients;
  (c) an Inf in ONE rank's cotangent: both ranks skip the step, the replicas stay identical;
  (c2) ONE rank's non-finite word raised with every gradient finite: both ranks skip (the MAX over the ranks' words);
  (d) after the reporting pass, another backward pass in the step, reporting or inside no_sync(), raises before it enqueues
      anything (no collective, gradients untouched);
  (e) every pass inside no_sync(): apply_gradients all-reduces the whole buffer once, and the step equals (b);
  (f) as (e) with .grad replaced after the passes: the replacement is what is summed, as on the one-rank path."""
import json
import os
import socket
import subprocess
import sys

import pytest

from tests import util

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def test_custom_loss_on_two_ranks(tmp_path):
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, PYTHONPATH=util.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    procs = [subprocess.Popen([sys.executable, os.path.join(util.ROOT, "tests", "autograd_dist2_worker.py"), str(r), "2", str(port),
                               str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=900)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o)
    assert all(p.returncode == 0 for p in procs), "\n".join(l[-3000:] for l in logs)
    res = [json.load(open(os.path.join(tmp_path, f"rank{r}.json"))) for r in range(2)]

    for r in res:
        # (a)
        assert r["a_buckets"] >= 4 and r["a_buckets_from_library_stream"], r
        assert r["a_grads_equal_flat"] and r["a_params_equal_reference"], r
        assert r["a_params_moved"] and r["a_not_skipped"] and r["a_replicas_identical"], r
        # (b)
        assert r["b_no_sync_collectives"] == 0 and r["b_reporting_collectives"] >= 4, r
        assert r["b_grads_equal_flat"] and r["b_params_equal_reference"] and r["b_replicas_identical"], r
        # (c)
        assert r["c_skipped"] and r["c_params_unchanged"], r
        assert r["c_finite_step_applied"] and r["c_replicas_identical"], r
        # (c2)
        assert r["c2_grads_finite"] and r["c2_skipped"] and r["c2_params_unchanged"] and r["c2_replicas_identical"], r
        # (d)
        assert r["d_raised"] and r["d_collectives"] == 0 and r["d_grads_untouched"], r
        assert r["d_next_step_equal_a"], r
        # (e)
        assert r["e_backward_collectives"] == 0 and r["e_apply_collectives"] == 2, r
        assert r["e_params_equal_b"] and r["e_replicas_identical"], r
        # (f)
        assert r["f_params_equal_reference"] and r["f_replicas_identical"], r
    assert res[0]["a_crc"] == res[1]["a_crc"]
