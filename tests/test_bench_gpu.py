"""GPU: a plain `bench.py` run (set-up, warm-up, the timed steps, the line) and what `--dump-outputs` writes -- the last timed step's
outputs of the default workload (config/h36m_351.json, batch 128, seeded inputs), checked against the CPU oracle and against a
second run with other step counts (same arguments otherwise: the same inputs, so the same outputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import uplift_upsample_3dhpe_amd as pkg
from tests import util

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _bench(out_dir, steps, warmup):
    r = subprocess.run([sys.executable, os.path.join(util.ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, cwd=util.ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    return line, {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_plain_run_and_dumped_outputs(tmp_path):
    from oracle import uplift_oracle as O
    line, out = _bench(tmp_path / "a", steps=3, warmup=2)
    assert line["metric"] == "pose-sequences/sec" and line["unit"] == "pose-sequences/s" and line["higher_is_better"] is True
    assert line["steps"] == 3 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["dtype"].startswith("f16x3")
    assert abs(line["value"] - 128 * 1e3 / line["ms_per_step"]) <= 1e-3 * line["value"]
    assert not {"roofline", "kernel_ms_per_forward", "secondary"} & set(line) and line["cpu_baseline"] is None and line["parity"] is None

    cfg = util.load_config("h36m_351")
    arch = pkg.arch_from_config(cfg)
    B, N, J = 128, arch.num_frames, arch.num_keypoints
    assert set(out) <= {"full", "central", "per_joint_error"} and {"central", "per_joint_error"} <= set(out)
    assert out["central"].dtype == np.float32 and out["central"].shape == (B, J, 3)
    assert out["per_joint_error"].dtype == np.float64 and out["per_joint_error"].shape == (B, J)
    if "full" in out:
        assert out["full"].dtype == np.float32 and out["full"].shape == (B, N, J, 3)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20

    # the inputs bench.py builds (seed 1000 for the windows, 2000 for the ground truth, weights seed 0), on rows of the first,
    # middle and last row tiles
    s_in = cfg.MASK_STRIDE[0] if isinstance(cfg.MASK_STRIDE, list) else cfg.MASK_STRIDE
    x, m = util.synthetic_batch(cfg, B, seed=1000, mask_specs=[(s_in, 0)])
    x = x * m[:, :, None, None].astype(np.float32)
    idx = [0, 1, B // 2, B - 1]
    f32, c32 = O.forward(O.hp_from_arch(arch), pkg.init_weights(arch, seed=0), x[idx], m[idx], torch.float32)
    assert np.abs(out["central"][idx] - c32).max() <= util.TOL_MAX_ABS
    if "full" in out and f32 is not None:
        assert np.abs(out["full"][idx] - f32).max() <= util.TOL_MAX_ABS
    rng = np.random.default_rng(2000)
    gt = np.concatenate([rng.normal(0, 0.3, size=(B, J, 3)), np.ones((B, J, 1))], -1).astype(np.float32)
    ref = O.mpjpe(out["central"], gt, cfg.ROOT_KEYTPOINT, normalize=False)
    assert np.abs(out["per_joint_error"] - ref).max() < 1e-9

    # another run with other step counts: the same inputs, the same outputs
    line2, out2 = _bench(tmp_path / "b", steps=5, warmup=1)
    assert line2["steps"] == 5 and set(out2) == set(out)
    for k in out:
        assert np.allclose(out2[k], out[k], rtol=0, atol=1e-6), k
