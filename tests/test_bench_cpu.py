"""bench.py without a GPU: --dump-outputs' writer (dtypes, the 64 MB bound, a seeded sample), the step loop handing back the
last step's outputs, and the argument checks that run before anything touches a device."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from tests import util


def test_dump_outputs_writes_float_arrays_and_skips_missing(tmp_path):
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    b = np.linspace(0, 1, 5)
    c = np.arange(6, dtype=np.int32)
    shapes = bench.dump_outputs(str(tmp_path / "out"), {"a": a, "b": b, "c": c, "none": None})
    assert shapes == {"a": [3, 4], "b": [5], "c": [6]}
    assert sorted(os.listdir(tmp_path / "out")) == ["a.npy", "b.npy", "c.npy"]
    ra, rb, rc = (np.load(tmp_path / "out" / f"{n}.npy") for n in "abc")
    assert ra.dtype == np.float32 and np.array_equal(ra, a)
    assert rb.dtype == np.float64 and np.array_equal(rb, b)
    assert rc.dtype == np.float64 and np.array_equal(rc, c)                 # (other dtypes are widened to float64)


def test_dump_outputs_stays_within_64_mb_with_a_fixed_sample(tmp_path, monkeypatch):
    assert bench.DUMP_LIMIT_BYTES == 64 << 20
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)                     # (the same rule as at 64 MB, on small arrays)
    small = np.ones(100, dtype=np.float64)                                   # 928 bytes with its header
    big = np.arange(10000, dtype=np.float32)
    d1, d2 = str(tmp_path / "1"), str(tmp_path / "2")
    bench.dump_outputs(d1, {"small": small, "big": big})
    bench.dump_outputs(d2, {"small": small, "big": big})
    total = sum(os.path.getsize(os.path.join(d1, f)) for f in os.listdir(d1))
    assert total <= 4096
    s1, s2 = np.load(os.path.join(d1, "big.npy")), np.load(os.path.join(d2, "big.npy"))
    assert 0 < s1.size < big.size and s1.dtype == np.float32
    assert np.array_equal(s1, s2)                                            # same size and seed: the same elements
    assert np.all(np.diff(s1) > 0) and np.all(np.isin(s1, big))              # elements of the output, in order
    assert np.array_equal(np.load(os.path.join(d1, "small.npy")), small)     # what fits is written whole


class _Pipe:
    """ForwardPipeline's surface for run_pipelined_steps: step k's outputs are filled with k."""

    def __init__(self, depth):
        self.n, self.depth, self.live = 0, depth, {}

    def launch(self, wait_caller=True):
        t = self.n
        self.n += 1
        assert len(self.live) < self.depth
        self.live[t] = (torch.full((2, 3, 17, 3), float(t)), torch.full((2, 17, 3), float(t)), torch.full((2, 17), float(t), dtype=torch.float64))
        return t

    def result(self, t):
        return self.live.pop(t)

    def after(self, t, fn):
        return fn(*self.live.pop(t))

    def join(self):
        pass


@pytest.mark.parametrize("mode", ["end", "step"])
@pytest.mark.parametrize("steps,depth", [(1, 4), (7, 3), (8, 8)])
def test_step_loop_returns_the_last_steps_outputs(mode, steps, depth):
    pipe = _Pipe(depth)
    g = bench.ErrorGather(mode, steps, 2, 17, 1, "cpu", False)
    bench.run_pipelined_steps(pipe, 5, depth, g)                             # warm-up
    full, central, err = bench.run_pipelined_steps(pipe, steps, depth, g)
    last = 5 + steps - 1
    assert g.k == steps and pipe.n == 5 + steps
    assert torch.all(full == last) and torch.all(central == last) and torch.all(err == last)
    assert torch.all(g.local[steps - 1] == last)


def test_bad_step_counts_are_refused_before_any_device_work():
    for argv in (["--steps", "0"], ["--warmup", "-1"]):
        r = subprocess.run([sys.executable, os.path.join(util.ROOT, "bench.py"), *argv], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--steps must be >= 1" in r.stderr


def test_full_and_dump_outputs_are_options():
    r = subprocess.run([sys.executable, os.path.join(util.ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs DIR" in r.stdout
