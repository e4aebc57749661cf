"""bench.py's contract: a plain run prints the headline keys only, --steps sets the timed steps, and --dump-outputs
writes the last timed step's state as float .npy files under a 64 MB cap."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from _gpu_child import ROOT, run

DUMPED = ("params", "grads", "exp_avg", "exp_avg_sq", "loss")


class _FakeEngine:
    """Host tensors behind the SirenEngine calls dump_outputs makes."""
    out_features, npix = 3, 100

    def __init__(self, n):
        self.n = n

    def get_params(self):
        return torch.arange(self.n, dtype=torch.float32)

    def get_grads(self):
        return torch.full((self.n,), -1.0)

    def get_adam_state(self):
        return torch.zeros(self.n), torch.full((self.n,), 2.0), 7

    def sse_view(self):
        return torch.tensor([30.0], dtype=torch.float64)


@pytest.mark.parametrize("n", [1000, (3 << 20) + 17])
def test_dump_outputs_files_dtypes_and_cap(tmp_path, n):
    import bench
    bench.dump_outputs(_FakeEngine(n), str(tmp_path / "a"))
    bench.dump_outputs(_FakeEngine(n), str(tmp_path / "b"))
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f + ".npy" for f in DUMPED)
    total = 0
    for f in DUMPED:
        a, b = np.load(tmp_path / "a" / (f + ".npy")), np.load(tmp_path / "b" / (f + ".npy"))
        total += os.path.getsize(tmp_path / "a" / (f + ".npy"))
        assert a.dtype in (np.float32, np.float64)
        assert np.array_equal(a, b)                                  # the sample is fixed
    assert total <= 64e6
    p = np.load(tmp_path / "a" / "params.npy")
    assert p.size == min(n, bench.DUMP_MAX_ELEMS)
    assert np.all(np.diff(p) > 0) and p[-1] < n                      # sorted, distinct entries of the array
    assert np.load(tmp_path / "a" / "loss.npy")[0] == 0.1            # SSE / (3 * npix)


@pytest.mark.gpu
def test_plain_bench_run_and_dump(tmp_path):
    stdout = run([sys.executable, os.path.join(ROOT, "bench.py"), "--size", "256", "--steps", "3", "--warmup", "1",
                  "--dump-outputs", str(tmp_path)], timeout=300, split=True)
    line = json.loads(stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0
    for k in ("roofline", "kernels", "cpu_baseline", "by_scratch_format", "psnr_after_run"):
        assert k not in line                                         # --full only
    n = 2 * 256 + 256 + 6 * (256 * 256 + 256) + 3 * 256 + 3
    for f in DUMPED:
        a = np.load(tmp_path / (f + ".npy"))
        assert a.shape == ((1,) if f == "loss" else (n,)) and np.all(np.isfinite(a))
    assert np.any(np.load(tmp_path / "grads.npy") != 0) and 0 < np.load(tmp_path / "loss.npy")[0] < 1
