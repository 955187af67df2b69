"""bench.py's command line: a plain run times the steps and prints the headline line only, --full adds the other
measurements, --dump-outputs writes what the last timed step left as float32 .npy files (a fixed sample of the hash
grid, the same entries in every run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("roofline", "kernels", "mfma_mlp_train", "line_traffic", "early_steps", "levels16", "psnr", "marching_cubes",
             "cpu_baseline")
# the smallest run of the bench's own path: 4 views of 64x48, 4096 samples and rays per step, 3 timed steps
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "2", "--prepare", "4", "--views", "4", "--width", "64", "--height", "48",
         "--batch", "4096", "--rays", "4096"]


def _bench_module():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def _parse(bench, argv, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_full_and_dump_are_off_by_default(monkeypatch):
    bench = _bench_module()
    a = _parse(bench, ["--gpus", "1", "--steps", "7", "--warmup", "3"], monkeypatch)
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    a = _parse(bench, ["--full", "--dump-outputs", "somewhere"], monkeypatch)
    assert a.full is True and a.dump_outputs == "somewhere"


class _FakeTestbed:
    """Layout of a network with 100 MLP weights, a 3 M-entry grid and the variance; each getter a distinct ramp."""
    N_MLP, N_GRID = 100, 3_000_000

    def layout(self):
        return {"n_params": self.N_MLP + self.N_GRID + 1, "grid_offset": self.N_MLP, "n_grid_params": self.N_GRID}

    def _ramp(self, k):
        return (np.arange(self.N_MLP + self.N_GRID + 1, dtype=np.float64) * k).astype(np.float32)

    def get_params(self):
        return self._ramp(1)

    def get_ema_params(self):
        return self._ramp(2)

    def get_gradients(self):
        return self._ramp(3)


def test_dump_outputs_fixed_sample(tmp_path):
    bench = _bench_module()
    tb = _FakeTestbed()
    st = {"loss": 1.5, "ray_loss": 0.25, "ek_loss": 0.5, "mask_loss": 0.125}
    for d in ("a", "b"):
        bench.dump_outputs(tb, st, str(tmp_path / d))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["ema_params.npy", "gradients.npy", "losses.npy", "params.npy"]
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype == np.float32
        np.testing.assert_array_equal(x, y)
        total += x.nbytes
    assert total <= 64 << 20
    p = np.load(tmp_path / "a" / "params.npy")
    assert p.size == tb.N_MLP + bench.DUMP_GRID_SAMPLE + 1
    # every MLP weight and the variance, and distinct grid entries in ascending order
    np.testing.assert_array_equal(p[: tb.N_MLP], np.arange(tb.N_MLP, dtype=np.float32))
    assert p[-1] == tb.N_MLP + tb.N_GRID
    grid = p[tb.N_MLP: -1]
    assert np.all(np.diff(grid) > 0) and grid[0] >= tb.N_MLP and grid[-1] < tb.N_MLP + tb.N_GRID
    # the same entries of each array
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "gradients.npy"), (p.astype(np.float64) * 3).astype(np.float32))
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "losses.npy"), np.array([1.5, 0.25, 0.5, 0.125], np.float32))


def _run_bench(extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps(torch_cuda, tmp_path):
    out = _run_bench(["--dump-outputs", str(tmp_path / "dump")])
    for k in HEADLINE:
        assert k in out, k
    assert not [k for k in FULL_ONLY if k in out]
    assert out["steps"] == 3 and out["warmup"] == 2 and out["unit"] == "samples/s" and out["higher_is_better"] is True
    assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(4096 * 1e3 / out["ms_per_step"], rel=1e-9)
    arrays = {n: np.load(tmp_path / "dump" / n) for n in sorted(os.listdir(tmp_path / "dump"))}
    assert sorted(arrays) == ["ema_params.npy", "gradients.npy", "losses.npy", "params.npy"]
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["params.npy"].shape == arrays["ema_params.npy"].shape == arrays["gradients.npy"].shape
    assert np.count_nonzero(arrays["gradients.npy"]) > 0 and arrays["losses.npy"].shape == (4,)


@pytest.mark.gpu
def test_full_run_adds_the_other_measurements(torch_cuda):
    out = _run_bench(["--full", "--psnr-steps", "4", "--mc-res", "32", "--cpu-baseline", "0"])
    for k in HEADLINE + tuple(k for k in FULL_ONLY if k != "cpu_baseline"):
        assert k in out, k
    assert out["steps"] == 3 and out["early_steps"]["ms_per_step"] > 0 and out["levels16"]["ms_per_step"] > 0
