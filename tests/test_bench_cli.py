"""bench.py's command line and its --dump-outputs writer (CPU; no GPU work)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    """--full and --dump-outputs are off unless asked for; --steps / --warmup
    set the timed and untimed step counts."""
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None
    a = _parse(monkeypatch, "--full", "--dump-outputs", "somewhere")
    assert a.full is True and a.dump_outputs == "somewhere"


def test_dump_outputs_whole_arrays(tmp_path):
    """Under the budget every array is saved whole, in its shape, as float32;
    None entries (no gate with one sub-NeRF) are left out."""
    g = torch.Generator().manual_seed(0)
    t = {"rgb": torch.rand(33, 3, generator=g), "depth": torch.rand(33, 2, generator=g).double(),
         "gate": None, "grid_grad": torch.rand(1000, generator=g)}
    saved = bench.dump_outputs(str(tmp_path / "d"), t)
    assert sorted(saved) == ["depth", "grid_grad", "rgb"]
    assert sorted(os.listdir(tmp_path / "d")) == ["depth.npy", "grid_grad.npy", "rgb.npy"]
    for k in saved:
        a = np.load(tmp_path / "d" / (k + ".npy"))
        assert a.dtype == np.float32 and list(a.shape) == saved[k][0] and a.size == saved[k][1]
        assert np.array_equal(a, t[k].float().numpy())


def test_dump_outputs_samples_over_budget(tmp_path, monkeypatch):
    """Over the budget the large arrays are cut to a fixed sample: within the
    budget in all, elements of the array itself, the same on every call."""
    monkeypatch.setattr(bench, "DUMP_BUDGET", 3 << 20)
    g = torch.Generator().manual_seed(1)
    big = torch.rand(1 << 20, 2, generator=g)              # 8 MiB
    mid = torch.rand(300000, generator=g)                   # 1.14 MiB: over 1 MiB, under its share
    small = torch.rand(100, 3, generator=g)
    t = {"rgb": small, "mlp_grad": mid, "grid_grad": big}
    s1 = bench.dump_outputs(str(tmp_path / "a"), t)
    s2 = bench.dump_outputs(str(tmp_path / "b"), t)
    assert s1 == s2
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= (3 << 20) + 3 * 128                     # payload + the .npy headers
    a, b = (np.load(tmp_path / d / "grid_grad.npy") for d in "ab")
    assert a.dtype == np.float32 and a.ndim == 1 and np.array_equal(a, b)
    assert s1["grid_grad"] == [[1 << 20, 2], a.size] and a.size < big.numel()
    idx = np.sort(np.random.default_rng(0).integers(0, big.numel(), a.size))
    assert np.array_equal(a, big.reshape(-1).numpy()[idx])
    assert np.array_equal(np.load(tmp_path / "a" / "mlp_grad.npy"), mid.numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "rgb.npy"), small.numpy())
