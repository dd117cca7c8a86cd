"""CPU checks of bench.py's command line: --full is off by default, and --dump-outputs writes float32 arrays within the
size cap, sampling the same elements every time when the outputs are larger."""
import os
import sys

import numpy as np
import torch


def _bench(monkeypatch):
    # bench.py sets SRF_SPLIT_TUNE_AFTER for its own process only when it is unset: keep it from leaking into this session
    monkeypatch.setenv("SRF_SPLIT_TUNE_AFTER", os.environ.get("SRF_SPLIT_TUNE_AFTER", "3"))
    import bench
    return bench


def test_plain_run_is_the_default(monkeypatch):
    bench = _bench(monkeypatch)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_float32_and_capped(monkeypatch, tmp_path):
    bench = _bench(monkeypatch)
    g = torch.Generator().manual_seed(0)
    small = {"out": torch.randn(2, 3, 5, generator=g), "loss": torch.tensor([1.5], dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path / "small"), small)
    for name, t in small.items():
        a = np.load(tmp_path / "small" / (name + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, t.float().numpy())
    big = {"a": torch.randn(3000, generator=g), "b": torch.randn(1000, generator=g)}
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4 * 400)
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), big)
    total = 0
    for name, t in big.items():
        a, b = np.load(tmp_path / "x" / (name + ".npy")), np.load(tmp_path / "y" / (name + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, b)            # the same seeded sample in every run
        assert np.isin(a, t.numpy()).all() and a.size == t.numel() // 10    # each array keeps the same share
        total += a.nbytes
    assert total <= 4 * 400
