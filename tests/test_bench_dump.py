"""bench.py --dump-outputs and --full without a GPU: Workload.dump on host tensors (every row when the outputs fit the budget, the
same seeded sample of rows for every output when they do not), and the defaults of the two options."""
import os
import sys

import numpy as np
import torch

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)
import bench


def _workload(kind, n, batches):
    wl = bench.Workload.__new__(bench.Workload)
    wl.kind, wl.n, wl.dev = kind, n, torch.device("cpu")
    wl.batches = []
    g = np.random.default_rng(7)
    for _ in range(batches):
        B = bench.Batch()
        for _, attr, width in bench.OUTPUTS[kind]:
            setattr(B, attr, torch.from_numpy(g.integers(0, 256, n * width, dtype=np.uint8)))
        wl.batches.append(B)
    return wl


def test_dump_writes_every_row_of_the_last_steps_batch(tmp_path):
    wl = _workload("sign", 1000, 3)
    shapes = wl.dump(7, str(tmp_path))                 # launch 7 used batch 7 % 3
    B = wl.batches[1]
    assert shapes == {"r8": [1000, 64], "s": [1000, 32], "ok": [1000]}
    assert sorted(os.listdir(tmp_path)) == ["ok.npy", "r8.npy", "s.npy"]
    for name, attr, width in bench.OUTPUTS["sign"]:
        a = np.load(tmp_path / (name + ".npy"))
        assert a.dtype == np.float32
        assert (a.reshape(1000, width) == getattr(B, attr).numpy().reshape(1000, width)).all()


def test_dump_samples_rows_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * 97 * 100)      # room for 100 rows of 64 + 32 + 1 bytes
    wl = _workload("sign", 5000, 2)
    wl.dump(0, str(tmp_path / "a"))
    wl.dump(0, str(tmp_path / "b"))
    rows = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(5000, 100, replace=False))
    total = 0
    for name, attr, width in bench.OUTPUTS["sign"]:
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert (a == b).all() and a.shape[0] == 100
        assert (a.reshape(100, width) == getattr(wl.batches[0], attr).numpy().reshape(5000, width)[rows]).all()
        total += a.nbytes
    assert total <= bench.DUMP_BYTES


def test_every_workload_names_its_outputs():
    assert set(bench.OUTPUTS) == set(bench.ALGO_BYTES)
    assert bench.DUMP_BYTES <= 64 << 20


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 5 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "out"
