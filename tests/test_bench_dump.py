"""CPU: bench.py --dump-outputs writes the last timed step's outputs -- small arrays whole, large tables as a seeded row sample
within the byte budget, the same rows on every run -- and rejects arguments it cannot honour."""
import os
import subprocess
import sys

import numpy as np
import torch

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_writes_small_arrays_whole_and_samples_large_tables(tmp_path, monkeypatch):
    bench = _bench_module()
    monkeypatch.setattr(bench, "DUMP_BYTES", 64 << 10)
    monkeypatch.setattr(bench, "DUMP_WHOLE_BYTES", 4 << 10)
    g = torch.Generator().manual_seed(0)
    outputs = {"loss": torch.tensor([0.6931], dtype=torch.float32), "w": torch.randn(16, 8, generator=g),
               "U": torch.randn(5000, 16, generator=g), "I": torch.randn(20000, 16, generator=g), "d": torch.randn(100, 4, dtype=torch.float64, generator=g)}
    man = bench.dump_outputs(outputs, str(tmp_path / "a"))
    assert set(man) == set(outputs)
    total = 0
    for k, t in outputs.items():
        a = np.load(tmp_path / "a" / (k + ".npy"))
        total += a.nbytes
        assert a.dtype == (np.float64 if k == "d" else np.float32)
        if man[k]["rows"] == "all":
            np.testing.assert_array_equal(a, t.numpy())
        else:
            rows = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(t.shape[0], size=a.shape[0], replace=False))
            np.testing.assert_array_equal(a, t.numpy()[rows])
            assert 0 < a.shape[0] < t.shape[0] and man[k]["of"] == list(t.shape)
    assert man["U"]["rows"] == man["I"]["rows"] == "sampled" and man["w"]["rows"] == man["d"]["rows"] == "all"
    assert total <= bench.DUMP_BYTES
    bench.dump_outputs(outputs, str(tmp_path / "b"))        # same inputs, same files
    for k in outputs:
        np.testing.assert_array_equal(np.load(tmp_path / "a" / (k + ".npy")), np.load(tmp_path / "b" / (k + ".npy")))


def test_bench_rejects_what_it_cannot_honour(tmp_path):
    for argv in (["--steps", "0"], ["--warmup", "-1"], ["--gpus", "2", "--dump-outputs", str(tmp_path)]):
        p = subprocess.run([sys.executable, BENCH] + argv, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert p.returncode == 2 and "error" in p.stderr, (argv, p.stderr[-2000:])
        assert not [l for l in p.stdout.splitlines() if l.startswith("{")]
