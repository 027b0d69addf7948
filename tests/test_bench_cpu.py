"""CPU: bench.py's --dump-outputs writer (the GPU run itself is covered by the GPU suites and the bench line)."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("_ctn_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _arrays():
    g = torch.Generator().manual_seed(3)
    return {"loss": torch.tensor(-1.5), "estimate": torch.randn(2, 2, 100, generator=g),
            "flat_grads": torch.randn(300000, generator=g), "flat_params": torch.randn(300000, generator=g).double()}


def test_dump_outputs_whole_when_it_fits(tmp_path):
    b = _bench()
    arrs = _arrays()
    b.dump_outputs(str(tmp_path), arrs)
    for k, v in arrs.items():
        a = np.load(tmp_path / (k + ".npy"))
        assert a.dtype == np.float32 and a.shape == tuple(v.shape)
        assert np.array_equal(a, v.float().numpy())


def test_dump_outputs_samples_within_the_limit_and_repeats(tmp_path, monkeypatch):
    b = _bench()
    monkeypatch.setattr(b, "DUMP_LIMIT_BYTES", 10 ** 6)
    arrs = _arrays()
    b.dump_outputs(str(tmp_path / "a"), arrs)
    b.dump_outputs(str(tmp_path / "b"), arrs)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 10 ** 6
    for k, v in arrs.items():
        a, a2 = np.load(tmp_path / "a" / (k + ".npy")), np.load(tmp_path / "b" / (k + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, a2)          # the same sample every run
        flat = v.float().numpy().reshape(-1)
        if k in ("loss", "estimate"):
            assert np.array_equal(a.reshape(-1), flat)                  # small arrays stay whole
        else:
            assert 0 < a.size < flat.size and np.isin(a, flat).all()    # the large ones are a sample of their elements
