"""bench.py --dump-outputs on the CPU: bench.dump_outputs writes every array as float32, whole when the arrays fit the byte limit,
and otherwise the same fixed, seeded sample of each from run to run, within the limit."""
import importlib.util
import os

import numpy as np
import torch

from helpers import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("gsr_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _arrays():
    g = torch.Generator().manual_seed(3)
    return {"color": torch.rand(3, 48, 64, generator=g), "radii": torch.randint(0, 300, (5000,), generator=g, dtype=torch.int32),
            "invdepth": torch.rand(1, 48, 64, generator=g, dtype=torch.float64)}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_writes_whole_arrays_as_float32(tmp_path):
    bench, arrays = _bench(), _arrays()
    bench.dump_outputs(str(tmp_path / "out"), arrays)
    got = _load(tmp_path / "out")
    assert sorted(got) == ["color", "invdepth", "radii"]
    for name, t in arrays.items():
        assert got[name].dtype == np.float32 and got[name].shape == tuple(t.shape)
        assert np.array_equal(got[name], t.float().numpy())


def test_dump_outputs_samples_each_array_the_same_way_above_the_limit(tmp_path, monkeypatch):
    bench, arrays = _bench(), _arrays()
    total = sum(4 * t.numel() for t in arrays.values())
    limit = total // 4 + 1024 * len(arrays)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", limit)
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(os.path.getsize(tmp_path / "a" / f"{n}.npy") for n in a) <= limit
    frac = (limit - 1024 * len(arrays)) / total
    for name, t in arrays.items():
        n = t.numel()
        assert a[name].dtype == np.float32 and a[name].shape == (int(n * frac),) and 0 < int(n * frac) < n
        assert np.array_equal(a[name], b[name])                                   # the same sample from run to run
        idx = torch.randperm(n, generator=torch.Generator().manual_seed(bench.DUMP_SAMPLE_SEED))[:int(n * frac)].sort().values
        assert np.array_equal(a[name], t.float().reshape(-1)[idx].numpy())      # the values at the seeded positions, in order
