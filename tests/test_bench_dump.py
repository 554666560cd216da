"""`bench.py --dump-outputs`: the last timed step's outputs as float32 / float64 .npy files, exact, within the size
budget, and -- when the layer is sampled -- the same rows on every run."""
import importlib.util
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _outs(seed):
    g = torch.Generator().manual_seed(seed)
    outs = {}
    for name, R, K in (("q_proj", 96, 256), ("down_proj", 64, 512), ("experts.3.w1", 160, 256)):
        outs[f"{name}.weight_packed"] = torch.randint(-2 ** 31, 2 ** 31 - 1, (R, K // 8), generator=g, dtype=torch.int32)
        outs[f"{name}.weight_scale"] = torch.rand((R, K // 128), generator=g).to(torch.bfloat16)
    return outs


def test_full_dump_is_exact(tmp_path):
    bench = _bench()
    outs = _outs(0)
    bench.dump_outputs(outs, tmp_path)
    names = sorted(p.name for p in tmp_path.iterdir())
    assert names == sorted([f"{k}.npy" for k in outs] + [f"{n}.rows.npy" for n in ("q_proj", "down_proj", "experts.3.w1")])
    for k, t in outs.items():
        a = np.load(tmp_path / f"{k}.npy")
        assert a.dtype == (np.float64 if t.dtype == torch.int32 else np.float32)
        assert np.array_equal(a, t.to(torch.float64).numpy())


def test_sampled_dump_fits_the_budget_and_repeats(tmp_path):
    bench = _bench()
    bench.DUMP_BUDGET_BYTES = 40_000
    outs = _outs(1)
    for d in ("a", "b"):
        bench.dump_outputs(outs, tmp_path / d)
    files = sorted((tmp_path / "a").iterdir())
    assert sum(p.stat().st_size for p in files) <= 40_000 + 128 * len(files)      # payload + .npy headers
    for p in files:
        assert np.array_equal(np.load(p), np.load(tmp_path / "b" / p.name))
    for name in ("q_proj", "down_proj", "experts.3.w1"):
        rows = np.load(tmp_path / "a" / f"{name}.rows.npy")
        packed = outs[f"{name}.weight_packed"]
        assert 0 < len(rows) < packed.shape[0] and np.all(np.diff(rows) > 0)
        idx = torch.from_numpy(rows.astype(np.int64))
        assert np.array_equal(np.load(tmp_path / "a" / f"{name}.weight_packed.npy"),
                              packed[idx].to(torch.float64).numpy())
        assert np.array_equal(np.load(tmp_path / "a" / f"{name}.weight_scale.npy"),
                              outs[f"{name}.weight_scale"][idx].float().numpy())
