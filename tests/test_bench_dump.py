"""CPU-only checks of bench.py --dump-outputs: the files it writes fit the size limit, hold float32 or float64, keep small
arrays whole, and sample a large one at the same positions every time."""
import os

import numpy as np

import bench


def _arrays():
    rng = np.random.default_rng(3)
    return {"refno": np.arange(4096, dtype=np.int32), "flip": (np.arange(4096) % 2).astype(np.uint8),
            "sx": rng.standard_normal(4096), "volume": rng.standard_normal((64, 64, 64)),
            "aligned_sum": rng.standard_normal((300, 400)).astype(np.float32)}


def test_dump_outputs_within_the_limit_and_repeatable(tmp_path):
    arrays = _arrays()
    limit = 1 << 20                                   # below the volume's 2 MB: the volume is sampled
    info_a = bench.dump_outputs(str(tmp_path / "a"), arrays, limit=limit)
    info_b = bench.dump_outputs(str(tmp_path / "b"), arrays, limit=limit)
    assert info_a == info_b
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(k + ".npy" for k in arrays)
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= limit
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64)
        assert np.array_equal(a, b)
    for k in ("refno", "flip", "sx"):
        assert not info_a[k][1]
        assert np.array_equal(np.load(tmp_path / "a" / (k + ".npy")), arrays[k].astype(np.float64))
    assert np.load(tmp_path / "a" / "aligned_sum.npy").dtype == np.float32
    assert info_a["volume"] == ([64, 64, 64], True)
    v = np.load(tmp_path / "a" / "volume.npy")
    assert 0 < v.size < arrays["volume"].size and np.isin(v, arrays["volume"]).all()


def test_dump_outputs_whole_when_small(tmp_path):
    arrays = _arrays()
    info = bench.dump_outputs(str(tmp_path), arrays)
    assert not any(s for _, s in info.values())
    assert np.array_equal(np.load(tmp_path / "volume.npy"), arrays["volume"])
