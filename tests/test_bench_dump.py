"""bench.py --dump-outputs: what the timed path returned goes to DIR/<name>.npy as float64, within bench.DUMP_LIMIT bytes,
with the same rows for the same arguments (bench.dump_outputs, a pure function of its arrays)."""
import os
import sys

import numpy as np

from conftest import REPO

sys.path.insert(0, REPO)


def _arrays(N, n=81, seed=7):
    rng = np.random.default_rng(seed)
    return {"x": rng.standard_normal((N, n)), "costs": rng.standard_normal((N, 4)),
            "nit": rng.integers(0, 100, N).astype(np.int32), "status": rng.integers(0, 512, N).astype(np.int32)}


def test_small_outputs_are_written_whole_and_exactly(tmp_path):
    import bench
    arr = _arrays(1000)
    assert bench.dump_outputs(str(tmp_path), arr) == 1000
    assert sorted(os.listdir(tmp_path)) == ["costs.npy", "index.npy", "nit.npy", "status.npy", "x.npy"]
    np.testing.assert_array_equal(np.load(tmp_path / "index.npy"), np.arange(1000))
    for k, v in arr.items():
        got = np.load(tmp_path / f"{k}.npy")
        assert got.dtype == np.float64 and np.array_equal(got, v), k


def test_large_outputs_are_a_fixed_sample_within_the_limit(tmp_path):
    import bench
    arr = _arrays(40 * 4096)          # the cfg2 step: 40 batches x 4096 trajectories, 81 variables (~110 MB as float64)
    a, b = tmp_path / "a", tmp_path / "b"
    k = bench.dump_outputs(str(a), arr)
    assert bench.dump_outputs(str(b), arr) == k and 0 < k < 40 * 4096
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) <= bench.DUMP_LIMIT
    idx = np.load(a / "index.npy")
    assert np.array_equal(idx, np.load(b / "index.npy")) and np.all(np.diff(idx) > 0)
    rows = idx.astype(np.int64)
    for key, v in arr.items():
        got = np.load(a / f"{key}.npy")
        assert got.dtype == np.float64 and np.array_equal(got, v[rows]) and np.array_equal(got, np.load(b / f"{key}.npy"))
