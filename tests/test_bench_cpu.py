"""bench.py --dump-outputs without a GPU: what dump_outputs writes for outputs below and above its 64 MB budget."""
import os

import numpy as np

import bench


def test_small_outputs_are_written_whole_in_float64(tmp_path):
    F = np.random.default_rng(1).random((56, 7634))
    bench.dump_outputs(str(tmp_path), {"F_nu": F, "spectrum": F[-1].astype(np.float32)})
    assert np.array_equal(np.load(tmp_path / "F_nu.npy"), F)
    s = np.load(tmp_path / "spectrum.npy")
    assert s.dtype == np.float64 and np.array_equal(s, F[-1].astype(np.float32))


def test_large_outputs_keep_the_same_seeded_columns_within_64_mb(tmp_path):
    n_d, n_nu = 56, 120398  # S-c3 / S-c4m: two (N_d, N_nu) planes of 54 MB each
    col = np.arange(n_nu, dtype=np.float64)
    arrays = {"F_nu": np.broadcast_to(col, (n_d, n_nu)), "total_alphas": np.broadcast_to(-col, (n_d, n_nu))}
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), arrays)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["F_nu.npy", "total_alphas.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 10**6 + 1024
    F, T = np.load(tmp_path / "a" / "F_nu.npy"), np.load(tmp_path / "a" / "total_alphas.npy")
    kept = F[0]
    assert F.shape == T.shape and F.shape[0] == n_d and 0 < kept.size < n_nu
    assert np.all(np.diff(kept) > 0) and np.array_equal(T, -F) and np.all(F == kept)  # the same columns, in order, in every array
    for f in files:  # the sample is fixed: two runs write the same bytes
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
