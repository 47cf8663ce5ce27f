"""bench.py's --dump-outputs helpers on the host: the sample layout they cut, and the fixed sample that keeps a large output within budget."""
import numpy as np

import bench


def test_last_sample_arrays_cut_the_gathered_block():
    N, D, P = 5, 4, 3
    s = np.random.default_rng(1).standard_normal((2, 7, N * D + D + P))          # [chains, results, N*D + D + P]
    o = bench.last_sample_arrays(s, N, D, P)
    assert np.array_equal(o["X"], s[:, -1, :N * D].reshape(2, N, D))
    assert np.array_equal(o["sig_pre"], s[:, -1, N * D:N * D + D]) and np.array_equal(o["th_pre"], s[:, -1, -P:])


def test_dump_outputs_float64_within_budget_and_repeatable(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)
    arrays = {"big": np.arange(2000.0), "flags": np.arange(10, dtype=np.int32)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    a = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in arrays}
    b = {k: np.load(tmp_path / "b" / (k + ".npy")) for k in arrays}
    assert all(v.dtype == np.float64 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 4000
    assert all(np.array_equal(a[k], b[k]) for k in arrays)                        # the same elements in every run
    assert np.all(np.diff(a["big"]) > 0) and np.isin(a["big"], arrays["big"]).all()
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1 << 20)
    bench.dump_outputs(str(tmp_path / "c"), arrays)                               # within budget: written whole
    assert np.array_equal(np.load(tmp_path / "c" / "big.npy"), arrays["big"])
