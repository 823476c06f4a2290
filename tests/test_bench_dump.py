"""bench.py --dump-outputs on the host: what it writes for one window and for a batch, in float32 / float64, and the seeded
row sample that keeps a large output within its 64 MB (the GPU side: tests/test_gpu_bench_multi.py)."""
import os

import numpy as np

import bench


def _res(rng, n, n1):
    return dict(n=n, hole_at=0, paths=rng.integers(0, 7, (n, n1), dtype=np.uint8), hp_current=rng.random(n),
                hp_original=rng.random(n), ratio=rng.random(n), magnitude=rng.random(n), min_marginal=rng.random(n))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_one_window_is_written_whole(tmp_path):
    r = _res(np.random.default_rng(1), 5, 12)
    bench.dump_outputs(str(tmp_path), r, (3, 40, 11))
    z = _load(str(tmp_path))
    assert sorted(z) == sorted(["n", "hole_at", "hp_current", "hp_original", "ratio", "magnitude", "min_marginal", "fill_stats", "paths"])
    assert z["paths"].dtype == np.float32 and np.array_equal(z["paths"], r["paths"])
    assert z["n"].tolist() == [5] and z["fill_stats"].tolist() == [3, 40, 11]
    for k in ("hp_current", "hp_original", "ratio", "magnitude", "min_marginal"):
        assert z[k].dtype == np.float64 and np.array_equal(z[k], r[k]), k


def test_a_batch_goes_window_after_window(tmp_path):
    rng = np.random.default_rng(2)
    rs = [_res(rng, n, 9) for n in (3, 0, 4)]
    bench.dump_outputs(str(tmp_path), rs)
    z = _load(str(tmp_path))
    assert "fill_stats" not in z and "paths_rows" not in z
    assert z["n"].tolist() == [3, 0, 4]
    assert np.array_equal(z["paths"], np.concatenate([r["paths"] for r in rs]))
    assert np.array_equal(z["ratio"], np.concatenate([r["ratio"] for r in rs]))


def test_a_large_output_is_a_fixed_sample_within_64_mb(tmp_path):
    n, n1 = 400, 50001                                      # 80 MB of paths as float32
    r = _res(np.random.default_rng(3), n, n1)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), r)
    bench.dump_outputs(str(b), r)
    za, zb = _load(str(a)), _load(str(b))
    total = sum(os.path.getsize(os.path.join(str(a), f)) for f in os.listdir(str(a)))
    assert total <= 64 << 20 and sum(x.nbytes for x in za.values()) <= 64 << 20
    rows = za["paths_rows"].astype(np.int64)
    assert 0 < len(rows) < n and np.all(np.diff(rows) > 0)
    assert np.array_equal(za["paths"], r["paths"][rows]) and np.array_equal(za["hp_current"], r["hp_current"])
    for k in za:
        assert np.array_equal(za[k], zb[k]), k              # the same sample every time
