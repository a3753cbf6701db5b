"""bench.py --dump-outputs without a GPU: bench.dump_outputs on stand-in results of a timed step — the whole cost vector when
it fits the size limit, a fixed sample of it (the same positions every run) when it does not, one set of files per rank."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _res(n, resident=False):
    costs = np.linspace(-2.0, 50.0, n)
    best = {"index": 7, "cost": 1.5, "vx": 0.25, "vtheta": -0.125, "n_valid": n - 3}
    return {"costs": None if resident else costs, "best": best, "key": (1.5, -0.25, 0.125, -7.0)}


def _load(d):
    return {p[:-4]: np.load(os.path.join(d, p)) for p in sorted(os.listdir(d))}


def test_whole_vector(tmp_path):
    res = _res(1000)
    bench.dump_outputs(str(tmp_path), res, 0, 1)
    out = _load(tmp_path)
    assert sorted(out) == ["best", "best_key", "costs"] and all(a.dtype == np.float64 for a in out.values())
    assert np.array_equal(out["costs"], res["costs"])
    assert out["best"].tolist() == [7.0, 1.5, 0.25, -0.125, 997.0] and out["best_key"].tolist() == [1.5, -0.25, 0.125, -7.0]


def test_sample_of_a_vector_over_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096 + 16 * 100)
    res = _res(5000)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), res, 0, 1)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["best", "best_key", "costs_sample", "costs_sample_index"]
    idx = a["costs_sample_index"].astype(np.int64)
    assert len(idx) == 100 and np.all(np.diff(idx) > 0) and idx[-1] < 5000
    assert np.array_equal(a["costs_sample"], res["costs"][idx])
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_LIMIT_BYTES


def test_ranks_and_resident(tmp_path):
    for r in range(2):
        bench.dump_outputs(str(tmp_path), _res(64), r, 2)
    assert sorted(os.listdir(tmp_path)) == sorted(f"{n}_rank{r}.npy" for n in ("best", "best_key", "costs") for r in range(2))
    bench.dump_outputs(str(tmp_path / "res"), _res(64, resident=True), 0, 1)
    assert sorted(os.listdir(tmp_path / "res")) == ["best.npy", "best_key.npy"]
