"""bench.py --dump-outputs without a GPU: the sample of a long vector is fixed, the files are float32 / float64 and stay
under 64 MB, and a sharded run writes the same arrays as an unsharded one (stand-in problems in place of the library)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class FakeProblem:
    SCALAR_NAMES = ("k", "gamma")

    def __init__(self, full, lo, hi):
        self.vecs = {k: v[lo:hi] for k, v in full.items()}
        self.n = hi - lo

    def panoc_vector(self, which):
        return self.vecs[which].copy()

    def panoc_scalars(self):
        return {"k": 35.0, "gamma": 0.5}


class FakeGroup:
    """allgather over ranks whose contributions were recorded beforehand (rank order)"""

    def __init__(self, parts):
        self.parts = parts

    def allgather(self, b):
        return self.parts.pop(0)


def _full(n, dtype):
    rng = np.random.default_rng(1)
    return {k: rng.standard_normal(n).astype(dtype) for k in ("z", "x", "res")}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_sample_index_is_fixed_sorted_and_bounded():
    a, b = bench.dump_sample_index(10_000_000), bench.dump_sample_index(10_000_000)
    assert np.array_equal(a, b) and len(a) <= bench.DUMP_SAMPLE and len(a) > bench.DUMP_SAMPLE * 0.9
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < 10_000_000
    assert np.array_equal(bench.dump_sample_index(1000), np.arange(1000))


def test_dump_writes_float_arrays_under_64mb(tmp_path):
    n = 3 * bench.DUMP_SAMPLE
    full = _full(n, np.float64)
    bench.dump_outputs(str(tmp_path), FakeProblem(full, 0, n))
    out = _load(str(tmp_path))
    assert set(out) == {"z", "x", "res", "index", "scalars"}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)) <= 64 * 2 ** 20
    idx = out["index"].astype(np.int64)
    assert np.array_equal(idx, bench.dump_sample_index(n)) and np.array_equal(out["x"], full["x"][idx])
    assert list(out["scalars"]) == [35.0, 0.5]


def test_sharded_dump_matches_the_unsharded_one(tmp_path):
    n, cut = 3 * bench.DUMP_SAMPLE + 7, 1_234_567
    full = _full(n, np.float32)
    bench.dump_outputs(str(tmp_path / "one"), FakeProblem(full, 0, n))
    idx = bench.dump_sample_index(n)
    parts = []      # what each rank contributes to the three allgathers (z, x, res)
    for name in ("z", "x", "res"):
        parts.append([full[name][idx[idx < cut]].tobytes(), full[name][idx[idx >= cut]].tobytes()])
    bench.dump_outputs(str(tmp_path / "two"), FakeProblem(full, 0, cut), n, 0, FakeGroup(parts), 0)
    one, two = _load(str(tmp_path / "one")), _load(str(tmp_path / "two"))
    assert set(one) == set(two) and all(np.array_equal(one[k], two[k]) and one[k].dtype == two[k].dtype for k in one)
