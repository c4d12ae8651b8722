"""CPU tests of bench.py --dump-outputs' writer: every output becomes DIR/<name>.npy in float32 or
float64, and outputs over the byte budget are cut to a fixed, seeded sample of their rows (the
same rows in every run and in arrays of equal leading size)."""
import numpy as np

import bench


def _arrays():
    rng = np.random.default_rng(5)
    return {"xi": rng.standard_normal((1000, 7, 2)), "vrp32": rng.standard_normal((1000, 6)).astype(np.float32),
            "status": np.arange(1000, dtype=np.int32), "window": {"omega": np.zeros(3)}}


def test_small_outputs_are_written_whole(tmp_path):
    arr = _arrays()
    bench.dump_outputs(str(tmp_path), arr)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["status.npy", "vrp32.npy", "xi.npy"]
    xi, v32, st = (np.load(tmp_path / f"{k}.npy") for k in ("xi", "vrp32", "status"))
    assert xi.dtype == np.float64 and v32.dtype == np.float32 and st.dtype == np.float64
    np.testing.assert_array_equal(xi, arr["xi"])
    np.testing.assert_array_equal(v32, arr["vrp32"])
    np.testing.assert_array_equal(st, arr["status"])


def test_large_outputs_keep_a_fixed_sample_of_rows(tmp_path, monkeypatch):
    arr = _arrays()
    monkeypatch.setattr(bench, "DUMP_BYTES", 40000)
    bench.dump_outputs(str(tmp_path / "a"), arr)
    bench.dump_outputs(str(tmp_path / "b"), arr, rank=1, world=2)
    a = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in ("xi", "vrp32", "status")}
    assert sum(v.nbytes for v in a.values()) <= 40000
    rows = a["status"].astype(np.int64)
    assert 1 < len(rows) < 1000 and (np.diff(rows) > 0).all()
    np.testing.assert_array_equal(a["xi"], arr["xi"][rows])          # the same rows in every array
    np.testing.assert_array_equal(a["vrp32"], arr["vrp32"][rows])
    b = {k: np.load(tmp_path / "b" / f"{k}_rank1.npy") for k in ("xi", "vrp32", "status")}
    assert sum(v.nbytes for v in b.values()) <= 20000                 # the budget is shared by the ranks
    np.testing.assert_array_equal(b["xi"], arr["xi"][b["status"].astype(np.int64)])
    bench.dump_outputs(str(tmp_path / "c"), arr)                      # a second run: the same rows
    np.testing.assert_array_equal(np.load(tmp_path / "c" / "status.npy"), a["status"])
