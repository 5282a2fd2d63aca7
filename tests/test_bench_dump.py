"""bench.py --dump-outputs (dump_outputs): the planes of the last timed frame as float32 / float64 .npy files, whole
where they fit the budget and otherwise the same seeded sample of pixels in every plane; child_argv drops the options
a child run of the bench must not inherit. CPU only."""
import os

import numpy as np

import bench


def _planes(n):
    rng = np.random.default_rng(1)
    return {"rgba": rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32),
            "depth": rng.random(n, dtype=np.float32),
            "value": rng.integers(-1, 2 ** 31 - 1, size=n, dtype=np.int64).astype(np.int32),
            "normal": rng.random((n, 3), dtype=np.float32)}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_whole_planes(tmp_path):
    p = _planes(1000)
    bench.dump_outputs(str(tmp_path / "a"), p)
    got = _load(str(tmp_path / "a"))
    assert sorted(got) == ["depth", "normal", "rgba", "value"]
    assert got["rgba"].dtype == np.float32 and got["rgba"].shape == (1000, 4)
    assert np.array_equal(got["rgba"].astype(np.uint8), p["rgba"].view(np.uint8).reshape(-1, 4))
    assert got["depth"].dtype == np.float32 and np.array_equal(got["depth"], p["depth"])
    assert got["value"].dtype == np.float64 and np.array_equal(got["value"], p["value"])
    assert got["normal"].dtype == np.float32 and np.array_equal(got["normal"], p["normal"])


def test_dump_sample_fits_budget_and_repeats(tmp_path, monkeypatch):
    p = _planes(1000)
    per_pixel = 16 + 4 + 8 + 12
    monkeypatch.setattr(bench, "DUMP_BUDGET", 100 * per_pixel + per_pixel - 1)
    bench.dump_outputs(str(tmp_path / "a"), p)
    bench.dump_outputs(str(tmp_path / "b"), {k: v.copy() for k, v in p.items()})
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sum(v.nbytes for v in a.values()) == 100 * per_pixel
    sel = np.sort(np.random.default_rng(0).choice(1000, size=100, replace=False))
    for k in a:
        assert len(a[k]) == 100 and np.array_equal(a[k], b[k])
    assert np.array_equal(a["depth"], p["depth"][sel]) and np.array_equal(a["value"], p["value"][sel])
    assert np.array_equal(a["normal"], p["normal"][sel])


def test_dump_is_finite_and_marks_nonfinite_entries(tmp_path):
    p = _planes(1000)
    p["depth"][[3, 500]] = np.inf  # the depth of a miss
    p["normal"][7, 1] = np.nan
    p["normal"][8, 2] = -np.inf
    bench.dump_outputs(str(tmp_path / "a"), p)
    got = _load(str(tmp_path / "a"))
    assert sorted(got) == ["depth", "depth_nonfinite", "normal", "normal_nonfinite", "rgba", "value"]
    assert all(np.isfinite(v).all() and v.dtype in (np.float32, np.float64) for v in got.values())
    m = got["depth_nonfinite"]
    assert m.shape == (1000,) and np.array_equal(np.nonzero(m)[0], [3, 500]) and (m[[3, 500]] == 1).all()
    assert (got["depth"][[3, 500]] == 0).all() and np.array_equal(got["depth"][m == 0], p["depth"][m == 0])
    mn = got["normal_nonfinite"]
    assert mn.shape == (1000, 3) and mn[7, 1] == 3 and mn[8, 2] == 2 and mn.sum() == 5
    assert got["normal"][7, 1] == 0 and got["normal"][8, 2] == 0


def test_child_argv_drops_full_and_dump(monkeypatch):
    monkeypatch.setattr(bench.sys, "argv", ["bench.py", "--full", "--steps", "3", "--dump-outputs", "d", "--shadows",
                                            "--dump-outputs=e"])
    assert bench.child_argv() == ["--steps", "3", "--shadows"]
