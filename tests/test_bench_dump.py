"""bench.py's plain run and --dump-outputs: a run without --full measures the
headline only, and the dump holds what a caller of the timed path receives
(the iterate and the residual norms of the last timed region) as float64
.npy files, at most 64 MB, identical from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


class _Prob:
    def __init__(self, k):
        self.kc = k


class _State:
    """Stands in for the device CG state: get(0) is the padded iterate."""

    def __init__(self, x, k):
        self.x, self.prob = x, _Prob(k)

    def get(self, which):
        assert which == 0
        return self.x


def test_dump_writes_whole_small_iterate(tmp_path):
    x = np.arange(12, dtype=np.float64).reshape(6, 2)
    hist = np.linspace(1.0, 0.1, 5).reshape(5, 1)
    bench.dump_outputs(str(tmp_path / "d"), _State(x, 1), hist)  # creates the folder; 1 real column of 2
    got = np.load(tmp_path / "d" / "x.npy")
    assert got.dtype == np.float64 and got.shape == (6, 1)
    np.testing.assert_array_equal(got[:, 0], x[:, 0])
    np.testing.assert_array_equal(np.load(tmp_path / "d" / "resnorms.npy"), hist)


def test_dump_samples_a_large_iterate_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_X_BYTES", 64 * 8)  # room for 64 values
    x = np.arange(1000, dtype=np.float64).reshape(500, 2)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), _State(x, 2), np.zeros((3, 2)))
    a, b = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "b" / "x.npy")
    assert a.shape == (32, 2) and a.nbytes <= 64 * 8
    np.testing.assert_array_equal(a, b)
    rows = (a[:, 0] / 2).astype(int)  # x[i] = (2 i, 2 i + 1): the rows taken
    assert np.all(np.diff(rows) > 0) and np.array_equal(a, x[rows])


def test_dump_budget_is_within_64_mb():
    assert bench.DUMP_X_BYTES + (1 << 20) <= 64 * 10**6


def test_plain_line_without_a_roofline_pass():
    """A run without --full has no per-launch pass: cfg4_rooflines gives the
    iteration's roofline alone, and compact() prints a line without roofline."""
    n, k, ds = 10_004_569, 8, 50_016_768
    lay = dict(slots=1, slices=1, dia=True, dia_slots=ds, compact=False)
    res = {"n": n, "rhs": k, "layout": lay, "elapsed": 1.3e-3 * 40, "prof": {}, "ydefer": (15, 0)}
    spmv, it = bench.cfg4_rooflines(res, 40)
    assert spmv is None
    vec = n * k * 8
    assert it["bytes_per_iteration"] == pytest.approx(ds * 8 + ds / 128 * 20 + 2 * vec + 6 * vec + 16 / 15 * vec)
    line = {"metric": "m", "value": 3000.0, "unit": "u", "n_gpus": 1, "steps": 40, "warmup": 5, "ms_per_step": 1.3,
            "higher_is_better": True, "dtype": "f64", "iteration_roofline": it}
    c = bench.compact(line, idx={})
    assert "roofline" not in c and "legs" not in c and "cpu_baseline" not in c
    assert c["ms_per_step"] == 1.3 and c["value"] == 3000.0 and c["iteration_roofline"]["frac"] > 0


def _run_bench(*args):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", *args],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_is_the_headline_only_and_dumps_its_outputs(tmp_path):
    """A small stencil (20^3) through the whole command line, twice: the line
    of a plain run has the contract keys and no leg, --steps is the number of
    timed steps, and the two dumps are equal value for value."""
    lines = [_run_bench("--m", "20", "--steps", "37", "--warmup", "3", "--dump-outputs", str(tmp_path / d))
             for d in ("a", "b")]
    line = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 37 and line["warmup"] == 3 and line["repeats"] == 1
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(1e3 / line["ms_per_step"], rel=1e-3)
    for k in ("legs", "roofline", "cpu_baseline"):
        assert k not in line, k
    x, rn = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "a" / "resnorms.npy")
    assert x.dtype == np.float64 and x.shape == (20 ** 3, 1) and np.all(np.isfinite(x))
    assert rn.dtype == np.float64 and rn.shape == (37, 1) and np.all(np.isfinite(rn))
    # 40 CG iterations on the SPD stencil from x0 = 0, b = ones: below ||r_0|| = ||b||
    assert 0.0 < rn[-1, 0] < np.sqrt(20 ** 3)
    # no atomics on data, fixed reduction order: run-to-run bitwise
    np.testing.assert_array_equal(x, np.load(tmp_path / "b" / "x.npy"))
    np.testing.assert_array_equal(rn, np.load(tmp_path / "b" / "resnorms.npy"))
