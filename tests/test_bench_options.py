"""bench.py's command line without a GPU: a plain run is leg 1 alone and everything else needs --full, bad options
are refused before anything starts, and the --dump-outputs writer turns a downloaded state into float64 arrays."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("args", [("--legs", "batched"), ("--legs", "pivots,cfg2b"), ("--steps", "0"),
                                  ("--full", "--legs", "nope"), ("--full", "--legs", "batched", "--dump-outputs", "x")])
def test_bench_refuses_bad_options(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       timeout=120, cwd=ROOT)
    assert r.returncode == 2 and not r.stdout, r.stdout + r.stderr
    assert "error:" in r.stderr


def test_dump_outputs_writes_float64_arrays(tmp_path):
    import bench
    rng = np.random.default_rng(3)
    rows, W = 700, 24
    got = dict(tab=rng.standard_normal((rows, W)), tgtf=rng.standard_normal(W), rhs=W - 1,
               eq2bv=rng.permutation(rows).astype(np.int32), bv2eq=rng.integers(-1, rows, W - 1).astype(np.int32))
    names = bench.dump_outputs(got, str(tmp_path / "a"))
    assert bench.dump_outputs(got, str(tmp_path / "b")) == names
    a = {n: np.load(str(tmp_path / "a" / (n + ".npy"))) for n in names}
    b = {n: np.load(str(tmp_path / "b" / (n + ".npy"))) for n in names}
    assert all(x.dtype == np.float64 and np.array_equal(x, b[n]) for n, x in a.items())     # the same sample every time
    assert a["tableau_rows"].shape == (bench.DUMP_ROWS, W)
    assert all((got["tab"] == r).all(axis=1).any() for r in a["tableau_rows"])
    assert np.array_equal(a["tableau_rhs_column"], got["tab"][:, -1]) and np.array_equal(a["objective_row"], got["tgtf"])
    assert np.array_equal(a["eq2bv"], got["eq2bv"]) and np.array_equal(a["bv2eq"], got["bv2eq"])
