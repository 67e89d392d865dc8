"""bench.py's plain single-GPU line and its --dump-outputs files: the timed steps are the --steps asked for, ms_per_step and value
describe the same time, a plain run carries none of the --full legs, and the arrays the last timed step returned are written as
float64 .npy files that are the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMPED = ("x.npy", "x_rows.npy", "residual_history.npy", "solve_status.npy")


def test_dump_outputs_small_and_large(tmp_path):
    """Every row of a small solution; a fixed, seeded sample of DUMP_ROWS rows of a larger one -- float64, within 64 MB."""
    import bench
    x = np.linspace(0.0, 1.0, 1000)
    bench.dump_outputs(str(tmp_path / "small"), x, np.array([1.0, 0.5, 0.25]), 2, 0.25)
    assert np.array_equal(np.load(tmp_path / "small" / "x.npy"), x)
    assert np.array_equal(np.load(tmp_path / "small" / "x_rows.npy"), np.arange(1000.0))
    assert np.array_equal(np.load(tmp_path / "small" / "solve_status.npy"), [2.0, 0.25])
    big = np.arange(bench.DUMP_ROWS * 4, dtype=np.float64) * 0.5
    for d in ("big1", "big2"):
        bench.dump_outputs(str(tmp_path / d), big, np.ones(3), 1, 1.0)
    rows = np.load(tmp_path / "big1" / "x_rows.npy")
    assert rows.shape == (bench.DUMP_ROWS,) and np.all(np.diff(rows) > 0) and rows[-1] < big.size
    assert np.array_equal(np.load(tmp_path / "big1" / "x.npy"), big[rows.astype(np.int64)])
    for name in DUMPED:
        a, b = np.load(tmp_path / "big1" / name), np.load(tmp_path / "big2" / name)
        assert a.dtype == np.float64 and np.array_equal(a, b), name
    assert sum(os.path.getsize(tmp_path / "big1" / name) for name in DUMPED) <= 64e6


def _plain_run(n, steps, warmup, dump):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--n", str(n), "--dump-outputs", dump], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(gpu, tmp_path):
    """P7(64), 3 timed steps after 1 warm-up, twice: the line's steps and ms_per_step, no --full leg, the dumped solution against the
    exact one and the line's iterations / relres, the same files from both runs."""
    n, m = 64, 64 ** 3
    outs = [_plain_run(n, 3, 1, str(tmp_path / d)) for d in ("a", "b")]
    for out in outs:
        assert out["n_gpus"] == 1 and out["steps"] == 3 and out["warmup"] == 1
        assert out["unit"] == "DOF/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
        assert out["ms_per_step"] > 0 and abs(out["value"] - m * 1e3 / out["ms_per_step"]) <= 1e-9 * out["value"]
        assert out["iterations"] == 9                      # P7(64): the reference's count (tests/golden/p7_scale.npz)
        for key in ("cpu_baseline", "parity_reference", "variable_coefficient", "other_configs"):
            assert key not in out, key
        assert out["ceilings"] is None
    d = tmp_path / "a"
    assert sum(os.path.getsize(d / name) for name in DUMPED) <= 64e6
    x, rows = np.load(d / "x.npy"), np.load(d / "x_rows.npy")
    assert x.dtype == np.float64 and np.array_equal(rows, np.arange(float(m)))
    _ia, _ja, _a, _f, ue = gpu.poisson7pt(n)
    assert np.max(np.abs(x - ue)) < 5e-4                 # second-order discretisation error at h = 1/65
    status = np.load(d / "solve_status.npy")
    assert status[0] == outs[0]["iterations"] and status[1] == outs[0]["relres"]
    hist = np.load(d / "residual_history.npy")
    assert hist.dtype == np.float64 and len(hist) >= outs[0]["iterations"]
    for name in DUMPED:
        assert np.array_equal(np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)), name
