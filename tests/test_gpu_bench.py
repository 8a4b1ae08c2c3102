"""bench.py end to end on a small grid: a plain run (the timed steps only, their outputs written with
--dump-outputs) and a --full run (true-residual check, per-phase timing).  Each is started once and shared."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID, STEPS, WARMUP = 256, 20, 4  # 1024 SELL slices: several blocks; 24 iterations, short of one 32-iteration graph


def _bench(extra):
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--grid", str(GRID), "--steps", str(STEPS), "--warmup",
                        str(WARMUP)] + extra, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout  # one JSON line on stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    return _bench(["--dump-outputs", str(d)]), d


@pytest.fixture(scope="module")
def full():
    return _bench(["--full"])


def test_plain_run_result_line(plain):
    """--steps sets the timed iterations (the device-side counter agrees), ms_per_step is one timed step,
    and nothing beyond the headline figure ran: no true-residual figures, no phase timing."""
    line, _ = plain
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["n_gpus"] == 1
    assert line["unit"] == "iterations/s" and line["higher_is_better"] is True and line["dtype"] == "fp64"
    assert line["check"]["ok"] and line["check"]["device_iterations"] == STEPS + WARMUP
    assert line["ms_per_step"] > 0 and line["value"] * line["ms_per_step"] * 1e-3 == pytest.approx(1.0, rel=1e-3)
    assert not [k for k in line["check"] if k.startswith("true_") or k.startswith("phase_us")], line["check"]


def test_dump_outputs_are_the_timed_path_results(mcg, plain):
    """x.npy / rnorm.npy hold the solution and the recurrence residual after the last timed step: the
    CPU reference recurrence run for the same warmup + steps iterations on the same seeded system gives
    them to rounding (different summation order over 24 iterations of a system with condition number
    ~3e4: far below 1e-9 of the largest entry)."""
    line, d = plain
    assert sorted(os.listdir(d)) == ["rnorm.npy", "x.npy"]
    x, rnorm = np.load(d / "x.npy"), np.load(d / "rnorm.npy")
    assert x.dtype == np.float64 and x.shape == (GRID * GRID,) and rnorm.dtype == np.float64 and rnorm.shape == (1,)
    assert rnorm[0] == line["check"]["rnorm"]
    spec = mcg.make_problem("poisson2d", n=GRID, rhs="random")
    cpu = mcg.native().cpu_cg(spec.native(), mcg.native().CgOptions(maxit=STEPS + WARMUP, tol=1e-30))
    assert cpu["iterations"] == STEPS + WARMUP
    np.testing.assert_allclose(x, cpu["x"], rtol=0, atol=1e-9 * np.abs(cpu["x"]).max())
    assert abs(rnorm[0] - cpu["rnorm"]) <= 1e-9 * cpu["rnorm"]


def test_full_run_adds_the_checks(plain, full):
    """--full: the true residual tracks the recurrence's, the phase iterations run after the timed ones
    (and are counted), and the timed path is the plain run's."""
    assert full["check"]["ok"] and full["check"]["true_gap_rel"] <= 1e-8, full["check"]
    assert full["check"]["phase_us"]["iteration"] > 0
    assert full["check"]["device_iterations"] == STEPS + WARMUP + 10
    assert full["config"] == plain[0]["config"] and full["metric"] == plain[0]["metric"]
