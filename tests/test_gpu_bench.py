"""bench.py on the GPU: a plain run times its steps and prints the headline
line only; --dump-outputs writes what the last timed LM step computed, the
same from run to run; --full adds the roofline record."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

SMALL = ["--gpus", "1", "--scale", "0.02", "--steps", "2", "--warmup", "1"]   # C3 at 2000 points, 20k observations


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, str(ROOT / "bench.py")] + SMALL + args, capture_output=True, text=True,
                         timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [x for x in out.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain_runs(tmp_path_factory):
    """Two plain runs with the same arguments, each dumping its outputs."""
    dirs = [tmp_path_factory.mktemp(f"bench_out{i}") for i in range(2)]
    return [(_bench(["--dump-outputs", str(d)]), d) for d in dirs]


@pytest.mark.gpu
def test_plain_run_reports_the_headline_only(plain_runs):
    d, _ = plain_runs[0]
    assert d["metric"] == "M-obs/s per LM iteration (residual+Jacobian+Schur)" and d["unit"] == "M-obs/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f64" and d["n_gpus"] == 1
    assert d["steps"] == 2 and d["warmup"] == 1 and d["full"] is False
    assert d["ms_per_step"] > 0
    assert abs(d["value"] - d["config"]["global_obs"] / (d["ms_per_step"] * 1e-3) / 1e6) <= 0.01 * d["value"]
    assert d["roofline"] is None and d["cpu_baseline"] is None     # runs of their own: --full


@pytest.mark.gpu
def test_dumped_outputs_are_the_step_and_repeat(plain_runs):
    from bundleadjustment_amd import Options, Solver, make_config
    (_, a), (_, b) = plain_runs
    got = {f.stem: np.load(f) for f in sorted(a.glob("*.npy"))}
    assert sorted(got) == ["cams", "iterations", "pts", "pts_rows"]
    for name, arr in got.items():
        assert arr.dtype == np.float64 and np.all(np.isfinite(arr))
        assert np.array_equal(arr, np.load(b / f"{name}.npy")), name        # same inputs, fixed-order reductions
    # one LM step of the benchmark's problem from x0, as a caller of the library takes it
    p = make_config("c3", scale=0.02)
    with Solver(0) as s:
        s.set_problem(p)
        s.solve(Options(max_num_iterations=1, function_tolerance=0.0, gradient_tolerance=0.0,
                        parameter_tolerance=0.0))
        cams, pts = s.params()
        log = s.iteration_log()
    assert got["cams"].shape == (p.n_cams, 6) and got["pts"].shape == (p.n_pts, 3)
    assert np.array_equal(got["pts_rows"], np.arange(p.n_pts))
    assert np.array_equal(got["cams"], cams) and np.array_equal(got["pts"], pts)
    assert got["iterations"].shape == (2, 12)
    assert got["iterations"][:, 4].tolist() == [r["cost"] for r in log]
    assert log[1]["step_is_successful"] == 1 and not np.array_equal(cams, s.problem.cams)   # the step moved x


@pytest.mark.gpu
def test_full_adds_the_roofline_record():
    d = _bench(["--full", "--no-cpu-baseline"])
    assert d["full"] is True and d["steps"] == 2 and d["cpu_baseline"] is None
    r = d["roofline"]
    assert r["avg_launch_ms"] > 0 and r["measured_copy"] > 0 and r["achieved"] > 0
