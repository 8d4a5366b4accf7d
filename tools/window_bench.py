#!/usr/bin/env python3
"""Latency of local-BA-sized problems: ba_solve_window_batch (the whole LM
loop in one launch) against the general route ba_set_problem + ba_solve +
ba_get_params (what HipBackend::solve does without BA_WINDOW_SOLVER), and the
oracle on the CPU.  Synthetic generators only.  Not bench.py.

  (a) one window: 11 variable + 6 constant cameras, ~2000 points, 5
      observations per point, 30 iterations; C1 the same way
  (b) a batch of such windows: windows per second, time per LM iteration
      inside the kernel

Every figure is the median of --reps timed calls after --warmup calls; wall
time (host clock around the blocking call) with the kernel's device time
(HIP events) beside it.  Writes one JSON record (default
profiles/window_bench.json) and prints it.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

from bundleadjustment_amd import Options, Solver, make_config, make_synthetic, pack_window_batch  # noqa: E402
from bundleadjustment_amd.problem import fix_camera  # noqa: E402


def local_window(seed: int, n_pts: int = 2000):
    """The reference's local BA: current frame + 10 covisible frames variable,
    6 further observers constant (Optimizer.cpp:500-698)."""
    p = make_synthetic(17, n_pts, 5, seed=seed)
    for c in range(1, 6):
        fix_camera(p, c)
    return p


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(t), min(t), max(t)


def time_window(s, probs, opts, reps, warmup):
    b = pack_window_batch(probs)
    kern = []
    state = {}

    def call():
        state["res"] = s.solve_window_batch(b, opts)
        kern.append(s.window_times())
    wall = median_ms(call, reps, warmup)
    k = np.array(kern[warmup:])
    out, summs = state["res"]
    its = [x.num_iterations for x in summs]
    return {"wall_ms": wall[0], "wall_ms_min": wall[1], "wall_ms_max": wall[2],
            "host_prep_ms": float(np.median(k[:, 0])), "kernel_ms": float(np.median(k[:, 1])),
            "iterations_mean": float(np.mean(its)), "iterations_max": int(max(its)),
            "kernel_ms_per_iteration": float(np.median(k[:, 1]) / max(max(its), 1)),
            "final_cost_0": summs[0].final_cost, "termination_0": summs[0].termination_type}


def time_general(s, p, opts, reps, warmup):
    p = p.normalized()
    state = {}

    def call():
        s.set_problem(p)
        state["summ"] = s.solve(opts)
        state["params"] = s.params()
    wall = median_ms(call, reps, warmup)
    summ = state["summ"]
    return {"wall_ms": wall[0], "wall_ms_min": wall[1], "wall_ms_max": wall[2],
            "iterations": summ.num_iterations, "final_cost": summ.final_cost, "termination": summ.termination_type,
            "solve_only_wall_ms": 1e3 * summ.total_time_s}


def time_oracle(p, iters, threads, reps):
    import oracle
    oracle.set_threads(threads)
    oo = oracle.default_options(max_num_iterations=iters)
    oracle.solve(p, oo)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        oracle.solve(p, oo)
        t.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(t)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "window_bench.json"))
    ap.add_argument("--no-oracle", action="store_true")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: at least 20 timed calls")
    opts = Options(max_num_iterations=a.iters)
    win = local_window(0xBA5E0900, a.points)
    c1 = make_config("c1")
    rec = {"reps": a.reps, "warmup": a.warmup, "iterations_cap": a.iters,
           "window": {"cams": win.n_cams, "variable_cams": int((win.cam_fixed == 0).sum()), "points": win.n_pts,
                      "observations": win.n_obs},
           "c1": {"cams": c1.n_cams, "points": c1.n_pts, "observations": c1.n_obs}}
    with Solver(0) as s:
        rec["window"]["window_batch"] = time_window(s, [win], opts, a.reps, a.warmup)
        rec["window"]["general"] = time_general(s, win, opts, a.reps, a.warmup)
        rec["c1"]["window_batch"] = time_window(s, [c1], opts, a.reps, a.warmup)
        rec["c1"]["general"] = time_general(s, c1, opts, a.reps, a.warmup)
        probs = [local_window(0xBA5E0A00 + i, a.points) for i in range(a.batch)]
        b = time_window(s, probs, opts, a.reps, a.warmup)
        b["windows"] = a.batch
        b["windows_per_second_wall"] = a.batch / (1e-3 * b["wall_ms"])
        b["windows_per_second_kernel"] = a.batch / (1e-3 * b["kernel_ms"])
        rec["batch"] = b
    for k in ("window", "c1"):
        g, w = rec[k]["general"], rec[k]["window_batch"]
        rec[k]["speedup_wall"] = g["wall_ms"] / w["wall_ms"]
    if not a.no_oracle:
        rec["window"]["oracle_ms"] = {str(t): time_oracle(win, a.iters, t, 5) for t in (4, 16)}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
