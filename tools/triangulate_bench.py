#!/usr/bin/env python3
"""Throughput of ba_triangulate (batched DLT + per-point LM + acceptance tests
in one launch) against the two routes that existed before it.  Synthetic
generators only.  Not bench.py.

  (a) the reference's case: 2 cameras x 100k two-view points, DLT + tests
  (b) C3's structure with every camera constant (200 cameras x 100k points x
      10 views): DLT + tests, and DLT + refine + tests
  baselines, same session, same iteration cap:
      one-point windows through ba_solve_window_batch (a subset of the
      points, scaled per point; each window holds only the cameras that
      observe its point, the cheapest form of that route), started at the
      DLT points: the same semantics as the refinement;
      ba_set_problem + ba_solve + ba_get_params on the joint problem with
      every camera constant: DIFFERENT semantics (one trust region and one
      accept / reject decision for all points), recorded for scale only.

Every figure is the median of --reps timed calls after --warmup calls; wall
time (host clock around the blocking call) with the kernels' device time (HIP
events) beside it.  Writes one JSON record (default
profiles/triangulate_bench.json) and prints it.
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

from bundleadjustment_amd import (Options, Problem, Solver, make_config, make_synthetic, pack_window_batch,  # noqa: E402
                                  triangulation_batch)
from bundleadjustment_amd import _native as N  # noqa: E402
from bundleadjustment_amd.problem import fix_camera  # noqa: E402


def all_fixed(p):
    for c in range(p.n_cams):
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


def time_triangulate(s, b, opts, reps, warmup, refine):
    kern, state = [], {}

    def call():
        state["res"] = s.triangulate(b.extr, b.K, b.obs_offset, b.obs_cam, b.obs_uv, cam_center=b.cam_center,
                                     refine=refine, options=opts, huber_a=b.huber_a, with_summaries=False)
        kern.append(s.triangulate_times())
    wall = median_ms(call, reps, warmup)
    k = np.array(kern[warmup:])
    pts, status, _ = state["res"]
    n = len(status)
    rec = {"points": n, "observations": int(b.obs_offset[-1]), "refine": bool(refine),
           "wall_ms": wall[0], "wall_ms_min": wall[1], "wall_ms_max": wall[2],
           "host_prep_ms": float(np.median(k[:, 0])), "kernel_ms": float(np.median(k[:, 1])),
           "wall_us_per_point": 1e3 * wall[0] / n, "kernel_us_per_point": 1e3 * float(np.median(k[:, 1])) / n,
           "status_counts": {N.TRI_STATUS_NAMES[i]: int(c) for i, c in enumerate(np.bincount(status, minlength=6))}}
    if refine:   # iteration counts, outside the timed calls
        _, _, summ = s.triangulate(b.extr, b.K, b.obs_offset, b.obs_cam, b.obs_uv, cam_center=b.cam_center, refine=True,
                                   options=opts, huber_a=b.huber_a, with_summaries=True)
        its = np.array([x.num_iterations for x in summ])
        rec["iterations_mean"] = float(its.mean())
        rec["iterations_max"] = int(its.max())
    return rec, pts


def one_point_windows(b, X0, idx):
    """Point q as a window of its own: only the cameras that observe it, all
    constant, one variable point at X0[q]."""
    out = []
    for q in idx:
        a0, a1 = int(b.obs_offset[q]), int(b.obs_offset[q + 1])
        cams, loc = np.unique(b.obs_cam[a0:a1], return_inverse=True)
        out.append(Problem(cams=np.zeros((len(cams), 6)), K=b.K[cams], pts=X0[q].reshape(1, 3).copy(),
                           obs_cam=loc.astype(np.int32), obs_pt=np.zeros(a1 - a0, np.int32), obs_uv=b.obs_uv[a0:a1],
                           cam_fixed=np.ones(len(cams), np.uint8), cam_fixed_extr=b.extr[cams],
                           huber_a=b.huber_a))
    return out


def time_windows(s, probs, opts, reps, warmup):
    wb = pack_window_batch(probs)
    kern, state = [], {}

    def call():
        state["res"] = s.solve_window_batch(wb, opts)
        kern.append(s.window_times())
    wall = median_ms(call, reps, warmup)
    k = np.array(kern[warmup:])
    n = len(probs)
    its = np.array([x.num_iterations for x in state["res"][1]])
    return {"semantics": "same as the refinement (one LM per point)", "points": n,
            "wall_ms": wall[0], "wall_ms_min": wall[1], "wall_ms_max": wall[2],
            "host_prep_ms": float(np.median(k[:, 0])), "kernel_ms": float(np.median(k[:, 1])),
            "wall_us_per_point": 1e3 * wall[0] / n, "kernel_us_per_point": 1e3 * float(np.median(k[:, 1])) / n,
            "iterations_mean": float(its.mean()), "iterations_max": int(its.max())}


def time_joint(s, p, X0, opts, reps, warmup):
    q = p.copy()
    q.pts = X0.copy()
    q = q.normalized()
    state = {}

    def call():
        s.set_problem(q)
        state["summ"] = s.solve(opts)
        state["params"] = s.params()
    wall = median_ms(call, reps, warmup)
    summ = state["summ"]
    return {"semantics": "DIFFERENT: one joint LM over all points (one trust region, one accept/reject)",
            "points": q.n_pts, "wall_ms": wall[0], "wall_ms_min": wall[1], "wall_ms_max": wall[2],
            "wall_us_per_point": 1e3 * wall[0] / q.n_pts, "iterations": summ.num_iterations,
            "termination": summ.termination_type}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--window-points", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "triangulate_bench.json"))
    a = ap.parse_args()
    opts = Options(max_num_iterations=a.iters)
    two = all_fixed(make_synthetic(2, a.points, 2, seed=0xBA5E0B00, perturb=None, anchor=False))
    c3 = all_fixed(make_config("c3", scale=a.points / 100_000, perturb=None, anchor=False))
    b2, b3 = triangulation_batch(two), triangulation_batch(c3)
    rec = {"reps": a.reps, "warmup": a.warmup, "iterations_cap": a.iters, "group_lanes": 8}
    with Solver(0) as s:
        rec["two_view"], _ = time_triangulate(s, b2, opts, a.reps, a.warmup, refine=False)
        rec["two_view"]["cams"] = 2
        rec["c3_fixed"] = {"cams": c3.n_cams}
        rec["c3_fixed"]["dlt"], X0 = time_triangulate(s, b3, opts, a.reps, a.warmup, refine=False)
        rec["c3_fixed"]["dlt_refine"], _ = time_triangulate(s, b3, opts, a.reps, a.warmup, refine=True)
        ok = np.flatnonzero((np.diff(b3.obs_offset) >= 2) & np.all(np.isfinite(X0), axis=1))
        idx = ok[:: max(1, len(ok) // a.window_points)][:a.window_points]
        rec["c3_fixed"]["baseline_one_point_windows"] = time_windows(s, one_point_windows(b3, X0, idx), opts, a.reps,
                                                                     a.warmup)
        Xj = np.where(np.isfinite(X0), X0, 0.0)
        rec["c3_fixed"]["baseline_joint_solve"] = time_joint(s, c3, Xj, opts, max(3, a.reps // 4), 1)
    r, w, j = (rec["c3_fixed"][k] for k in ("dlt_refine", "baseline_one_point_windows", "baseline_joint_solve"))
    rec["ratios"] = {
        "one_point_windows_over_refine_wall_per_point": w["wall_us_per_point"] / r["wall_us_per_point"],
        "one_point_windows_over_refine_kernel_per_point": w["kernel_us_per_point"] / r["kernel_us_per_point"],
        "joint_solve_over_refine_wall_per_point_DIFFERENT_SEMANTICS": j["wall_us_per_point"] / r["wall_us_per_point"],
        "refine_takes_at_most_half_of_the_window_route": bool(2.0 * r["wall_us_per_point"] <= w["wall_us_per_point"]),
    }
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
