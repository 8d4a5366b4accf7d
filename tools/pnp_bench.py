#!/usr/bin/env python3
"""Time of ba_pnp_ransac (P3P RANSAC on the device + the pose LM on the
consensus set) beside ba_solve_pose_batch on the same batch, which is the
refinement alone.  Synthetic scenes only.  Not bench.py.

  shapes: one frame of --points points x --hypotheses hypotheses, and
          --frames such frames in one call
  per shape: pnp_ransac with refine (the whole entry), pnp_ransac without
          refine (the RANSAC stage alone: score, select, mask), and
          solve_pose_batch from the prior on all observations with Huber

Every figure is the median of --reps timed calls after --warmup calls: wall
time (host clock around the blocking call) and, for pnp_ransac, the kernels'
device time (HIP events) beside it.  The RANSAC stage is then stated as a
multiple of the pose batch.  Writes one JSON record (default
profiles/pnp_bench.json) and prints it.
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

from bundleadjustment_amd import Options, Solver  # noqa: E402
from bundleadjustment_amd import _native as N  # noqa: E402
from bundleadjustment_amd.problem import K_colmajor, angle_axis_to_rotation  # noqa: E402

FX, FY, CX, CY = 525.0, 525.0, 319.5, 239.5


def frame(n, outlier_frac, noise_px, rng):
    """One frame: a pose, n points seen at uniform pixels and depths 1 .. 6,
    noise, a fraction displaced by 50 .. 150 px."""
    w, t = 0.2 * rng.normal(size=3), 0.3 * rng.normal(size=3)
    R = angle_axis_to_rotation(w)
    px = np.stack([rng.uniform(20.0, 620.0, n), rng.uniform(20.0, 460.0, n)], 1)
    depth = rng.uniform(1.0, 6.0, n)
    pc = np.stack([(px[:, 0] - CX) / FX, (px[:, 1] - CY) / FY, np.ones(n)], 1) * depth[:, None]
    X = (pc - t) @ R
    uv = px + noise_px * rng.normal(size=(n, 2))
    inl = np.ones(n, bool)
    idx = rng.choice(n, int(round(outlier_frac * n)), replace=False)
    ang, r = rng.uniform(0.0, 2.0 * np.pi, len(idx)), rng.uniform(50.0, 150.0, len(idx))
    uv[idx] += np.stack([r * np.cos(ang), r * np.sin(ang)], 1)
    inl[idx] = False
    return np.concatenate([w, t]), X, uv.astype(np.float32), inl


def make_batch(frames, n, outlier_frac, prior_sigma, seed):
    rng = np.random.default_rng(seed)
    fr = [frame(n, outlier_frac, 0.5, rng) for _ in range(frames)]
    off = (np.arange(frames + 1) * n).astype(np.int32)
    truth = np.stack([f[0] for f in fr])
    prior = truth + prior_sigma * rng.normal(size=truth.shape)
    K = np.tile(K_colmajor(FX, FY, CX, CY).astype(np.float32), (frames, 1))
    return (off, prior, K, np.concatenate([f[1] for f in fr]), np.concatenate([f[2] for f in fr])), truth, \
        np.concatenate([f[3] for f in fr])


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(t), min(t), max(t)


def time_pnp(s, b, opts, H, refine, reps, warmup):
    kern, state = [], {}

    def call():
        state["res"] = s.pnp_ransac(*b, options=opts, max_hypotheses=H, refine=int(refine))
        kern.append(s.pnp_times())
    wall = median_ms(call, reps, warmup)
    k = np.array(kern[warmup:])
    cams, inl, res = state["res"]
    rec = {"refine": bool(refine), "wall_ms": wall[0], "wall_ms_min": wall[1], "wall_ms_max": wall[2],
           "host_prep_ms": float(np.median(k[:, 0])), "kernel_ms": float(np.median(k[:, 1])),
           "status_counts": {N.PNP_STATUS_NAMES[i]: int(c)
                             for i, c in enumerate(np.bincount([r.status for r in res], minlength=4))}}
    return rec, cams, inl, res


def time_pose(s, b, opts, reps, warmup):
    state = {}

    def call():
        state["res"] = s.solve_pose_batch(*b, opts)
    wall = median_ms(call, reps, warmup)
    its = np.array([x.num_iterations for x in state["res"][1]])
    return {"wall_ms": wall[0], "wall_ms_min": wall[1], "wall_ms_max": wall[2], "iterations_mean": float(its.mean()),
            "iterations_max": int(its.max())}, state["res"][0]


def shape(s, frames, a, opts):
    b, truth, inl_true = make_batch(frames, a.points, a.outliers, a.prior_sigma, 0xBA5E0C00 + frames)
    rec = {"frames": frames, "points": a.points, "hypotheses": a.hypotheses, "outlier_fraction": a.outliers,
           "prior_sigma": a.prior_sigma}
    rec["pnp_refine"], cams, inl, res = time_pnp(s, b, opts, a.hypotheses, True, a.reps, a.warmup)
    rec["pnp_ransac_only"], _, _, _ = time_pnp(s, b, opts, a.hypotheses, False, a.reps, a.warmup)
    rec["pose_batch"], lm = time_pose(s, b, opts, a.reps, a.warmup)
    rec["pnp_refine"]["max_abs_error_to_truth"] = float(np.max(np.abs(cams - truth)))
    rec["pnp_refine"]["inlier_mask_equals_generator"] = bool(np.array_equal(inl, inl_true))
    rec["pnp_refine"]["lm_iterations_mean"] = float(np.mean([r.refine.num_iterations for r in res]))
    rec["pose_batch"]["max_abs_error_to_truth"] = float(np.max(np.abs(lm - truth)))
    ro, pb = rec["pnp_ransac_only"], rec["pose_batch"]
    evals = frames * a.hypotheses * a.points
    rec["ratios"] = {"ransac_wall_over_pose_batch_wall": ro["wall_ms"] / pb["wall_ms"],
                     "ransac_kernel_over_pose_batch_wall": ro["kernel_ms"] / pb["wall_ms"],
                     "whole_call_wall_over_pose_batch_wall": rec["pnp_refine"]["wall_ms"] / pb["wall_ms"]}
    rec["ransac_kernel_ns_per_hypothesis_point"] = 1e6 * ro["kernel_ms"] / evals
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--hypotheses", type=int, default=1000)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--outliers", type=float, default=0.3)
    ap.add_argument("--prior-sigma", type=float, default=0.02)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--tree", default="", help="a label of the source tree, recorded as given")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pnp_bench.json"))
    a = ap.parse_args()
    opts = Options(max_num_iterations=a.iters)
    rec = {"date": time.strftime("%Y-%m-%d"), "tree": a.tree, "reps": a.reps, "warmup": a.warmup,
           "iterations_cap": a.iters}
    with Solver(0) as s:
        rec["one_frame"] = shape(s, 1, a, opts)
        rec["many_frames"] = shape(s, a.frames, a, opts)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
