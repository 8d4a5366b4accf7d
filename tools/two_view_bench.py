#!/usr/bin/env python3
"""Time of ba_two_view_ransac (E and H RANSAC on the device, model choice,
decomposition, depth vote).  Synthetic scenes only.  Not bench.py.

  shapes: one pair of --matches matches x --hypotheses hypotheses, and
          --pairs such pairs in one call (half general scenes, half planar)

Every figure is the median of --reps timed calls after --warmup calls: wall
time (host clock around the blocking call) and the kernels' device time (HIP
events) beside it, then picoseconds per (hypothesis x match), where one unit
is both models' predicates on one match.  The numbers are reported, not
gated.  --e-solver picks the essential solver: eight (the default) or five
(the five-point solver, every real root scored; a unit is then still one
hypothesis x match, whatever the number of roots).  Each shape runs in a child process of its own under `timeout -k 10`;
the first shape that fails ends the run.  Writes one JSON record (default
profiles/two_view_bench.json) and prints it.
"""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

FX, FY, CX, CY = 525.0, 525.0, 319.5, 239.5


def pair(n, outlier_frac, noise_px, planar, rng):
    """One pair: a small rotation, baseline 0.5; n points at depths 2 .. 8 or on
    the plane z = 5 + 0.1 x + 0.05 y; noise; a fraction displaced by 30 .. 120
    px in image 2."""
    from bundleadjustment_amd.problem import angle_axis_to_rotation
    Km = np.array([[FX, 0.0, CX], [0.0, FY, CY], [0.0, 0.0, 1.0]])
    R = angle_axis_to_rotation(0.08 * rng.normal(size=3))
    t = np.array([1.0, 0.0, 0.0]) + 0.3 * rng.normal(size=3)
    t *= 0.5 / np.linalg.norm(t)
    if planar:
        xy = np.stack([rng.uniform(-2.4, 2.4, n), rng.uniform(-1.8, 1.8, n)], 1)
        X = np.column_stack([xy, 5.0 + 0.1 * xy[:, 0] + 0.05 * xy[:, 1]])
    else:
        px = np.stack([rng.uniform(40.0, 600.0, n), rng.uniform(40.0, 440.0, n)], 1)
        X = np.column_stack([(px[:, 0] - CX) / FX, (px[:, 1] - CY) / FY, np.ones(n)]) * rng.uniform(2.0, 8.0, n)[:, None]
    p1, p2 = X @ Km.T, (X @ R.T + t) @ Km.T
    uv1 = p1[:, :2] / p1[:, 2:] + noise_px * rng.normal(size=(n, 2))
    uv2 = p2[:, :2] / p2[:, 2:] + noise_px * rng.normal(size=(n, 2))
    idx = rng.choice(n, int(round(outlier_frac * n)), replace=False)
    ang, r = rng.uniform(0.0, 2.0 * np.pi, len(idx)), rng.uniform(30.0, 120.0, len(idx))
    uv2[idx] += np.stack([r * np.cos(ang), r * np.sin(ang)], 1)
    return R, t / np.linalg.norm(t), uv1.astype(np.float32), uv2.astype(np.float32)


def child(a, pairs):
    from bundleadjustment_amd import Solver
    from bundleadjustment_amd import _native as N
    from bundleadjustment_amd.problem import K_colmajor, angle_axis_to_rotation, rotation_to_angle_axis
    rng = np.random.default_rng(0xBA5E0D00 + pairs)
    sc = [pair(a.matches, a.outliers, 0.3, bool(i & 1), rng) for i in range(pairs)]
    off = (np.arange(pairs + 1) * a.matches).astype(np.int32)
    K = np.tile(K_colmajor(FX, FY, CX, CY).astype(np.float32), (pairs, 1))
    uv1, uv2 = np.concatenate([s[2] for s in sc]), np.concatenate([s[3] for s in sc])
    wall, kern = [], []
    with Solver(0) as s:
        for it in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            inl, res = s.two_view_ransac(off, K, None, uv1, uv2, max_hypotheses=a.hypotheses,
                                         e_solver=N.TV_E_FIVE_POINT if a.e_solver == "five" else N.TV_E_EIGHT_POINT)
            if it >= a.warmup:
                wall.append(1e3 * (time.perf_counter() - t0))
                kern.append(s.two_view_times())
    k = np.array(kern)
    rot = [float(np.linalg.norm(rotation_to_angle_axis((angle_axis_to_rotation(r.cam[:3]) @ sc[i][0].T)[None])[0]))
           for i, r in enumerate(res) if r.status == N.TV_OK]
    units = pairs * a.hypotheses * a.matches
    # the census of section 21.4: the share of the E winner's votes that its essential projection keeps
    kept = [r.n_inliers / r.votes_e for r in res if r.status == N.TV_OK and r.model == N.TV_ESSENTIAL and r.votes_e > 0]
    general_as_h = sum(r.model == N.TV_HOMOGRAPHY for i, r in enumerate(res) if not i & 1)
    rec = {"pairs": pairs, "e_solver": a.e_solver, "matches": a.matches, "hypotheses": a.hypotheses, "outlier_fraction": a.outliers,
           "wall_ms": statistics.median(wall), "wall_ms_min": min(wall), "wall_ms_max": max(wall),
           "host_prep_ms": float(np.median(k[:, 0])), "kernel_ms": float(np.median(k[:, 1])),
           "wall_ps_per_hypothesis_match": 1e9 * statistics.median(wall) / units,
           "kernel_ps_per_hypothesis_match": 1e9 * float(np.median(k[:, 1])) / units,
           "status_counts": {N.TV_STATUS_NAMES[i]: int(c)
                             for i, c in enumerate(np.bincount([r.status for r in res], minlength=4))},
           "model_counts": {"ESSENTIAL": sum(r.model == N.TV_ESSENTIAL for r in res),
                            "HOMOGRAPHY": sum(r.model == N.TV_HOMOGRAPHY for r in res)},
           "expected_models": {"ESSENTIAL": (pairs + 1) // 2, "HOMOGRAPHY": pairs // 2},
           "general_scenes_scored_as_homographies": int(general_as_h),
           "votes_kept_by_projection": {"pairs": len(kept), "min": min(kept) if kept else None,
                                        "mean": float(np.mean(kept)) if kept else None},
           "inliers_mean": float(np.mean([r.n_inliers for r in res])),
           "rotation_error_rad_max": max(rot) if rot else None}
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--matches", type=int, default=1000)
    ap.add_argument("--hypotheses", type=int, default=1000)
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--outliers", type=float, default=0.3)
    ap.add_argument("--e-solver", choices=("eight", "five"), default="eight")
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds per shape")
    ap.add_argument("--tree", default="", help="a label of the source tree, recorded as given")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "two_view_bench.json"))
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a, a.child)
        return 0
    rec = {"date": time.strftime("%Y-%m-%d"), "tree": a.tree, "e_solver": a.e_solver, "reps": a.reps, "warmup": a.warmup,
           "pnp_kernel_ps_per_hypothesis_point": {"one_frame": 116.0, "many_frames": 7.8}}
    rc = 0
    for name, pairs in (("one_pair", 1), ("many_pairs", a.pairs)):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, __file__, "--child", str(pairs),
               "--reps", str(a.reps), "--warmup", str(a.warmup), "--matches", str(a.matches),
               "--hypotheses", str(a.hypotheses), "--outliers", str(a.outliers), "--e-solver", a.e_solver]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:      # a fault, an abort or the time limit: nothing more is started
            rec[name] = {"exit_status": p.returncode, "stderr_tail": p.stderr[-2000:]}
            rc = p.returncode
            break
        rec[name] = json.loads(p.stdout.strip().splitlines()[-1])
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))
    return rc


if __name__ == "__main__":
    sys.exit(main())
