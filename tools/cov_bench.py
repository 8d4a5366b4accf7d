#!/usr/bin/env python3
"""Time ba_covariance against the host route a user had before it.

  python tools/cov_bench.py --config c3      --out profiles/cov_bench_c3.json
  python tools/cov_bench.py --config c4shard --out profiles/cov_bench_c4shard.json

(on the GPU box through tools/gpu_run.sh: step cov:c3 / cov:c4shard, which
gives the run its time limit).  The problem is the BASELINE config with
camera 1 made constant as well (two anchored cameras: no gauge freedom).

Reported, one JSON record:
  feature   ba_covariance with every diagonal camera block and every observed
            point: host wall time of the blocking call and the device time of
            its phases (ba_covariance_times) - linearisation + reduced system,
            factorisation (the launches of a DENSE_SCHUR step), inverse,
            gathers; the median of --reps calls after one warm-up.  Also the
            same call with the camera blocks only.
  feature_ex  ba_covariance_ex legs, each with its wall time and the four phase
            times: the diagonal camera blocks only; the leverages of all
            observations only; every observed point's cross block with its
            first observing camera only; all of these and the point marginals
            in one call.  A leg minus the cameras-only leg isolates its pass.
  host      the route without it, cameras only (it cannot produce the points):
            ba_debug_blocks at an infinite radius (the undamped S to the
            host), then LAPACK potrf + potri on the host's threads, then the
            Jacobi scaling.  The scale factors are taken from the feature's
            result (a user of the route would have to recompute them from J).
  agreement the largest |feature - host| / sqrt(v_i v_j) over the diagonal
            camera blocks.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from bundleadjustment_amd import Solver, make_config   # noqa: E402
from bundleadjustment_amd.problem import fix_camera    # noqa: E402

CONFIGS = {"c3": ("c3", 1.0), "c4shard": ("c4", 0.125)}


def median(v):
    return float(np.median(np.asarray(v, float)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import scipy.linalg

    name, scale = CONFIGS[a.config]
    p = fix_camera(make_config(name, scale=scale), 1)
    seen = np.bincount(p.obs_pt, minlength=p.n_pts) > 0
    points = np.flatnonzero(seen).astype(np.int32)
    rec = {"config": a.config, "n_cams": p.n_cams, "n_pts": p.n_pts, "n_obs": p.n_obs, "points_requested": int(points.size),
           "host_threads": os.environ.get("OMP_NUM_THREADS")}
    with Solver(0) as s:
        s.set_problem(p)
        cam_cov, _ = s.covariance(None, points)          # warm-up (allocations, first launches)
        wall, phases, wall_c = [], [], []
        for _ in range(a.reps):
            t = time.perf_counter()
            cam_cov, pt_cov = s.covariance(None, points)
            wall.append((time.perf_counter() - t) * 1e3)
            phases.append(s.covariance_times())
            t = time.perf_counter()
            s.covariance(None, None)
            wall_c.append((time.perf_counter() - t) * 1e3)
        ph = np.median(np.stack(phases), axis=0)
        rec["feature"] = {"wall_ms": median(wall), "device_ms": float(ph.sum()),
                          "device_ms_linearise_and_reduced_system": float(ph[0]), "device_ms_factorisation": float(ph[1]),
                          "device_ms_inverse": float(ph[2]), "device_ms_gathers": float(ph[3]),
                          "wall_ms_cameras_only": median(wall_c)}
        # ba_covariance_ex legs; the new pass alone is a leg minus "cameras_only"
        first = np.full(p.n_pts, -1, np.int64)
        u, i = np.unique(p.obs_pt, return_index=True)        # each point's first observing camera
        first[u] = p.obs_cam[i]
        cam_pt = np.stack([first[points], points], 1).astype(np.int32)
        diag = np.stack([np.arange(p.n_cams)] * 2, 1).astype(np.int32)
        legs = {"cameras_only": dict(cam_pairs=diag),
                "all_leverages": dict(leverage_obs="all"),
                "cross_block_per_point": dict(cam_pt=cam_pt),
                "cameras_points_cross_leverages": dict(cam_pairs=diag, points=points, cam_pt=cam_pt,
                                                       leverage_obs="all")}
        rec["feature_ex"] = {"leverages_requested": p.n_obs, "cross_blocks_requested": int(cam_pt.shape[0])}
        for leg, kw in legs.items():
            s.covariance_ex(**kw)                            # warm-up (the J records' first allocation)
            wall, phases = [], []
            for _ in range(a.reps):
                t = time.perf_counter()
                out = s.covariance_ex(**kw)
                wall.append((time.perf_counter() - t) * 1e3)
                phases.append(s.covariance_times())
            ph = np.median(np.stack(phases), axis=0)
            rec["feature_ex"][leg] = {"wall_ms": median(wall), "device_ms": float(ph.sum()),
                                      "device_ms_linearise_and_reduced_system": float(ph[0]),
                                      "device_ms_factorisation": float(ph[1]), "device_ms_inverse": float(ph[2]),
                                      "device_ms_gathers": float(ph[3])}
            if "leverages" in leg:   # (their traces sum to n_variable_parameters)
                lev = out["leverage"]
                rec["feature_ex"][leg]["trace_sum"] = float(np.einsum("oii->", lev))
                rec["feature_ex"][leg]["max_leverage_entry"] = float(lev.max())
        var_c = (p.cam_fixed == 0) & (np.bincount(p.obs_cam, minlength=p.n_cams) > 0)
        pt_fixed = np.zeros(p.n_pts, bool) if p.pt_fixed is None else p.pt_fixed != 0
        rec["n_variable_parameters"] = 6 * int(var_c.sum()) + 3 * int((seen & ~pt_fixed).sum())
        # host route: S at an infinite radius to the host, potrf + potri there
        n = C.c_int(0)
        s._check(s.lib.ba_debug_blocks(s.h, float("inf"), None, None, None, None, None, None, C.byref(n)), "sizing")
        n = n.value
        rec["n"] = n
        t_blocks, t_lapack = [], []
        for _ in range(a.reps):
            S = np.empty((n, n))
            rhs = np.empty(n)
            t = time.perf_counter()
            s._check(s.lib.ba_debug_blocks(s.h, float("inf"), None, None, None, None, S.ctypes.data_as(C.c_void_p),
                                           rhs.ctypes.data_as(C.c_void_p), None), "ba_debug_blocks")
            t_blocks.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            c, info = scipy.linalg.lapack.dpotrf(S, lower=1, overwrite_a=1)
            assert info == 0, info
            inv, info = scipy.linalg.lapack.dpotri(c, lower=1, overwrite_c=1)
            assert info == 0, info
            t_lapack.append((time.perf_counter() - t) * 1e3)
        rec["host"] = {"debug_blocks_ms": median(t_blocks), "potrf_potri_ms": median(t_lapack),
                       "total_ms": median(t_blocks) + median(t_lapack)}
    # agreement on the diagonal camera blocks: inv is the scaled inverse; the
    # ratio to the feature's variances gives the scale factors back
    var = np.flatnonzero((p.cam_fixed == 0) & (np.bincount(p.obs_cam, minlength=p.n_cams) > 0))
    worst = 0.0
    for k, c in enumerate(var):
        blk = np.tril(inv[6 * k:6 * k + 6, 6 * k:6 * k + 6])
        blk = blk + np.tril(blk, -1).T
        sc = np.sqrt(np.diag(cam_cov[c]) / np.diag(blk))
        got = blk * np.outer(sc, sc)
        d = np.sqrt(np.diag(cam_cov[c]))
        worst = max(worst, float((np.abs(got - cam_cov[c]) / np.outer(d, d)).max()))
    rec["agreement_diag_blocks"] = worst
    rec["feature_beats_host_cameras_only"] = rec["feature"]["wall_ms_cameras_only"] < rec["host"]["total_ms"]
    rec["feature_with_points_beats_host_cameras_only"] = rec["feature"]["wall_ms"] < rec["host"]["total_ms"]
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
