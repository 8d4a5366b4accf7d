#!/usr/bin/env python3
"""Time ba_covariance against the host route a user had before it.

  python tools/cov_bench.py --config c3      --out profiles/cov_bench_c3.json
  python tools/cov_bench.py --config c4shard --out profiles/cov_bench_c4shard.json
  python tools/cov_bench.py --iterative --config c3 --config c4 --out profiles/cov_iter_bench.json

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

--iterative times ba_covariance_iterative instead, per config (medians of
--reps runs after --warmup, HIP events unless noted; --request-reps /
--request-warmup set the runs of the request legs, whose calls take seconds
at C4, and --no-forced-b drops the legs with B forced):
  matvec    one implicit matvec: the single-vector launch_pcg_matvec of
            ITERATIVE_SCHUR ("single") against the multi-column one with B = 1,
            2, 4 column cameras (6, 12, 24 columns) on the same W records
  one_column_camera   one diagonal camera block end to end (one column camera,
            B = 1): wall time and the call's four phase times
  request   16 camera blocks + 64 points: ba_covariance_iterative (default B,
            and B forced to 1, 2, 4) against ba_covariance for the same request
            (wall time), and their largest disagreement
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

CONFIGS = {"c3": ("c3", 1.0), "c4shard": ("c4", 0.125), "c4": ("c4", 1.0)}


def median(v):
    return float(np.median(np.asarray(v, float)))


def iterative_record(config, reps, warmup, request_reps, request_warmup, forced_b):
    """The --iterative measurements of one config (a progress line per stage)."""
    def say(*a):
        print(f"[{config} {time.strftime('%H:%M:%S')}]", *a, flush=True)
    name, scale = CONFIGS[config]
    say("building the problem")
    p = fix_camera(make_config(name, scale=scale), 1)
    rec = {"config": config, "n_cams": p.n_cams, "n_pts": p.n_pts, "n_obs": p.n_obs, "reps": reps, "warmup": warmup,
           "request_reps": request_reps, "request_warmup": request_warmup}
    rng = np.random.default_rng(1)
    cams = np.sort(rng.choice(np.arange(2, p.n_cams), size=16, replace=False))
    pairs = np.stack([cams, cams], 1).astype(np.int32)
    seen = np.flatnonzero(np.bincount(p.obs_pt, minlength=p.n_pts) > 0)
    points = np.sort(rng.choice(seen, size=64, replace=False)).astype(np.int32)

    def timed(fn, reps=reps, warmup=warmup):
        for _ in range(warmup):
            fn()
        wall, infos = [], []
        for _ in range(reps):
            t = time.perf_counter()
            out = fn()
            wall.append((time.perf_counter() - t) * 1e3)
            infos.append(out[2]["ms"] if len(out) > 2 else None)
        r = {"wall_ms": median(wall)}
        if infos[0] is not None:
            ph = np.median(np.asarray(infos), axis=0)
            r.update(device_ms_setup=float(ph[0]), device_ms_cg=float(ph[1]),
                     device_ms_residual_check_and_gathers=float(ph[2]), device_ms_copies=float(ph[3]),
                     **{k: out[2][k] for k in ("n_columns", "n_converged", "max_iterations_used", "max_residual")})
        return r, out
    with Solver(0) as s:
        s.set_problem(p)
        say("set_problem done")
        rec["matvec_ms"] = {}
        for c in (0, 1, 2, 4):
            rec["matvec_ms"]["single" if c == 0 else f"B{c}"] = median(s.covariance_iterative_bench(c, reps, warmup))
            say("matvec", rec["matvec_ms"])
        rec["one_column_camera"], _ = timed(lambda: s.covariance_iterative(pairs[:1], None))
        say("one column camera", rec["one_column_camera"])
        req = {}
        rr = dict(reps=request_reps, warmup=request_warmup)
        req["iterative"], it_out = timed(lambda: s.covariance_iterative(pairs, points), **rr)
        say("request, iterative", req["iterative"])
        for b in ("1", "2", "4") if forced_b else ():
            os.environ["BA_COV_PCG_COLS"] = b
            req[f"iterative_B{b}"], _ = timed(lambda: s.covariance_iterative(pairs, points), **rr)
            say(f"request, iterative, B = {b}", req[f"iterative_B{b}"])
        os.environ.pop("BA_COV_PCG_COLS", None)
        req["dense"], d_out = timed(lambda: s.covariance(pairs, points), **rr)
        say("request, dense", req["dense"])
        dc = np.sqrt(np.einsum("kii->ki", d_out[0]))
        dp = np.sqrt(np.einsum("kii->ki", d_out[1]))
        req["max_disagreement_cameras"] = float((np.abs(it_out[0] - d_out[0]) / (dc[:, :, None] * dc[:, None, :])).max())
        req["max_disagreement_points"] = float((np.abs(it_out[1] - d_out[1]) / (dp[:, :, None] * dp[:, None, :])).max())
        rec["request_16_cameras_64_points"] = req
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), required=True, action="append")
    ap.add_argument("--out", required=True)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iterative", action="store_true", help="time ba_covariance_iterative (see the module text)")
    ap.add_argument("--request-reps", type=int, default=None, help="--iterative: runs of the request legs (default --reps)")
    ap.add_argument("--request-warmup", type=int, default=None, help="--iterative: their warm-ups (default --warmup)")
    ap.add_argument("--no-forced-b", action="store_true", help="--iterative: skip the request legs with B forced")
    ap.add_argument("--append", action="store_true", help="--iterative: extend the record list already in --out")
    a = ap.parse_args()
    if a.iterative:
        reps = a.reps or 20
        out = Path(a.out)
        recs = json.loads(out.read_text()) if a.append and out.exists() else []
        recs += [iterative_record(c, reps, a.warmup, a.request_reps or reps,
                                  a.warmup if a.request_warmup is None else a.request_warmup, not a.no_forced_b)
                 for c in a.config]
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(recs, indent=1) + "\n")
        print(json.dumps(recs))
        return
    a.config = a.config[-1]
    a.reps = a.reps or 3
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
