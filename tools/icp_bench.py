#!/usr/bin/env python3
"""Time of ba_icp.  Synthetic clouds only (a bumpy closed surface sampled
twice, noisy, the source displaced by 3 degrees / 0.02).  Not bench.py.

  100k_1m    one pair, 100k source points against 1M target points
  10k_100k   one pair, 10k against 100k
  256x2k     256 pairs of 2k against 2k (distinct sets), also under route
             GRID and route BRUTE
  crossover  one pair of 2k source points against 256 .. 16384 target points,
             route GRID and route BRUTE: the figures behind AUTO's threshold

Every figure is the median of --reps timed calls after --warmup calls of the
whole default loop (10 iterations and the fitness pass): kernel_ms is the
device time of the enqueued rounds (HIP events), round_ms that over the 11
rounds, host_prep_ms the checks, the grid build and the source permutation on
the host, wall_ms the host clock around the blocking call (upload included).
cpu_kdtree_ms, where scipy is present, is scipy.spatial.cKDTree on the host
for the same clouds: the build of the target's tree plus eleven
query(workers=16) passes of the initial source: the CPU figure for the same
number of correspondence passes, without the steps.  The numbers are reported,
not gated.  Each shape runs in a child process of its own under `timeout -k
10`; the first shape that fails ends the run.  Writes one JSON record (default
profiles/icp_bench.json) and prints it."""
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

# pairs, source points, target points
SHAPES = {"100k_1m": (1, 100_000, 1_000_000), "10k_100k": (1, 10_000, 100_000), "256x2k": (256, 2000, 2000)}
CROSSOVER = (256, 512, 1024, 2048, 4096, 8192, 16384)


def surface(rng, n):
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    th, ph = np.arccos(v[:, 2]), np.arctan2(v[:, 1], v[:, 0])
    r = 1.0 + 0.15 * np.sin(3 * th) * np.cos(2 * ph) + 0.1 * np.cos(5 * ph) * np.sin(th) ** 2
    return (v * r[:, None]) * np.array([1.0, 0.8, 0.6]) + rng.normal(scale=0.004, size=(n, 3))


def clouds(rng, n_src, n_tgt):
    a = np.deg2rad(3.0)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    src = surface(rng, n_src) @ R.T + np.array([0.02, -0.012, 0.009])
    return src.astype(np.float32), surface(rng, n_tgt).astype(np.float32)


def timed(s, sets, pairs, a, **kw):
    wall, t = [], []
    for it in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        res, _ = s.icp(sets, pairs, **kw)
        if it >= a.warmup:
            wall.append(1e3 * (time.perf_counter() - t0))
            t.append(s.icp_times())
    t = np.array(t)
    return {"wall_ms": statistics.median(wall), "wall_ms_min": min(wall), "wall_ms_max": max(wall),
            "host_prep_ms": float(np.median(t[:, 0])), "kernel_ms": float(np.median(t[:, 1])),
            "kernel_ms_min": float(t[:, 1].min()), "kernel_ms_max": float(t[:, 1].max()),
            "round_ms": float(np.median(t[:, 3])), "iterations": int(res["iterations"].max()),
            "fitness": float(res["fitness"][0])}


def cpu_kdtree_ms(sets, pairs, passes=11):
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return None
    t0 = time.perf_counter()
    trees = {}
    for s, t in pairs:
        if t not in trees:
            trees[t] = cKDTree(sets[t])
        for _ in range(passes):
            trees[t].query(sets[s], workers=16)
    return 1e3 * (time.perf_counter() - t0)


def child(a, name):
    from bundleadjustment_amd import Solver
    rng = np.random.default_rng(0xBA5E1C90)
    with Solver(0) as s:
        if name == "crossover":
            rec = {}
            for n_tgt in CROSSOVER:
                src, tgt = clouds(rng, 2000, n_tgt)
                rec[str(n_tgt)] = {route: timed(s, [src, tgt], [[0, 1]], a, route=route)["kernel_ms"] for route in ("GRID", "BRUTE")}
            print(json.dumps(rec))
            return
        n_pairs, n_src, n_tgt = SHAPES[name]
        sets, pairs = [], []
        for i in range(n_pairs):
            src, tgt = clouds(rng, n_src, n_tgt)
            sets += [src, tgt]
            pairs.append([2 * i, 2 * i + 1])
        rec = {"pairs": n_pairs, "n_src": n_src, "n_tgt": n_tgt, **timed(s, sets, pairs, a)}
        if n_pairs > 1:      # the batch under either route, beside the single pair of `crossover`
            for route in ("GRID", "BRUTE"):
                t = timed(s, sets, pairs, a, route=route)
                rec[route] = {k: t[k] for k in ("wall_ms", "host_prep_ms", "kernel_ms")}
    if not a.no_host:
        ms = cpu_kdtree_ms(sets, pairs)
        rec["cpu_kdtree_ms"] = ms if ms is not None else "scipy is not installed"
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-host", action="store_true", help="skip the host kd-tree")
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds per shape")
    ap.add_argument("--tree", default="", help="a label of the source tree, recorded as given")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "icp_bench.json"))
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a, a.child)
        return 0
    rec = {"date": time.strftime("%Y-%m-%d"), "tree": a.tree, "reps": a.reps, "warmup": a.warmup}
    rc = 0
    for name in list(SHAPES) + ["crossover"]:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, __file__, "--child", name,
               "--reps", str(a.reps), "--warmup", str(a.warmup)] + (["--no-host"] if a.no_host else [])
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
