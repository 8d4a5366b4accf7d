#!/usr/bin/env python3
"""Time of ba_map_graph.  Synthetic tables only.  Not bench.py.

  c3_all        200 frames x 100k points x 10 views, all frames queried, windows on
  c4_all        1000 frames x 1M points x 10 views, all frames queried, windows off
  c4_256        the same table, 256 queries, windows on
  c3_one        one query on the C3-like table (a keyframe insertion)

A point's track is `views` frames out of 2 * views consecutive ones, so a frame
shares points with about 4 * views neighbours.  Every figure is the median of
--reps timed calls after --warmup calls: wall time (host clock around the
blocking call: the upload of the table, the host's frame-sorted view, the
kernels, the records back), and host preparation and kernel time from
ba_map_graph_times.  The lists stay on the device (ba_map_graph_lists is not
timed).  host_ms is the same work in tests/cpp/map_graph_host.cpp built -O2
without sanitizers, on one host thread (its own tracks of the same shape).
The numbers are reported, not gated.  Each shape runs in a child process of
its own under `timeout -k 10`; the first shape that fails ends the run.
Writes one JSON record (default profiles/map_graph_bench.json) and prints it."""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

# frames, points, views, queries, windows
SHAPES = {"c3_all": (200, 100_000, 10, 200, 1), "c4_all": (1000, 1_000_000, 10, 1000, 0),
          "c4_256": (1000, 1_000_000, 10, 256, 1), "c3_one": (200, 100_000, 10, 1, 1)}


def table(rng, nf, n_pts, views):
    from bundleadjustment_amd.problem import MapTable
    f0 = rng.integers(0, nf, n_pts)
    frame = (f0[:, None] + 2 * np.arange(views)[None, :] + rng.integers(0, 2, (n_pts, views))) % nf
    return MapTable(frame_id=np.arange(nf), obs_offset=np.arange(n_pts + 1, dtype=np.int64) * views,
                    obs_frame=frame.reshape(-1), pt_ref_frame=f0, obs_octave=rng.integers(0, 8, n_pts * views),
                    obs_outlier=rng.random(n_pts * views) < 0.05).normalized()


def host_seconds(nf, n_pts, views, nq, windows):
    with tempfile.TemporaryDirectory() as tmp:
        exe, case = Path(tmp) / "map_graph_host", Path(tmp) / "case.txt"
        subprocess.run(["g++", "-std=c++17", "-O2", str(ROOT / "tests" / "cpp" / "map_graph_host.cpp"), "-o", str(exe)],
                       check=True)
        case.write_text(f"synth {nf} {n_pts} {views} {nq} {windows} 7\n")
        out = subprocess.run([str(exe), str(case)], capture_output=True, text=True, check=True).stdout
    return float(out.split()[0])


def child(a, name):
    from bundleadjustment_amd import Solver
    nf, n_pts, views, nq, windows = SHAPES[name]
    t = table(np.random.default_rng(0xBA5E1000), nf, n_pts, views)
    q = (np.arange(nq, dtype=np.int64) * nf // nq).astype(np.int32)
    opts = dict(build_windows=windows, debug_tile_frames=a.tile, debug_chunk_queries=a.chunk)
    wall, times = [], []
    with Solver(0) as s:
        for it in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            res = s.map_graph(t, q, lists=False, **opts)
            if it >= a.warmup:
                wall.append(1e3 * (time.perf_counter() - t0))
                times.append(s.map_graph_times())
    k, r = np.array(times), res.records
    rec = {"frames": nf, "points": n_pts, "views": views, "queries": nq, "windows": windows, "tile": a.tile, "chunk": a.chunk,
           "table_mib": sum(x.nbytes for x in (t.obs_frame, t.obs_octave, t.obs_outlier, t.obs_offset)) / 2 ** 20,
           "wall_ms": statistics.median(wall), "wall_ms_min": min(wall), "wall_ms_max": max(wall),
           "host_prep_ms": float(np.median(k[:, 0])), "kernel_ms": float(np.median(k[:, 1])),
           "kernel_ms_min": float(k[:, 1].min()), "kernel_ms_max": float(k[:, 1].max()),
           "mean_degree": float(r["degree"].mean()), "sum_win_obs": int(r["n_win_obs"].sum(dtype=np.int64)),
           "culled": int(r["cull"].sum())}
    if not a.no_host:
        rec["host_ms"] = 1e3 * host_seconds(nf, n_pts, views, nq, windows)
        rec["host_over_wall"] = rec["host_ms"] / rec["wall_ms"]
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tile", type=int, default=0, help="debug_tile_frames (0: automatic)")
    ap.add_argument("--chunk", type=int, default=0, help="debug_chunk_queries (0: from the scratch budget)")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--no-host", action="store_true", help="skip the one-thread host program")
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds per shape")
    ap.add_argument("--tree", default="", help="a label of the source tree, recorded as given")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "map_graph_bench.json"))
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a, a.child)
        return 0
    rec = {"date": time.strftime("%Y-%m-%d"), "tree": a.tree, "reps": a.reps, "warmup": a.warmup}
    rc = 0
    for name in a.shapes.split(","):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, __file__, "--child", name, "--reps", str(a.reps),
               "--warmup", str(a.warmup), "--tile", str(a.tile), "--chunk", str(a.chunk)] + (["--no-host"] if a.no_host else [])
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
