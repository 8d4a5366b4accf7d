#!/usr/bin/env python3
"""Time of ba_map_points_update and ba_associate.  Synthetic unit-norm
descriptors only.  Not bench.py.

  c3_map       100k points x 10 views, rows drawn from 200 frames of 5000 keypoints
  local_window 2000 points x 6 views
  long_tracks  2000 points x 64 views
  associate    25 neighbours x 1000 items (ba_associate)

Every figure is the median of --reps timed calls after --warmup calls: wall
time (host clock around the blocking call, which includes the upload of the
descriptor table) and, for ba_map_points_update, the kernels' device time (HIP
events).  gathered_gb_s is the bytes of the rows that the tracks name (n_obs
dim 4) over the kernel time: an effective rate beside the chip's 8 TB/s, not a
measured traffic.  host_ms is the same work in tests/cpp/map_points_host.cpp
built -O2 without sanitizers, on one host thread (its own synthetic rows of
the same shape).  The numbers are reported, not gated.  Each shape runs in a
child process of its own under `timeout -k 10`; the first shape that fails
ends the run.  Writes one JSON record (default profiles/map_points_bench.json)
and prints it."""
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

# points, views, descriptor rows
SHAPES = {"c3_map": (100_000, 10, 200 * 5000), "local_window": (2000, 6, 6 * 5000), "long_tracks": (2000, 64, 64 * 5000)}
HBM_SPEC_GB_S = 8000.0


def unit(rng, n, dim):
    x = rng.standard_normal((n, dim), dtype=np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def map_batch(rng, n_pts, views, n_rows, dim, n_cams=200):
    from bundleadjustment_amd.problem import MapPointBatch
    no = n_pts * views
    pts = (rng.uniform(-1, 1, (n_pts, 3)) + [0, 0, 6]).astype(np.float32)
    return MapPointBatch(dim=dim, cam_center=rng.uniform(-2, 2, (n_cams, 3)).astype(np.float32), pts=pts,
                         obs_offset=(np.arange(n_pts + 1, dtype=np.int64) * views).astype(np.int32),
                         obs_cam=rng.integers(0, n_cams, no).astype(np.int32),
                         obs_row=rng.integers(0, n_rows, no).astype(np.int32),
                         obs_scale=(1.2 ** rng.integers(0, 8, no)).astype(np.float32),
                         ref_obs=rng.integers(0, views, n_pts).astype(np.int32), desc=unit(rng, n_rows, dim))


def host_seconds(n_pts, views, n_rows, dim):
    with tempfile.TemporaryDirectory() as tmp:
        exe, case = Path(tmp) / "map_points_host", Path(tmp) / "case.txt"
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", str(ROOT / "tests" / "cpp" / "map_points_host.cpp"),
                        "-o", str(exe)], check=True)
        case.write_text(f"synth {dim} {n_pts} {views} {n_rows} 7\n")
        out = subprocess.run([str(exe), str(case)], capture_output=True, text=True, check=True).stdout
    return float(out.split()[0])


def child(a, name):
    from bundleadjustment_amd import Solver
    from bundleadjustment_amd.problem import pack_assoc_batch
    dim = a.dim
    rng = np.random.default_rng(0xBA5E0F00)
    wall, kern = [], []
    if name == "associate":
        n_cams, per = 25, 1000
        mb = map_batch(rng, 5000, 6, 30_000, dim, n_cams)
        with Solver(0) as s:
            rec, desc_out = s.map_points_update(mb, median_rule=1)
            extr = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (n_cams, 1))
            extr[:, 12:15] = -mb.cam_center
            K = np.tile(np.array([520, 0, 0, 0, 520, 0, 320, 240, 1], np.float32), (n_cams, 1))
            size = np.tile(np.array([640, 480], np.int32), (n_cams, 1))
            ni = n_cams * per
            cam, pt = np.repeat(np.arange(n_cams), per), rng.integers(0, 5000, ni)
            X = mb.pts[pt] - mb.cam_center[cam]
            uv = 520 * X[:, :2] / X[:, 2:3] + [320, 240] + rng.standard_normal((ni, 2))
            ab = pack_assoc_batch(extr, mb.cam_center, K, size, mb.pts, rec["view_dir"],
                                  np.stack([rec["min_dist"], rec["max_dist"]], axis=1), desc_out, mb.desc, cam, pt, uv,
                                  rng.integers(0, 30_000, ni), (1.2 ** rng.integers(0, 8, ni)).astype(np.float32),
                                  np.where(rng.random(ni) < 0.3, rng.integers(0, 30_000, ni), -1),
                                  rng.integers(0, 5000, (1000, 2)))
            for it in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                items, fuse = s.associate(ab)
                if it >= a.warmup:
                    wall.append(1e3 * (time.perf_counter() - t0))
        print(json.dumps({"cameras": n_cams, "items": ni, "fuse_pairs": 1000, "dim": dim,
                          "uploaded_mib": (ab.desc.nbytes + ab.pt_desc.nbytes) / 2 ** 20,
                          "wall_ms": statistics.median(wall), "wall_ms_min": min(wall), "wall_ms_max": max(wall),
                          "statuses": np.bincount(items["status"], minlength=9).tolist()}))
        return
    n_pts, views, n_rows = SHAPES[name]
    mb = map_batch(rng, n_pts, views, n_rows, dim)
    with Solver(0) as s:
        for it in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            s.map_points_update(mb, median_rule=1)
            if it >= a.warmup:
                wall.append(1e3 * (time.perf_counter() - t0))
                kern.append(s.map_points_times())
    k = np.array(kern)
    kernel_ms = float(np.median(k[:, 1]))
    gathered = float(n_pts) * views * dim * 4
    rec = {"points": n_pts, "views": views, "rows": n_rows, "dim": dim, "uploaded_mib": mb.desc.nbytes / 2 ** 20,
           "gathered_mib": gathered / 2 ** 20, "wall_ms": statistics.median(wall), "wall_ms_min": min(wall),
           "wall_ms_max": max(wall), "host_prep_ms": float(np.median(k[:, 0])), "kernel_ms": kernel_ms,
           "kernel_ms_min": float(k[:, 1].min()), "kernel_ms_max": float(k[:, 1].max()),
           "gathered_gb_s": 1e-6 * gathered / kernel_ms, "share_of_hbm_spec": 1e-6 * gathered / kernel_ms / HBM_SPEC_GB_S}
    if not a.no_host:
        rec["host_ms"] = 1e3 * host_seconds(n_pts, views, n_rows, dim)
        rec["host_over_kernel"] = rec["host_ms"] / kernel_ms
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dim", type=int, default=64, choices=(64, 128))
    ap.add_argument("--no-host", action="store_true", help="skip the one-thread host program")
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds per shape")
    ap.add_argument("--tree", default="", help="a label of the source tree, recorded as given")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "map_points_bench.json"))
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a, a.child)
        return 0
    rec = {"date": time.strftime("%Y-%m-%d"), "tree": a.tree, "reps": a.reps, "warmup": a.warmup, "dim": a.dim,
           "hbm_spec_gb_s": HBM_SPEC_GB_S}
    rc = 0
    for name in list(SHAPES) + ["associate"]:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, __file__, "--child", name,
               "--reps", str(a.reps), "--warmup", str(a.warmup), "--dim", str(a.dim)] + (["--no-host"] if a.no_host else [])
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
