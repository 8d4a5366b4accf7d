#!/usr/bin/env python3
"""Time of ba_match_descriptors (exact 2-NN on the f32 matrix cores, ratio
test, unique-train filter).  Synthetic unit-norm descriptors only.  Not
bench.py.

  shapes (dim 64): one pair of 2000 x 2000; ten pairs sharing one query set
                   (a frame against its ten covisible neighbours, the
                   searchInNeighbors shape); 256 pairs of 1000 x 1000

Every figure is the median of --reps timed calls after --warmup calls: wall
time (host clock around the blocking call) and the kernels' device time (HIP
events, with its three phases) beside it.  The contraction's rate is 2 n_q n_t
dim flop over the 2-NN phase's time, and is also given as a share of the f32
MFMA rate of an untuned LDS-tiled GEMM (--mfma-tflops, default 122).  The
numbers are reported, not gated.  Each shape runs in a child process of its
own under `timeout -k 10`; the first shape that fails ends the run.  Writes one
JSON record (default profiles/match_bench.json) and prints it.
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

SHAPES = {"one_pair": (1, 2000, False), "ten_neighbours": (10, 2000, True), "many_pairs": (256, 1000, False)}


def unit(rng, n, dim):
    x = rng.standard_normal((n, dim))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def child(a, name):
    from bundleadjustment_amd import Solver, pack_match_batch
    pairs, rows, shared = SHAPES[name]
    dim = a.dim
    rng = np.random.default_rng(0xBA5E0E00 + pairs)
    sets, idx, qs = [], [], 0
    for i in range(pairs):
        if not shared or i == 0:
            sets.append(unit(rng, rows, dim))
            qs = len(sets) - 1
        # 60 % of the train rows are noisy copies of query rows, the rest distractors
        train = unit(rng, rows, dim)
        k = int(0.6 * rows)
        src, dst = rng.permutation(rows)[:k], rng.permutation(rows)[:k]
        noisy = sets[qs][src].astype(np.float64) + 0.02 * rng.standard_normal((k, dim))
        train[dst] = (noisy / np.linalg.norm(noisy, axis=1, keepdims=True)).astype(np.float32)
        sets.append(train)
        idx.append((qs, len(sets) - 1))
    mb = pack_match_batch(sets, idx)
    wall, kern = [], []
    with Solver(0) as s:
        for it in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            off, m = s.match_descriptors(mb)
            if it >= a.warmup:
                wall.append(1e3 * (time.perf_counter() - t0))
                kern.append(s.match_times())
    k = np.array(kern)
    flop = 2.0 * pairs * rows * rows * dim
    nn_ms = float(np.median(k[:, 4]))
    rec = {"pairs": pairs, "rows": rows, "dim": dim, "shared_query_set": shared,
           "uploaded_mib": mb.desc.nbytes / 2 ** 20,
           "wall_ms": statistics.median(wall), "wall_ms_min": min(wall), "wall_ms_max": max(wall),
           "host_prep_ms": float(np.median(k[:, 0])), "kernel_ms": float(np.median(k[:, 1])),
           "norms_ms": float(np.median(k[:, 3])), "nn_ms": nn_ms, "select_ms": float(np.median(k[:, 5])),
           "nn_tflops": 1e-9 * flop / nn_ms, "nn_share_of_f32_mfma_gemm": 1e-9 * flop / nn_ms / a.mfma_tflops,
           "matches": int(m.size), "matches_per_pair": m.size / pairs}
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dim", type=int, default=64, choices=(64, 128))
    ap.add_argument("--mfma-tflops", type=float, default=122.0, help="the f32 MFMA GEMM rate the share refers to")
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds per shape")
    ap.add_argument("--tree", default="", help="a label of the source tree, recorded as given")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "match_bench.json"))
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a, a.child)
        return 0
    rec = {"date": time.strftime("%Y-%m-%d"), "tree": a.tree, "reps": a.reps, "warmup": a.warmup, "dim": a.dim,
           "f32_mfma_gemm_tflops": a.mfma_tflops}
    rc = 0
    for name in SHAPES:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, __file__, "--child", name,
               "--reps", str(a.reps), "--warmup", str(a.warmup), "--dim", str(a.dim), "--mfma-tflops", str(a.mfma_tflops)]
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
