"""Reconstruction error: the reference's second accuracy figure
(``--reconstruction-error``, ba_project/src/metrics/ReconstructionError.cpp:49-190),
beside the trajectory ATE of ``trajectory.py``.

``computeReconstructionError`` brings the estimated map into the frame of the
ground-truth mesh, normalises both clouds and returns the fitness score of a
PCL point-to-point ICP with every default.  ``normalise_clouds`` restates the
preparation in float32 numpy; the ICP and the fitness run on the device
(``Solver.icp``, ba_icp of include/ba_hip.h):

1. transform the map points by ``gt_pose0^-1`` (ReconstructionError.cpp:93-97;
   the inverse is formed in float64 and rounded to float32, the product is
   ``((m0 x + m1 y) + m2 z) + t`` per row in float32);
2. zero-centre both clouds (``zeroCenterPointCloud``): the centroid is the
   float64 mean rounded to float32.  PCL's ``compute3DCentroid`` accumulates in
   float32; for n points of magnitude m the two differ by at most about
   n * 2^-24 * m in the worst case (DESIGN.md 27.3 states the bound);
3. ``computeUniformScaleFactor`` with percentile 0: the ratio of the largest
   bounding-box extents, target over source, as a float32 quotient, and
   ``scalePointCloud``: a float32 product per coordinate;
4. ICP of the source against the target and ``getFitnessScore``.  As the
   reference does, a run that did not converge reports the float32 maximum.
"""
from __future__ import annotations

import os

import numpy as np

from .io import read_ply_vertices

FLT_MAX = float(np.finfo(np.float32).max)


def zero_centre(cloud: np.ndarray) -> np.ndarray:
    c = np.asarray(cloud, dtype=np.float32).reshape(-1, 3)
    centroid = c.astype(np.float64).mean(axis=0).astype(np.float32)
    return (c - centroid).astype(np.float32)


def largest_extent(cloud: np.ndarray) -> np.float32:
    c = np.asarray(cloud, dtype=np.float32).reshape(-1, 3)
    return np.float32((c.max(axis=0) - c.min(axis=0)).astype(np.float32).max())


def transform_cloud(cloud: np.ndarray, T: np.ndarray) -> np.ndarray:
    """T (4x4, row-major) applied to (n, 3) float32 points, in float32."""
    c = np.asarray(cloud, dtype=np.float32).reshape(-1, 3)
    m = np.asarray(T, dtype=np.float32).reshape(4, 4)
    x, y, z = c[:, 0], c[:, 1], c[:, 2]
    return np.stack([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)], axis=1).astype(np.float32)


def normalise_clouds(points, target, gt_pose0=None) -> tuple[np.ndarray, np.ndarray, np.float32]:
    """Steps 1-3: (source, target, scale factor), float32."""
    src = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    tgt = np.asarray(target, dtype=np.float32).reshape(-1, 3)
    if src.shape[0] == 0 or tgt.shape[0] == 0:
        raise ValueError("reconstruction_error: an empty cloud")
    if gt_pose0 is not None:
        inv = np.linalg.inv(np.asarray(gt_pose0, dtype=np.float64).reshape(4, 4)).astype(np.float32)
        src = transform_cloud(src, inv)
    src, tgt = zero_centre(src), zero_centre(tgt)
    scale = np.float32(largest_extent(tgt) / largest_extent(src))
    return (src * scale).astype(np.float32), tgt, scale


def reconstruction_error(points, target, gt_pose0=None, solver=None, **icp_options) -> dict:
    """The reference's reconstruction error of a map cloud.  points: (n, 3);
    target: (m, 3) points or the path of a PLY; gt_pose0: the 4x4 ground-truth
    pose of the first keyframe (None: identity); solver: a Solver (None: one on
    device 0 for this call).  Returns a dict: error (the fitness, or the
    float32 maximum when ICP did not converge), converged, state, iterations,
    final (4x4), scale, n_source, n_target."""
    if isinstance(target, (str, os.PathLike)):
        target = read_ply_vertices(target)
    src, tgt, scale = normalise_clouds(points, target, gt_pose0)
    own = solver is None
    if own:
        from .solver import Solver
        solver = Solver(0)
    try:
        res, _mse = solver.icp([src, tgt], [[0, 1]], **icp_options)
    finally:
        if own:
            solver.close()
    r = res[0]
    converged = bool(r["converged"])
    return dict(error=float(r["fitness"]) if converged else FLT_MAX, converged=converged, state=int(r["state"]),
                iterations=int(r["iterations"]), final=np.array(r["final"]), scale=float(scale),
                n_source=int(src.shape[0]), n_target=int(tgt.shape[0]))
