"""Problems with irregular visibility: mixed track lengths and a banded (or
full but very uneven) co-visibility graph.  Plain helper module.

make_synthetic gives every point exactly `obs_per_pt` cameras drawn uniformly,
so each of its problems has one track length and an (almost) full reduced
system.  `structured` starts from the same benign geometry with every visible
camera per point and keeps, for point q, the first lengths[q % len(lengths)]
visible cameras in cyclic ring order from a seeded start camera: tracks from 1
to "every camera", and windows on the camera ring, i.e. a banded S.  Only the
structure varies; cameras, points, noise and outliers are make_synthetic's.

SCENES lists the scenes the structure tests use and `plan_conditions` restates
in numpy the host rules (ensure_dense / ensure_pcg in ba_solver.hip) that pick
the code path from the structure, so a CPU test can assert that a scene is
built for the branch it is meant to reach.

Oracle-vs-oracle sensitivity to the caller's observation order (shuffled
against unshuffled build of the same scene, 6 LM iterations; measured by
tests/test_structured_problems_cpu.py, which asserts the cost and reduced
system bounds).  cost: largest relative difference of a per-iteration cost;
S: largest |diff| of oracle.reduced_system over its largest entry; params:
the smallest rtol at which cameras and points after the 6 iterations compare
equal with atol 1e-10 (0: every difference is below the atol).  Columns D =
DENSE_SCHUR, I = ITERATIVE_SCHUR + SCHUR_JACOBI.  The oracle's OpenMP sums are
not reproducible from run to run; each figure is the largest of several runs
at 1 to 8 threads, rounded up.

  scene      cost D   cost I   S        params D  params I
  band40     5e-14    3e-14    7e-14    3e-11     4e-11
  band40x    8e-15    2e-14    6e-15    3e-11     1e-11
  band40dup  4e-15    5e-15    3e-14    8e-12     7e-12
  mixed70    4e-15    7e-15    2e-14    0         0
  mixed66    6e-15    1e-14    2e-15    9e-12     2e-11
  band201    2e-13    6e-12    9e-15    1e-12     2e-12
  band230    9e-14    2e-14    2e-14    5e-12     9e-11
  ptfix40    2e-15    3e-15    5e-14    2e-11     2e-11

The parameter figures are the yardstick for the GPU parity tolerances
(tests/test_gpu_structure.py): a scene whose figure exceeded 1e-10 would be
compared at 100 x its figure (never above 1e-6); none does, so every scene is
compared at the project's rtol 1e-8 / atol 1e-10, >= 100 x above its figure.
The largest figures belong to the scenes with 1-tracks and to band230's
ITERATIVE_SCHUR run: a point seen once, or over a short baseline, is held
along its ray by the LM damping alone and sits at |X| ~ 1e4 after a step.
"""
from __future__ import annotations

import numpy as np

from bundleadjustment_amd import make_synthetic
from bundleadjustment_amd.problem import Problem, fix_camera


def structured(n_cams, n_pts, lengths, seed, fixed_cams=(), pt_fixed_every=0, shuffle=True, drop_cam=None,
               dup_every=0) -> Problem:
    p = make_synthetic(n_cams, n_pts, obs_per_pt=n_cams, seed=seed)
    cam, pt, uv = p.obs_cam.astype(np.int64), p.obs_pt.astype(np.int64), p.obs_uv
    L = np.asarray(lengths, np.int64)[np.arange(n_pts) % len(lengths)]
    start = np.random.default_rng(seed ^ 0x5EED).integers(0, n_cams, n_pts)
    # rank of each observation within its point, in ring order from the start
    rel = (cam - start[pt]) % n_cams
    order = np.lexsort((rel, pt))
    first = np.zeros(n_pts + 1, np.int64)
    np.cumsum(np.bincount(pt, minlength=n_pts), out=first[1:])
    rank = np.empty(len(pt), np.int64)
    rank[order] = np.arange(len(pt)) - first[pt[order]]
    keep = rank < L[pt]
    if drop_cam is not None:
        keep &= cam != drop_cam
    cam, pt, uv = cam[keep], pt[keep], uv[keep]
    if dup_every:
        dup = (pt * n_cams + cam) % dup_every == 0
        cam = np.concatenate([cam, cam[dup]])
        pt = np.concatenate([pt, pt[dup]])
        uv = np.concatenate([uv, uv[dup] + np.float32(0.5)])
    if shuffle:
        perm = np.random.default_rng(seed ^ 0x0BADC0DE).permutation(len(cam))
        cam, pt, uv = cam[perm], pt[perm], uv[perm]
    p.obs_cam, p.obs_pt, p.obs_uv = cam.astype(np.int32), pt.astype(np.int32), uv
    for c in fixed_cams:
        fix_camera(p, c)
    if pt_fixed_every:
        p.pt_fixed = np.zeros(n_pts, np.uint8)
        p.pt_fixed[::pt_fixed_every] = 1
    return p.normalized()


SCENES = {
    "band40": dict(n_cams=40, n_pts=600, lengths=(1, 2, 3, 4, 5, 7, 8), seed=101, fixed_cams=(1,)),
    "band40x": dict(n_cams=40, n_pts=600, lengths=(2, 3, 4, 5, 7, 8), seed=101, fixed_cams=(1,)),
    "band40dup": dict(n_cams=40, n_pts=600, lengths=(2, 3, 4, 5, 7, 8), seed=101, fixed_cams=(1,), dup_every=7),
    "mixed70": dict(n_cams=70, n_pts=400, lengths=(1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 70), seed=102,
                    fixed_cams=(1, 35)),
    "mixed66": dict(n_cams=66, n_pts=400, lengths=(2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 5, 47), seed=103,
                    fixed_cams=(1,)),
    "band201": dict(n_cams=201, n_pts=1500, lengths=(2, 3, 5, 9, 12), seed=104, fixed_cams=(1,)),
    # (with tracks of 90 in place of 100 — 20000 of 25878 blocks filled — the branches are the same, but the
    # oracle's own cost at the rejected candidate of iteration 3 moves by 8e-12 .. 3.5e-11 with the
    # observation order, and from run to run: around the 1e-11 asked of it, and a third of the 1e-10 the GPU
    # is compared at.  With 100 it measures <= 7e-14 over repeated runs and thread counts.)
    "band230": dict(n_cams=230, n_pts=1500, lengths=(2, 3, 60, 100, 5, 9), seed=105, fixed_cams=(1,)),
    "ptfix40": dict(n_cams=40, n_pts=600, lengths=(2, 3, 4, 5, 7, 8, 20), seed=106, fixed_cams=(1,),
                    pt_fixed_every=3, drop_cam=20),
}

_cache: dict = {}


def scene(name: str, shuffle: bool = True) -> Problem:
    """The named scene (built once per process; callers get their own copy)."""
    key = (name, shuffle)
    if key not in _cache:
        _cache[key] = structured(shuffle=shuffle, **SCENES[name])
    return _cache[key].copy().normalized()


def plan_conditions(p: Problem) -> dict:
    """The structure-dependent inputs of the library's host plans, recomputed
    in numpy (ensure_dense / ensure_pcg, ba_solver.hip):
      nc, nvc        cameras; variable cameras with an observation
      nlow           lower off-diagonal blocks of S, nvc (nvc - 1) / 2
      nfull          those with a common variable point; nempty = nlow - nfull
      s_memset       nempty > nfull (S is cleared by a memset each step)
      dup_diag       a variable point seen twice by one variable camera (an
                     (I, I) pair block)
      max_track      most observations of one point; chunks_ok: <= 64 (the
                     point-aligned PCG chunks exist)
      ndup           pairs of observations of one variable point by one
                     variable camera (ensure_pcg's duplicate pairs)
      covis          [nvc, nvc] bool, camera pairs with a common variable point
      cam_of_vc      camera index of each row of the reduced system / 6"""
    nc, npt = p.n_cams, p.n_pts
    fixed = np.zeros(nc, bool) if p.cam_fixed is None else p.cam_fixed != 0
    used = np.zeros(nc, bool)
    used[p.obs_cam] = True
    cam_of_vc = np.flatnonzero(used & ~fixed)
    nvc = len(cam_of_vc)
    vc = np.full(nc, -1)
    vc[cam_of_vc] = np.arange(nvc)
    pt_var = np.ones(npt, bool) if p.pt_fixed is None else p.pt_fixed == 0
    cnt = np.zeros((npt, max(nvc, 1)), np.int64)
    sel = pt_var[p.obs_pt] & (vc[p.obs_cam] >= 0)
    np.add.at(cnt, (p.obs_pt[sel], vc[p.obs_cam[sel]]), 1)
    A = (cnt > 0).astype(np.int64)
    covis = (A.T @ A) > 0
    nlow = nvc * (nvc - 1) // 2
    nfull = int(np.tril(covis, -1).sum())
    track = np.bincount(p.obs_pt, minlength=npt)
    return dict(nc=nc, nvc=nvc, nlow=nlow, nfull=nfull, nempty=nlow - nfull, s_memset=nlow - nfull > nfull,
                dup_diag=bool((cnt > 1).any()), max_track=int(track.max()), chunks_ok=bool(track.max() <= 64),
                ndup=int((cnt * (cnt - 1) // 2).sum()), covis=covis, cam_of_vc=cam_of_vc)
