"""CPU reference for the marginal covariances (ba_covariance) and the shared
test problems.  Never calls the HIP library.

oracle.linearize gives the Huber-corrected Jacobian J in caller order.  The
variable blocks are the cameras / points that are not constant and have at
least one observation.  H = J^T J is built with scipy.sparse, the 3x3 point
blocks are inverted, the reduced camera system S = Hcc - Hcp Hpp^-1 Hpc is
formed densely and inverted with numpy:

  cameras  Sigma_cc = S^-1
  point p  Hpp_p^-1 + T_p Sigma_cc T_p^T,  T_p = Hpp_p^-1 Hpc_p

Blocks of constant (or unobserved) cameras and points are zero.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

from bundleadjustment_amd import make_synthetic
from bundleadjustment_amd.problem import fix_camera

EPS = 2.0 ** -53

# cams x pts x obs/pt of the shared problems -> order n of the reduced system
CASES = {
    "n24": (6, 40, 4),         # one partial tile
    "n132": (24, 300, 6),      # three tiles, the last one 4 rows
    "n192": (34, 400, 6),      # exactly three full tiles
    "n408": (70, 1500, 10),    # a longer chain
    "n1488": (250, 5000, 10),  # 24 block columns: the split / flow factorisation's Lf and Vbuf
}
ORDER = {"n24": 24, "n132": 132, "n192": 192, "n408": 408, "n1488": 1488}


def make_case(name: str):
    """make_synthetic(..., seed=7) with cameras 0 and 1 constant."""
    nc, npts, k = CASES[name]
    return fix_camera(make_synthetic(nc, npts, k, seed=7), 1)


@dataclass
class Reference:
    cam_cov: np.ndarray      # [n_cams, n_cams, 6, 6], zero blocks for constant / unobserved cameras
    pt_cov: dict             # point index -> [3, 3]
    cond_S: float
    n: int                   # order of S
    cam_var: np.ndarray      # [n_cams] bool
    pt_var: np.ndarray       # [n_pts] bool
    H: object                # sparse H over [variable cameras | variable points]

    def tolerance(self) -> float:
        """First-order bound for an inverse obtained through a Cholesky factor."""
        return max(1e-12, 4.0 * self.n * EPS * self.cond_S)


def reference(oracle, p, points=None) -> Reference:
    """points: indices whose 3x3 marginals are wanted (None: every point)."""
    _, J, _, ok = oracle.linearize(p)
    assert ok
    nc, npt, no = p.n_cams, p.n_pts, p.n_obs
    cam_fixed = np.zeros(nc, bool) if p.cam_fixed is None else p.cam_fixed.astype(bool)
    pt_fixed = np.zeros(npt, bool) if p.pt_fixed is None else p.pt_fixed.astype(bool)
    cam_var = ~cam_fixed & (np.bincount(p.obs_cam, minlength=nc) > 0)
    pt_var = ~pt_fixed & (np.bincount(p.obs_pt, minlength=npt) > 0)
    vc = np.full(nc, -1)
    vc[cam_var] = np.arange(cam_var.sum())
    vp = np.full(npt, -1)
    vp[pt_var] = np.arange(pt_var.sum())
    n, q = 6 * int(cam_var.sum()), 3 * int(pt_var.sum())
    rows, cols, vals = [], [], []
    o = np.arange(no)
    for r in range(2):
        mc = vc[p.obs_cam] >= 0
        for a in range(6):
            rows.append(2 * o[mc] + r)
            cols.append(6 * vc[p.obs_cam[mc]] + a)
            vals.append(J[mc, r, a])
        mp = vp[p.obs_pt] >= 0
        for a in range(3):
            rows.append(2 * o[mp] + r)
            cols.append(n + 3 * vp[p.obs_pt[mp]] + a)
            vals.append(J[mp, r, 6 + a])
    Js = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(2 * no, n + q))
    # the Jacobian of a constant block is zero in J: nothing of it may have been kept
    assert np.all(J[~cam_var[p.obs_cam], :, :6] == 0.0) and np.all(J[~pt_var[p.obs_pt], :, 6:] == 0.0)
    H = (Js.T @ Js).tocsr()
    Hcc = H[:n, :n].toarray()
    Hcp = H[:n, n:].tocsr()
    d = H[n:, n:].tocoo()
    assert np.all(d.row // 3 == d.col // 3)          # Hpp is block diagonal
    blocks = np.zeros((q // 3, 3, 3))
    blocks[d.row // 3, d.row % 3, d.col % 3] = d.data
    binv = np.linalg.inv(blocks) if q else blocks
    Hpp_inv = (sp.bsr_matrix((binv, np.arange(q // 3), np.arange(q // 3 + 1)), shape=(q, q)).tocsr()
               if q else sp.csr_matrix((0, 0)))
    T = (Hpp_inv @ Hcp.T).tocsr() if q else sp.csr_matrix((0, n))           # [q, n] = Hpp^-1 Hpc
    S = Hcc - (Hcp @ T).toarray() if q else Hcc
    S = 0.5 * (S + S.T)
    Sigma = np.linalg.inv(S) if n else S
    cond = float(np.linalg.cond(S)) if n else 1.0
    cam_cov = np.zeros((nc, nc, 6, 6))
    if n:
        idx = np.flatnonzero(cam_var)
        cam_cov[np.ix_(idx, idx)] = Sigma.reshape(len(idx), 6, len(idx), 6).transpose(0, 2, 1, 3)
    pt_cov = {}
    want = range(npt) if points is None else [int(x) for x in points]
    for pt in want:
        if vp[pt] < 0:
            pt_cov[pt] = np.zeros((3, 3))
            continue
        Tp = T[3 * vp[pt]:3 * vp[pt] + 3].toarray()
        pt_cov[pt] = binv[vp[pt]] + Tp @ Sigma @ Tp.T
    return Reference(cam_cov, pt_cov, cond, n, cam_var, pt_var, H)


def dense_inverse_check(ref: Reference) -> float:
    """Largest disagreement (in the tests' error measure) between the Schur
    route above and the inverse of the whole dense H."""
    Hd = ref.H.toarray()
    full = np.linalg.inv(0.5 * (Hd + Hd.T))
    n = ref.n
    worst = 0.0
    idx = np.flatnonzero(ref.cam_var)
    d = np.sqrt(np.diag(full))
    blk = full[:n, :n] / np.outer(d[:n], d[:n])
    got = ref.cam_cov[np.ix_(idx, idx)].transpose(0, 2, 1, 3).reshape(n, n) / np.outer(d[:n], d[:n])
    worst = max(worst, float(np.abs(got - blk).max())) if n else worst
    pidx = np.flatnonzero(ref.pt_var)
    for k, pt in enumerate(pidx):
        if int(pt) not in ref.pt_cov:
            continue
        sl = slice(n + 3 * k, n + 3 * k + 3)
        e = np.abs(ref.pt_cov[int(pt)] - full[sl, sl]) / np.outer(d[sl], d[sl])
        worst = max(worst, float(e.max()))
    return worst


def block_error(got, ref, var_i, var_j) -> float:
    """max |got - ref| / sqrt(ref_ii ref_jj) over a block; var_i / var_j: the
    reference variances of the row / column coordinates."""
    return float((np.abs(got - ref) / np.sqrt(np.outer(var_i, var_j))).max())


def cam_errors(got, pairs, ref: Reference) -> float:
    """Worst block_error over requested camera pairs with both cameras variable."""
    worst = 0.0
    for blk, (i, j) in zip(got, pairs):
        if not (ref.cam_var[i] and ref.cam_var[j]):
            continue
        vi, vj = np.diag(ref.cam_cov[i, i]), np.diag(ref.cam_cov[j, j])
        worst = max(worst, block_error(blk, ref.cam_cov[i, j], vi, vj))
    return worst


def pt_errors(got, points, ref: Reference) -> float:
    worst = 0.0
    for blk, pt in zip(got, points):
        if not ref.pt_var[pt]:
            continue
        v = np.diag(ref.pt_cov[int(pt)])
        worst = max(worst, block_error(blk, ref.pt_cov[int(pt)], v, v))
    return worst


@functools.lru_cache(maxsize=None)
def case_requests(name: str):
    """(cam_pairs [m, 2], points [k]) of a shared problem: every ordered camera
    pair and every point, except for the largest: every diagonal block, 500
    seeded random pairs and 200 seeded random points."""
    nc, npts, _ = CASES[name]
    if name != "n1488":
        i, j = np.meshgrid(np.arange(nc), np.arange(nc), indexing="ij")
        return np.stack([i.ravel(), j.ravel()], 1).astype(np.int32), np.arange(npts, dtype=np.int32)
    rng = np.random.default_rng(7)
    d = np.arange(nc)
    pairs = np.concatenate([np.stack([d, d], 1), rng.integers(0, nc, size=(500, 2))]).astype(np.int32)
    return pairs, np.sort(rng.choice(npts, size=200, replace=False)).astype(np.int32)


_CACHE: dict = {}


def case_reference(oracle, name: str):
    """(problem, Reference) of a shared problem, computed once per process and
    never modified by the tests."""
    if name not in _CACHE:
        p = make_case(name)
        _, points = case_requests(name)
        _CACHE[name] = (p, reference(oracle, p, points))
    return _CACHE[name]
