"""CPU reference and helpers for ba_covariance_iterative: block columns of the
inverse reduced camera system by per-column PCG.  Never loads the HIP library.

Everything is built from the reference's own H = J^T J (covariance_ref.py, or
build_sparse below for problems whose dense S does not fit):

  Jacobi scaling   s = 1 / (1 + sqrt(diag Hcc))
  S_scaled,ref     s (Hcc - Hcp Hpp^-1 Hpc) s, applied through the sparse factors
  restatement      per-column PCG from x = 0 with the stopping rule |r|_2 <= tau
                   (|e|_2 = 1) and the residual reset every 10 iterations, then
                   Cov(i, v) = s_i X[i, :] s_v and, for a point,
                   Hpp_p^-1 + T_p Sigma[:, observers] T_p[:, observers]^T

Tolerances, all from the reference (rho_j the true residual of column j,
|rho_j| <= tau, kappa = cond2(S_scaled,ref)):

  cameras          tau sqrt(kappa) + ref.tolerance() in covariance_ref.block_error's
                   measure: |e_i^T S^-1 rho_j| <= sqrt((S^-1)_ii) |rho_j|_{S^-1} (Cauchy-
                   Schwarz in the S^-1 inner product), |rho_j|_{S^-1} <= tau / sqrt(lambda_min)
                   and (S^-1)_jj >= 1 / lambda_max
  point, k variable observers
                   2 sqrt(6 k) tau sqrt(kappa) + ref.tolerance(): the same argument
                   with |[rho_j]|_2 <= sqrt(6 k) tau over the 6 k columns
  residual check   x^ = s^-1 Cov[:, v] s_v^-1 rebuilt from a full requested column:
                   |e - S_scaled,ref x^|_2 <= tau + gamma, gamma = 4 k_max eps
                   |s (|Hcc| + |Hcp| |Hpp^-1| |Hpc|) (s |x^|)|_2, k_max the largest
                   observation count of a camera: the componentwise cost of
                   forming S x from sums of at most k_max terms; independent of kappa
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

import covariance_ref as R

EPS = R.EPS
TAU = 1e-10


@dataclass
class System:
    n: int
    s: np.ndarray            # [n] Jacobi scaling of the camera columns
    Hcc: object              # sparse [n, n]
    Hcp: object              # sparse [n, q]
    Hpp_inv: np.ndarray      # [q / 3, 3, 3]
    T: object                # sparse [q, n] = Hpp^-1 Hpc
    absT: object             # sparse [q, n] = |Hpp^-1| |Hpc|
    cam_var: np.ndarray
    pt_var: np.ndarray
    vc: np.ndarray           # camera -> compact variable index or -1
    vp: np.ndarray           # point -> compact variable index or -1
    k_max: int

    def apply(self, x):
        """S_scaled,ref x (x [n] or [n, c])."""
        s = self.s if x.ndim == 1 else self.s[:, None]
        y = s * x
        return s * (self.Hcc @ y - self.Hcp @ (self.T @ y))

    def apply_abs(self, x):
        """s (|Hcc| + |Hcp| |Hpp^-1| |Hpc|) (s x) for x >= 0."""
        s = self.s if x.ndim == 1 else self.s[:, None]
        y = s * x
        return s * (abs(self.Hcc) @ y + abs(self.Hcp) @ (self.absT @ y))

    def dense(self):
        return self.apply(np.eye(self.n))


def system_from_H(H, n, cam_var, pt_var, p) -> System:
    H = H.tocsr()
    q = H.shape[0] - n
    Hcc = H[:n, :n].tocsr()
    Hcp = H[:n, n:].tocsr()
    d = H[n:, n:].tocoo()
    assert np.all(d.row // 3 == d.col // 3)
    blocks = np.zeros((q // 3, 3, 3))
    blocks[d.row // 3, d.row % 3, d.col % 3] = d.data
    binv = np.linalg.inv(blocks) if q else blocks

    def bdiag(b):
        return (sp.bsr_matrix((b, np.arange(q // 3), np.arange(q // 3 + 1)), shape=(q, q)).tocsr()
                if q else sp.csr_matrix((0, 0)))
    T = (bdiag(binv) @ Hcp.T).tocsr() if q else sp.csr_matrix((0, n))
    absT = (bdiag(np.abs(binv)) @ abs(Hcp.T)).tocsr() if q else sp.csr_matrix((0, n))
    s = 1.0 / (1.0 + np.sqrt(Hcc.diagonal()))
    vc = np.full(p.n_cams, -1)
    vc[cam_var] = np.arange(cam_var.sum())
    vp = np.full(p.n_pts, -1)
    vp[pt_var] = np.arange(pt_var.sum())
    k_max = int(np.bincount(p.obs_cam, minlength=p.n_cams).max())
    return System(n, s, Hcc, Hcp, binv, T, absT, cam_var, pt_var, vc, vp, k_max)


def system_of(ref: R.Reference, p) -> System:
    return system_from_H(ref.H, ref.n, ref.cam_var, ref.pt_var, p)


def build_sparse(oracle, p) -> System:
    """The same H as covariance_ref.reference, kept sparse throughout (no dense
    S, no inverse): for problems beyond the dense route."""
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
    mc, mp = vc[p.obs_cam] >= 0, vp[p.obs_pt] >= 0
    for r in range(2):
        for a in range(6):
            rows.append(2 * o[mc] + r)
            cols.append(6 * vc[p.obs_cam[mc]] + a)
            vals.append(J[mc, r, a])
        for a in range(3):
            rows.append(2 * o[mp] + r)
            cols.append(n + 3 * vp[p.obs_pt[mp]] + a)
            vals.append(J[mp, r, 6 + a])
    Js = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(2 * no, n + q))
    return system_from_H((Js.T @ Js).tocsr(), n, cam_var, pt_var, p)


def preconditioner(sys: System, kind: str) -> np.ndarray:
    """[n / 6, 6, 6] inverses of the 6 x 6 diagonal blocks of s Hcc s ("jacobi")
    or of S_scaled,ref ("schur_jacobi")."""
    nv = sys.n // 6
    blocks = np.empty((nv, 6, 6))
    for v in range(nv):
        sl = slice(6 * v, 6 * v + 6)
        B = sys.Hcc[sl, sl].toarray()
        if kind == "schur_jacobi":
            B = B - (sys.Hcp[sl] @ sys.T[:, sl]).toarray()
        else:
            assert kind == "jacobi"
        blocks[v] = np.linalg.inv(sys.s[sl, None] * B * sys.s[None, sl])
    return blocks


def pcg_column(sys: System, Minv: np.ndarray, col: int, tau: float = TAU, max_iterations: int = 500):
    """One column of S_scaled,ref^-1 by PCG from x = 0.  Returns (x, iterations,
    converged)."""
    n = sys.n
    e = np.zeros(n)
    e[col] = 1.0

    def prec(r):
        return np.einsum("vab,vb->va", Minv, r.reshape(-1, 6)).ravel()
    x = np.zeros(n)
    r = e.copy()
    if np.linalg.norm(r) <= tau:
        return x, 0, True
    z = prec(r)
    pdir = z.copy()
    rho = r @ z
    for it in range(1, max_iterations + 1):
        q = sys.apply(pdir)
        pq = pdir @ q
        assert pq > 0.0 and np.isfinite(pq)
        alpha = rho / pq
        x = x + alpha * pdir
        r = e - sys.apply(x) if it % 10 == 0 else r - alpha * q
        if np.linalg.norm(r) <= tau:
            return x, it, True
        if it >= max_iterations:
            break
        z = prec(r)
        rho_new = r @ z
        pdir = z + (rho_new / rho) * pdir
        rho = rho_new
    return x, max_iterations, False


def column_cameras(sys: System, p, pairs, points) -> list[int]:
    """Distinct column cameras (camera ids, increasing) of a request."""
    cams = set()
    for i, j in np.asarray(pairs).reshape(-1, 2):
        if sys.cam_var[i] and sys.cam_var[j]:
            cams.add(int(j))
    order = np.argsort(p.obs_pt, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(p.obs_pt, minlength=p.n_pts))])
    for pt in np.asarray(points).reshape(-1):
        if not sys.pt_var[pt]:
            continue
        for c in p.obs_cam[order[off[pt]:off[pt + 1]]]:
            if sys.cam_var[c]:
                cams.add(int(c))
    return sorted(cams)


def restatement(sys: System, p, pairs, points, kind="schur_jacobi", tau=TAU, max_iterations=500):
    """The whole route in numpy: (cam_cov [m, 6, 6], pt_cov [k, 3, 3], info)."""
    Minv = preconditioner(sys, kind)
    pairs = np.asarray(pairs).reshape(-1, 2)
    points = np.asarray(points).reshape(-1)
    sigma_cols = {}          # camera id -> [n, 6] unscaled columns of Sigma_cc
    iters, conv = 0, 0
    for c in column_cameras(sys, p, pairs, points):
        v = sys.vc[c]
        X = np.empty((sys.n, 6))
        for j in range(6):
            X[:, j], it, ok = pcg_column(sys, Minv, 6 * v + j, tau, max_iterations)
            iters = max(iters, it)
            conv += int(ok)
        sigma_cols[c] = sys.s[:, None] * X * sys.s[None, 6 * v:6 * v + 6]
    cam_cov = np.zeros((len(pairs), 6, 6))
    for q, (i, j) in enumerate(pairs):
        if sys.cam_var[i] and sys.cam_var[j]:
            cam_cov[q] = sigma_cols[int(j)][6 * sys.vc[i]:6 * sys.vc[i] + 6]
    pt_cov = np.zeros((len(points), 3, 3))
    for q, pt in enumerate(points):
        if not sys.pt_var[pt]:
            continue
        Tp = sys.T[3 * sys.vp[pt]:3 * sys.vp[pt] + 3].toarray()           # [3, n]
        acc = sys.Hpp_inv[sys.vp[pt]].copy()
        for v in np.flatnonzero(np.abs(Tp).reshape(3, -1, 6).sum(axis=(0, 2)) > 0):
            cam = int(np.flatnonzero(sys.vc == v)[0])
            acc += Tp @ sigma_cols[cam] @ Tp[:, 6 * v:6 * v + 6].T
        pt_cov[q] = acc
    return cam_cov, pt_cov, {"n_columns": 6 * len(sigma_cols), "n_converged": conv, "max_iterations_used": iters}


def kappa(sys: System) -> float:
    S = sys.dense()
    return float(np.linalg.cond(0.5 * (S + S.T)))


def cam_bound(ref: R.Reference, kap: float, tau: float = TAU) -> float:
    return tau * np.sqrt(kap) + ref.tolerance()


def pt_bound(ref: R.Reference, kap: float, k_obs: int, tau: float = TAU) -> float:
    return 2.0 * np.sqrt(6.0 * k_obs) * tau * np.sqrt(kap) + ref.tolerance()


def variable_observers(sys: System, p, pt: int) -> int:
    """Observations of point pt by variable cameras (duplicates each count)."""
    return int(sys.cam_var[p.obs_cam[p.obs_pt == pt]].sum())


def pt_errors(got, points, ref: R.Reference, sys: System, p, kap: float, tau: float = TAU):
    """Worst (error / bound) over the requested variable points, and the worst error."""
    worst_ratio, worst = 0.0, 0.0
    for blk, pt in zip(got, points):
        if not ref.pt_var[pt]:
            continue
        v = np.diag(ref.pt_cov[int(pt)])
        e = R.block_error(blk, ref.pt_cov[int(pt)], v, v)
        worst = max(worst, e)
        worst_ratio = max(worst_ratio, e / pt_bound(ref, kap, variable_observers(sys, p, int(pt)), tau))
    return worst_ratio, worst


def column_residual(sys: System, cam: int, column_blocks: np.ndarray, tau: float = TAU):
    """column_blocks [n / 6, 6, 6]: Cov(i, cam) for every variable camera i in
    compact order.  Returns (worst |e - S_scaled,ref x^|_2 over the six
    columns, worst (residual - gamma), i.e. what must be <= tau)."""
    v = sys.vc[cam]
    C = np.asarray(column_blocks).reshape(sys.n, 6)
    xh = C / sys.s[:, None] / sys.s[None, 6 * v:6 * v + 6]
    E = np.zeros((sys.n, 6))
    E[6 * v:6 * v + 6] = np.eye(6)
    res = np.linalg.norm(E - sys.apply(xh), axis=0)
    gamma = 4.0 * sys.k_max * EPS * np.linalg.norm(sys.apply_abs(np.abs(xh)), axis=0)
    return float(res.max()), float((res - gamma).max()), float(gamma.max())
