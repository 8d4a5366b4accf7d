"""CPU reference for the cross blocks and leverages of ba_covariance_ex.
Never calls the HIP library.

Built on covariance_ref.reference() and its sparse H over [variable cameras |
variable points].  With Sigma_cc = S^-1 and T_p = Hpp_p^-1 Hpc_p (3 x n):

  Cov(cam i, p) = -(Sigma_cc T_p^T)[i]                       6 x 3
  Cov(p, q)     = T_p Sigma_cc T_q^T + delta_pq Hpp_p^-1     3 x 3
  h_o           = J_o Sigma J_o^T over the variable blocks of observation
                  o = (c, p), J_o = [Jc | Jp] the oracle's corrected Jacobian

Blocks of constant (or unobserved) cameras and points are zero and contribute
nothing to a leverage.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import covariance_ref as R


@dataclass
class FullReference:
    ref: R.Reference
    J: np.ndarray            # [n_obs, 2, 9] the oracle's Jacobian, caller order
    Sigma: np.ndarray        # [n, n] Sigma_cc over the variable cameras
    T: object                # sparse [3 P_var, n]: Hpp^-1 Hpc
    binv: np.ndarray         # [P_var, 3, 3] Hpp_p^-1
    vc: np.ndarray           # [n_cams] compact index or -1
    vp: np.ndarray           # [n_pts]  compact index or -1

    def tolerance(self) -> float:
        return self.ref.tolerance()

    def _t(self, p):
        """(T_p restricted to its nonzero columns [3, m], those columns)."""
        rows = self.T[3 * self.vp[p]:3 * self.vp[p] + 3]
        cols = np.unique(rows.indices)
        return rows[:, cols].toarray(), cols

    def cam_var_diag(self, c) -> np.ndarray:
        return np.diag(self.Sigma)[6 * self.vc[c]:6 * self.vc[c] + 6] if self.vc[c] >= 0 else np.zeros(6)

    def sigma_t(self, p) -> np.ndarray:
        """Sigma_cc T_p^T, [n, 3]."""
        memo = self.__dict__.setdefault("_sigma_t", {})
        if p not in memo:
            if len(memo) > 4096:
                memo.clear()
            Tp, cols = self._t(p)
            memo[p] = self.Sigma[:, cols] @ Tp.T
        return memo[p]

    def pt_pt(self, p, q) -> np.ndarray:
        if self.vp[p] < 0 or self.vp[q] < 0:
            return np.zeros((3, 3))
        Tp, cp = self._t(p)
        Tq, cq = self._t(q)
        out = Tp @ self.Sigma[np.ix_(cp, cq)] @ Tq.T
        return out + self.binv[self.vp[p]] if p == q else out

    def cam_pt(self, c, p) -> np.ndarray:
        if self.vc[c] < 0 or self.vp[p] < 0:
            return np.zeros((6, 3))
        return -self.sigma_t(p)[6 * self.vc[c]:6 * self.vc[c] + 6]

    def leverages(self, p):
        """(h [n_obs, 2, 2], g [n_obs, 2]) of problem p (the one the reference
        was built from): g_r = sum_k |J_o,rk| sqrt(Sigma_kk) over the variable
        parameters of the observation."""
        no = p.n_obs
        h, g = np.zeros((no, 2, 2)), np.zeros((no, 2))
        order = np.argsort(p.obs_pt, kind="stable")
        start = 0
        while start < no:
            pt = p.obs_pt[order[start]]
            end = start
            while end < no and p.obs_pt[order[end]] == pt:
                end += 1
            var_p = self.vp[pt] >= 0
            if var_p:
                A = self.sigma_t(pt)                                 # [n, 3]
                Tp, cols = self._t(pt)
                Spp = self.binv[self.vp[pt]] + Tp @ A[cols]
            for o in order[start:end]:
                v = self.vc[p.obs_cam[o]]
                Jc, Jp = self.J[o, :, :6], self.J[o, :, 6:]
                if v >= 0:
                    Scc = self.Sigma[6 * v:6 * v + 6, 6 * v:6 * v + 6]
                    h[o] += Jc @ Scc @ Jc.T
                    g[o] += np.abs(Jc) @ np.sqrt(np.diag(Scc))
                if var_p:
                    h[o] += Jp @ Spp @ Jp.T
                    g[o] += np.abs(Jp) @ np.sqrt(np.diag(Spp))
                if v >= 0 and var_p:
                    X = Jc @ (-A[6 * v:6 * v + 6]) @ Jp.T
                    h[o] += X + X.T
            start = end
        return h, g

    def n_params(self) -> int:
        return self.ref.n + 3 * int(self.ref.pt_var.sum())


def full_reference(oracle, p, ref=None) -> FullReference:
    """ref: the problem's covariance_ref.Reference if the caller has it."""
    import scipy.sparse as sp

    if ref is None:
        ref = R.reference(oracle, p, [])
    _, J, _, ok = oracle.linearize(p)
    assert ok
    n = ref.n
    vc = np.full(p.n_cams, -1)
    vc[ref.cam_var] = np.arange(ref.cam_var.sum())
    vp = np.full(p.n_pts, -1)
    vp[ref.pt_var] = np.arange(ref.pt_var.sum())
    q = 3 * int(ref.pt_var.sum())
    idx = np.flatnonzero(ref.cam_var)
    Sigma = ref.cam_cov[np.ix_(idx, idx)].transpose(0, 2, 1, 3).reshape(n, n)
    d = ref.H[n:, n:].tocoo()
    blocks = np.zeros((q // 3, 3, 3))
    blocks[d.row // 3, d.row % 3, d.col % 3] = d.data
    binv = np.linalg.inv(blocks) if q else blocks
    Hpp_inv = sp.bsr_matrix((binv, np.arange(q // 3), np.arange(q // 3 + 1)), shape=(q, q)).tocsr()
    T = (Hpp_inv @ ref.H[:n, n:].T.tocsr()).tocsr()
    return FullReference(ref, J, Sigma, T, binv, vc, vp)


def dense_check(full: FullReference, cam_pt, pt_pairs) -> float:
    """Largest disagreement (max |a - b| / sqrt(b_ii b_jj)) between the Schur
    route above and the inverse of the whole dense H, over the given (camera,
    point) and (point, point) requests with variable blocks."""
    Hd = full.ref.H.toarray()
    inv = np.linalg.inv(0.5 * (Hd + Hd.T))
    d = np.sqrt(np.diag(inv))
    n = full.ref.n
    worst = 0.0
    for c, p in cam_pt:
        if full.vc[c] < 0 or full.vp[p] < 0:
            continue
        r, s = slice(6 * full.vc[c], 6 * full.vc[c] + 6), slice(n + 3 * full.vp[p], n + 3 * full.vp[p] + 3)
        worst = max(worst, float((np.abs(full.cam_pt(c, p) - inv[r, s]) / np.outer(d[r], d[s])).max()))
    for p, q in pt_pairs:
        if full.vp[p] < 0 or full.vp[q] < 0:
            continue
        r, s = slice(n + 3 * full.vp[p], n + 3 * full.vp[p] + 3), slice(n + 3 * full.vp[q], n + 3 * full.vp[q] + 3)
        worst = max(worst, float((np.abs(full.pt_pt(p, q) - inv[r, s]) / np.outer(d[r], d[s])).max()))
    return worst


def pt_var_diag(full: FullReference, p) -> np.ndarray:
    return np.diag(full.pt_pt(p, p))


def cross_errors(full: FullReference, cam_pt, got_cp, pt_pairs, got_pq):
    """Worst block errors (covariance_ref.block_error) of the cross blocks
    whose two blocks are variable: (camera x point, point x point)."""
    pv = {}

    def pvar(p):
        if p not in pv:
            pv[p] = pt_var_diag(full, p)
        return pv[p]

    ecp = epq = 0.0
    for (c, p), blk in zip(cam_pt, got_cp):
        c, p = int(c), int(p)
        if full.vc[c] >= 0 and full.vp[p] >= 0:
            ecp = max(ecp, R.block_error(blk, full.cam_pt(c, p), full.cam_var_diag(c), pvar(p)))
    for (p, q), blk in zip(pt_pairs, got_pq):
        p, q = int(p), int(q)
        if full.vp[p] >= 0 and full.vp[q] >= 0:
            epq = max(epq, R.block_error(blk, full.pt_pt(p, q), pvar(p), pvar(q)))
    return ecp, epq


_CACHE: dict = {}


def case_full(oracle, name: str):
    """(problem, FullReference, (h, g)) of a shared problem of covariance_ref,
    computed once per process and never modified by the tests."""
    if name not in _CACHE:
        p, ref = R.case_reference(oracle, name)
        full = full_reference(oracle, p, ref)
        _CACHE[name] = (p, full, full.leverages(p))
    return _CACHE[name]
