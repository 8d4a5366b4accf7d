"""numpy reference of the five-point essential solver of ba_two_view_ransac
(BA_TV_E_FIVE_POINT, include/ba_hip.h): the null space by numpy.linalg.svd,
the ten cubic constraints of E = xX + yY + zZ + W, the elimination of the ten
cubic monomials by numpy.linalg.solve, the 10x10 action matrix of the
multiplication by z on the monomials of degree <= 2 and its eigenvectors by
numpy.linalg.eig.  The device takes another route to the same solutions (a
Householder null space, Nister's tenth-degree polynomial in z, bisection), so
the two share no arithmetic beyond the constraint equations.  Everything is
batched over the hypotheses."""
from __future__ import annotations

from functools import lru_cache
from itertools import product

import numpy as np

import two_view_ref as R

FIVE_POINT = 1
BORDER_REL = 1e-6        # the borderline criterion on the eigenvalues (fixed by the yardstick)

# monomials (exponents of x, y, z): the ten cubics, then the basis of degree <= 2
CUBICS = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3)]
BASIS = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
MONO3 = CUBICS + BASIS
LIN = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


def _table(A, B, C):
    T = np.zeros((len(A), len(B), len(C)))
    for (i, a), (j, b) in product(enumerate(A), enumerate(B)):
        T[i, j, C.index(tuple(p + q for p, q in zip(a, b)))] = 1.0
    return T


T11 = _table(LIN, LIN, BASIS)          # linear x linear -> degree <= 2
T21 = _table(BASIS, LIN, MONO3)        # degree <= 2 x linear -> degree <= 3


def null_basis(b1: np.ndarray, b2: np.ndarray) -> np.ndarray:
    """b1, b2: (H, 5, 3) bearings (x, y, 1) -> (H, 4, 3, 3): X, Y, Z, W"""
    A = np.einsum("hni,hnj->hnij", b2, b1).reshape(len(b1), 5, 9)
    return np.linalg.svd(A)[2][:, 5:].reshape(len(b1), 4, 3, 3)


def constraints(N: np.ndarray) -> np.ndarray:
    """(H, 4, 3, 3) -> (H, 10, 20): 2 E E^T E - tr(E E^T) E (row-major) and det E over MONO3"""
    E = np.moveaxis(N, 1, -1)                                     # (H, 3, 3, 4): entry (i, j) as a linear polynomial
    EEt = np.einsum("hika,hlkb,abc->hilc", E, E, T11)
    tr = np.einsum("hiic->hc", EEt)
    L = 2.0 * EEt - np.eye(3)[None, :, :, None] * tr[:, None, None, :]
    C = np.einsum("hilc,hljd,cde->hije", L, E, T21).reshape(len(N), 9, 20)

    def m11(a, b):
        return np.einsum("ha,hb,abc->hc", a, b, T11)

    det = np.zeros((len(N), 20))
    for k in range(3):
        k1, k2 = (k + 1) % 3, (k + 2) % 3
        det += np.einsum("hc,hd,cde->he", m11(E[:, 1, k1], E[:, 2, k2]) - m11(E[:, 1, k2], E[:, 2, k1]), E[:, 0, k], T21)
    return np.concatenate([C, det[:, None]], 1)


def action_matrix(Rm: np.ndarray, var: int) -> np.ndarray:
    """(H, 10, 10): variable `var` (0 x, 1 y, 2 z) times basis monomial i, over the basis"""
    A = np.zeros((len(Rm), 10, 10))
    for i, b in enumerate(BASIS):
        m = tuple(p + (1 if k == var else 0) for k, p in enumerate(b))
        if m in CUBICS:
            A[:, i] = -Rm[:, CUBICS.index(m)]
        else:
            A[:, i, BASIS.index(m)] = 1.0
    return A


def solve(b1: np.ndarray, b2: np.ndarray):
    """The solutions of H five-point samples: (lam (H, 10) complex eigenvalues,
    E (H, 10, 3, 3) of the real ones (norm 1; zeros elsewhere), real (H, 10) bool).
    The description leaves the action variable open.  The eigenvalues of a
    non-normal matrix are as good as its eigenvector matrix is conditioned, so
    the reference forms the action matrices of z, x and y from the one
    elimination and keeps, per hypothesis, the one with the smallest cond(V)
    (ties: that order): its own error estimate decides, nothing else."""
    N = null_basis(b1, b2)
    M = constraints(N)
    Rm = np.linalg.solve(M[:, :, :10], M[:, :, 10:])              # cubic_i = -Rm[i] . basis
    lam = V = cond = None
    for var in (2, 0, 1):
        l, v = np.linalg.eig(action_matrix(Rm, var))              # A v = var v, v the basis at the solution
        with np.errstate(all="ignore"):
            c = np.nan_to_num(np.linalg.cond(v), nan=np.inf)
        if lam is None:
            lam, V, cond = l, v, c
        else:
            better = c < cond
            lam[better], V[better], cond[better] = l[better], v[better], c[better]
    real = lam.imag == 0.0
    with np.errstate(all="ignore"):
        xyz = (V[:, 6:9] / V[:, 9:10]).real                       # (H, 3, 10)
        E = np.einsum("hvs,hvij->hsij", xyz, N[:, :3]) + N[:, None, 3]
        E /= np.linalg.norm(E, axis=(2, 3), keepdims=True)
    real &= np.isfinite(E).all(axis=(2, 3))
    E[~real] = 0.0
    return lam, E, real


def borderline(lam: np.ndarray) -> np.ndarray:
    """(H,) bool: an eigenvalue barely complex, or two real ones barely apart"""
    out = np.zeros(len(lam), bool)
    for h, w in enumerate(lam):
        scale = np.maximum(1.0, np.abs(w))
        if np.any((w.imag != 0.0) & (np.abs(w.imag) <= BORDER_REL * scale)):
            out[h] = True
            continue
        r = np.sort(w.real[w.imag == 0.0])
        if len(r) > 1 and np.any(np.diff(r) <= BORDER_REL * np.maximum(1.0, np.abs(r[1:]))):
            out[h] = True
    return out


def sample_bearings(sc: R.Scene, smp: np.ndarray):
    """smp (H, 8): the bearings of the first five picks"""
    s = np.asarray(smp)[:, :5]
    return R.bearings(sc.uv1[s.reshape(-1)]).reshape(-1, 5, 3), R.bearings(sc.uv2[s.reshape(-1)]).reshape(-1, 5, 3)


def sample_residual(E: np.ndarray, b1: np.ndarray, b2: np.ndarray) -> np.ndarray:
    """max |b2^T E b1| over the five samples: E (H, S, 3, 3) -> (H, S)"""
    return np.max(np.abs(np.einsum("hni,hsij,hnj->hsn", b2, E, b1)), axis=2)


def constraint_residual(E: np.ndarray) -> np.ndarray:
    """|2 E E^T E - tr(E E^T) E| (Frobenius) of E (..., 3, 3)"""
    EEt = E @ np.swapaxes(E, -1, -2)
    tr = np.trace(EEt, axis1=-2, axis2=-1)[..., None, None]
    return np.linalg.norm(2.0 * EEt @ E - tr * E, axis=(-2, -1))


def sign_free_dist(E: np.ndarray, T: np.ndarray) -> np.ndarray:
    """E (..., 3, 3) against one matrix T"""
    return np.minimum(np.linalg.norm(E - T, axis=(-2, -1)), np.linalg.norm(E + T, axis=(-2, -1)))


SOLVER_NS = (8, 9, 64, 65)
SOLVER_H = 1000
MAX_BORDER = 0.01       # of a case's hypotheses


@lru_cache(maxsize=None)
def solver_reference(n: int, planar: bool):
    """Per hypothesis of the solver case R.solver_scene(n, planar): the sample,
    the reference's solutions and what the yardstick needs of them.  Computed
    once and shared; read-only."""
    sc = R.solver_scene(n, planar)
    smp = R.samples(0, n, SOLVER_H)
    b1, b2 = sample_bearings(sc, smp)
    lam, E, real = solve(b1, b2)
    truth = R.E_true(sc)
    res = np.where(real, sample_residual(E, b1, b2), 0.0)
    con = np.where(real, constraint_residual(E), 0.0)
    dist = np.where(real, sign_free_dist(E, truth), np.inf)
    near = np.argmin(dist, axis=1)
    out = dict(smp=smp, b1=b1, b2=b2, E=E, real=real, n_sol=real.sum(1), border=borderline(lam), res=res,
               con_worst=con.max(1), near=E[np.arange(SOLVER_H), near], near_dist=dist.min(1), truth=truth)
    for a in out.values():
        a.setflags(write=False)
    return out


def check_yardstick(n: int, planar: bool, n_sol: np.ndarray, E: np.ndarray, margin: float = 16.0):
    """The solver yardstick for the solutions (n_sol (H,), E (H, 10, 3, 3)) of
    any implementation on the case (n, planar).  Prints the worst figures,
    then asserts.  Returns them."""
    ref = solver_reference(n, planar)
    H = SOLVER_H
    n_sol = np.asarray(n_sol).reshape(H)
    E = np.asarray(E).reshape(H, 10, 3, 3)
    used = np.arange(10)[None, :] < n_sol[:, None]
    border = ref["border"]
    mism = int(np.sum((n_sol != ref["n_sol"]) & ~border))
    norms = np.linalg.norm(E, axis=(2, 3))
    res = np.where(used, sample_residual(E, ref["b1"], ref["b2"]), 0.0)
    con = np.where(used, constraint_residual(E), 0.0)
    con_ratio = float(np.max(con.max(1) / (margin * ref["con_worst"] + 1e-12)))
    near_ratio = 0.0
    if not planar:
        d = np.where(used, np.minimum(np.linalg.norm(E - ref["near"][:, None], axis=(2, 3)),
                                      np.linalg.norm(E + ref["near"][:, None], axis=(2, 3))), np.inf).min(1)
        has = np.isfinite(ref["near_dist"])
        near_ratio = float(np.max(d[has] / (margin * ref["near_dist"][has] + 1e-12))) if has.any() else 0.0
    fig = dict(borderline=int(border.sum()), n_sol_mismatch=mism, mean_solutions=float(n_sol.mean()),
               worst_sample_residual=float(res.max()), worst_constraint=float(con.max()),
               reference_worst_constraint=float(ref["con_worst"].max()), constraint_over_bound=con_ratio,
               nearest_over_bound=near_ratio)
    print(f"five-point n={n} planar={planar}: {fig}")
    assert border.sum() <= MAX_BORDER * H
    assert np.all((n_sol >= 0) & (n_sol <= 10))
    assert np.all(np.abs(norms[used] - 1.0) <= 1e-14) and np.all(E[~used] == 0.0)
    assert mism == 0
    assert res.max() <= margin * 1e-14
    assert con_ratio <= 1.0
    assert near_ratio <= 1.0
    return fig


# ---------------------------------------------------------------------------
# the vote of a whole five-point RANSAC in numpy (the reference end to end)
# ---------------------------------------------------------------------------
def ransac(sc: R.Scene, H: int = 1000, seed: int = 0, thr2: float = 1.0):
    """(E of the winner, its vote, votes kept by the essential projection)"""
    smp = R.samples(seed, len(sc.uv1), H)
    b1, b2 = sample_bearings(sc, smp)
    _, E, real = solve(b1, b2)
    best, win = -1, None
    for h in range(H):
        for s in np.flatnonzero(real[h]):
            d1, d2 = R.e_dist2(E[h, s], sc.uv1, sc.uv2)
            with np.errstate(invalid="ignore"):
                v = int(np.sum((d1 <= thr2) & (d2 <= thr2)))
            if v > best:
                best, win = v, E[h, s]
    Ep = R.project_e(win)[0]
    d1, d2 = R.e_dist2(Ep, sc.uv1, sc.uv2)
    return win, best, int(np.sum((d1 <= thr2) & (d2 <= thr2)))
