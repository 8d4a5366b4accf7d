"""CPU reference and checker for the dense Cholesky + back substitution behind
DENSE_SCHUR (ba_debug_factor).  Never calls the HIP library; numpy only.

The kernels factor the (n+1) x n trapezoid A+ = [A; rhs^T] in 64-column blocks
into L+ = [L; z^T] (z = L^-1 rhs), keep the explicit inverses V_k of the
diagonal 64-blocks instead of the blocks themselves, and solve L^T y = z with
them.  The checks are backward errors with known bounds, so they do not depend
on the conditioning of A:

  factor_ratio  max over the lower trapezoid of
                |A+ - L+ L^T|_ij / (gamma_{n+1} ((|L+| |L^T|) + E)_ij),
                gamma_k = k u / (1 - k u), u = 2^-53, the diagonal blocks of L
                rebuilt as L_kk = V_k^-1 (assemble_L).  Higham (Accuracy and
                Stability of Numerical Algorithms, Thm 10.3) bounds the
                numerator of a Cholesky factor computed in ANY summation order
                by gamma_{n+1} (|L||L^T|)_ij; forming the product L+ L^T in
                float64 adds at most gamma_n of the same denominator, so a
                correct factor gives at most 2.  E is the term the explicit
                inverses need (below); without it correct factors fail.
  solve_error   |y - y*| / |y*| with L^T y* = z solved from the RETURNED factor
                in longdouble: the forward error of a triangular solve, bounded
                by ~ n u cond(L) (the tests allow 4 n u cond_2(L)).

Why E.  Thm 10.3 is about a factor whose diagonal blocks are the ones the
elimination produced and whose panels come from triangular solves.  Here the
diagonal block the kernels factored, L^_kk, never leaves the workgroup: what is
stored, and what every later operation uses, is V_k = fl(L^_kk^-1), and the
panels are products L_Ik = fl(A'_Ik V_k^T) with A'_Ik = fl(A_Ik - sum_{p<k}
L_Ip L_kp^T).  With L_kk := V_k^-1 (exact):
  panel rows   L_Ik L_kk^T = A'_Ik + d L_kk^T, |d| <= gamma_64 |A'_Ik| |V_k^T|,
               so |A - L L^T|_Ik <= gamma (B_Ik + B_Ik |V_k^T| |L_kk^T|) with
               B_Ik = |A_Ik| + sum_{p<k} |L_Ip| |L_kp|^T >= |A'_Ik|;
  the diagonal L^_kk = L_kk (I + F) with |F| <= gamma_64 |V_k| |L^_kk| (the
  block        residual of a triangular inverse by substitution), hence
               L^ L^^T - L_kk L_kk^T = L_kk (F + F^T) L_kk^T to first order, at
               most gamma (M X + X M^T) with M = |L_kk| |V_k|, X = |L_kk| |L_kk^T|.
So E_Ik = B_Ik M_k^T below the diagonal block and E_kk = M_k X_k + X_k M_k^T on
it.  M >= I entrywise: for a well-conditioned block E is a small multiple of
Higham's term.  Measured on a float64 model of the kernels' algorithm
(blocked_model; orders 6 .. 1542, kappa 1e2 and 1e10): at most 0.10 with E,
against up to 287 without it (e.g. 6.9 at n = 12, 22.8 at n = 258, both kappa
= 1e2: a near-zero L_i0 leaves Higham's denominator |L_i0| L_00 no room for
the normwise error of an inverted block).  One entry of L off by 1e-9 relative
still gives 99 or more (tests/test_cholesky_ref_cpu.py).
"""
from __future__ import annotations

import functools

import numpy as np

U = 2.0 ** -53
CB = 64


def gamma(k: int) -> float:
    return k * U / (1.0 - k * U)


def spd(n: int, kappa: float, seed: int) -> np.ndarray:
    """Q diag(logspace(0, log10 kappa, n)) Q^T, symmetrised; Q from the QR of a
    seeded normal matrix."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    d = np.logspace(0.0, np.log10(kappa), n)
    A = (Q * d) @ Q.T
    return 0.5 * (A + A.T)


def make_indefinite(A: np.ndarray, j: int) -> np.ndarray:
    """A with 2 L0[j,j]^2 taken off A[j,j] (L0 = cholesky(A)): pivots 0..j-1
    are unchanged and pivot j becomes -L0[j,j]^2."""
    L0 = np.linalg.cholesky(A)
    B = A.copy()
    B[j, j] -= 2.0 * L0[j, j] ** 2
    return B


def _tri_inverse(Vk: np.ndarray, dtype=np.float64) -> np.ndarray:
    """Inverse of a lower-triangular matrix in `dtype` (row-oriented forward
    substitution on the identity)."""
    b = Vk.shape[0]
    Vl = np.tril(Vk).astype(dtype)
    X = np.zeros((b, b), dtype)
    for i in range(b):
        row = -(Vl[i, :i] @ X[:i, :]) if i else np.zeros(b, dtype)
        row[i] += 1.0
        X[i] = row / Vl[i, i]
    return X


def _tri_inverse_ld(Vk: np.ndarray) -> np.ndarray:
    return _tri_inverse(Vk, np.longdouble)


def assemble_L(L_rows: np.ndarray, V: np.ndarray, n: int) -> np.ndarray:
    """The whole (n+1) x n factor: L_rows (what the kernels store: the tiles
    left of the diagonal 64-blocks, and row n = z) with the diagonal blocks
    L_kk = V_k^-1 filled in (inverted in longdouble, rounded to double).  Only
    the lower triangle of V_k's leading b x b part is read."""
    L = np.array(L_rows, dtype=np.float64, copy=True)
    assert L.shape == (n + 1, n)
    for k in range((n + CB - 1) // CB):
        s = k * CB
        b = min(CB, n - s)
        L[s:s + b, s:s + b] = np.tril(_tri_inverse_ld(V[k][:b, :b]).astype(np.float64))
        L[s:s + b, s + b:] = 0.0
    return L


def inverse_term(A: np.ndarray, rhs: np.ndarray, L: np.ndarray, V: np.ndarray) -> np.ndarray:
    """E of the module docstring, [n+1, n] (zero above the diagonal blocks)."""
    n = A.shape[0]
    Ap = np.abs(np.vstack([A, rhs[None, :]]))
    aL = np.abs(L)
    E = np.zeros((n + 1, n))
    for k in range((n + CB - 1) // CB):
        s = k * CB
        b = min(CB, n - s)
        e = s + b
        M = aL[s:e, s:e] @ np.abs(np.tril(V[k][:b, :b]))           # |L_kk| |V_k| >= I
        X = aL[s:e, s:e] @ aL[s:e, s:e].T
        E[s:e, s:e] = M @ X + X @ M.T
        B = Ap[e:, s:e] + aL[e:, :s] @ aL[s:e, :s].T
        E[e:, s:e] = B @ M.T
    return E


def factor_ratio(A: np.ndarray, rhs: np.ndarray, L: np.ndarray, V: np.ndarray | None = None) -> float:
    """See the module docstring.  L: [n+1, n] with its diagonal blocks (from
    assemble_L, or a factor that has them).  V: the explicit inverses the
    diagonal blocks were rebuilt from (None: L's diagonal blocks are the
    factor's own, Higham's denominator alone).  Only the lower triangle of A is
    read.  A non-finite factor gives inf."""
    n = A.shape[0]
    if not np.all(np.isfinite(L)):
        return float("inf")
    Ap = np.vstack([A, rhs[None, :]])
    Lt = L[:n]
    P = L @ Lt.T
    D = np.abs(L) @ np.abs(Lt).T
    if V is not None:
        D = D + inverse_term(A, rhs, L, V)
    num = np.abs(Ap - P)
    mask = np.vstack([np.tril(np.ones((n, n), bool)), np.ones((1, n), bool)])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(num == 0.0, 0.0, num / (gamma(n + 1) * D))
    return float(r[mask].max())


def solve_error(L: np.ndarray, z: np.ndarray, y: np.ndarray) -> tuple[float, float]:
    """(|y - y*|_2 / |y*|_2, cond_2(L)) with L^T y* = z by longdouble back
    substitution on the n x n factor L."""
    n = L.shape[1]
    Ll = L[:n].astype(np.longdouble)
    zl = np.asarray(z, np.longdouble)
    ys = np.zeros(n, np.longdouble)
    for i in range(n - 1, -1, -1):
        ys[i] = (zl[i] - Ll[i + 1:, i] @ ys[i + 1:]) / Ll[i, i]
    err = np.linalg.norm((np.asarray(y, np.longdouble) - ys).astype(np.float64)) / np.linalg.norm(ys.astype(np.float64))
    return float(err), float(np.linalg.cond(L[:n]))


def reference_solution(A: np.ndarray, rhs: np.ndarray) -> np.ndarray:
    """float64 solve + 6 steps of iterative refinement with the residual in
    longdouble."""
    Ainv = np.linalg.inv(A)
    Al, bl = A.astype(np.longdouble), rhs.astype(np.longdouble)
    x = (Ainv @ rhs).astype(np.longdouble)
    for _ in range(6):
        r = (bl - Al @ x).astype(np.float64)
        x = x + (Ainv @ r).astype(np.longdouble)
    return x.astype(np.float64)


def blocked_model(A: np.ndarray, rhs: np.ndarray) -> dict:
    """The kernels' algorithm in numpy float64, with the outputs of
    ba_debug_factor: right-looking over 64-column blocks, V_k = L_kk^-1
    explicit, L_Ik = A_Ik V_k^T (the rhs row included), A_IJ -= L_Ik L_Jk^T,
    then y_K = V_K^T (z_K - sum_{J>K} L_JK^T y_J).  The diagonal blocks of L
    are not stored."""
    n = A.shape[0]
    T = (n + CB - 1) // CB
    W = np.vstack([np.tril(A), rhs[None, :]])
    L = np.zeros((n + 1, n))
    V = np.zeros((T, CB, CB))
    ok = True
    for k in range(T):
        s = k * CB
        b = min(CB, n - s)
        e = s + b
        Akk = np.tril(W[s:e, s:e])
        Akk = Akk + np.tril(Akk, -1).T
        try:
            Lkk = np.linalg.cholesky(Akk)
        except np.linalg.LinAlgError:
            ok = False
            break
        Vk = _tri_inverse(Lkk)
        V[k] = np.eye(CB)
        V[k][:b, :b] = Vk
        L[e:, s:e] = W[e:, s:e] @ Vk.T
        P = L[e:, s:e]
        W[e:, e:] -= P @ P[:n - e].T
    z = L[n].copy()
    y = np.zeros(n)
    if ok:
        for K in range(T - 1, -1, -1):
            s = K * CB
            b = min(CB, n - s)
            e = s + b
            t = z[s:e] - L[e:n, s:e].T @ y[e:]
            y[s:e] = V[K][:b, :b].T @ t
    return {"L": L, "V": V, "y": y, "ok": ok, "n": n}


# ---------------------------------------------------------------------------
# shared inputs and references: computed once per process, returned read-only
# ---------------------------------------------------------------------------
def _frozen(a: np.ndarray) -> np.ndarray:
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def system(n: int, kappa: float, seed: int) -> tuple[np.ndarray, np.ndarray]:
    """(A, rhs): spd(n, kappa, seed) and a seeded normal right-hand side."""
    rhs = np.random.default_rng(seed + 0x5EED).standard_normal(n)
    return _frozen(spd(n, kappa, seed)), _frozen(rhs)


@functools.lru_cache(maxsize=None)
def system_reference(n: int, kappa: float, seed: int) -> np.ndarray:
    A, rhs = system(n, kappa, seed)
    return _frozen(reference_solution(A, rhs))


def check(A: np.ndarray, rhs: np.ndarray, out: dict) -> dict:
    """Every figure the tests bound, from the outputs of ba_debug_factor (or of
    blocked_model): factor_ratio, solve_error, cond_L and the assembled L."""
    n = A.shape[0]
    L = assemble_L(out["L"], out["V"], n)
    fr = factor_ratio(A, rhs, L, out["V"])
    se, cond_l = solve_error(L, L[n], out["y"])
    return {"factor_ratio": fr, "solve_error": se, "cond_L": cond_l, "L": L}
