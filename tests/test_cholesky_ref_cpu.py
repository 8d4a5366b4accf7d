"""CPU tests of the Cholesky checker (tests/cholesky_ref.py) that the GPU tests
of ba_debug_factor rely on: it accepts numpy's own factor and a float64 model
of the kernels' blocked algorithm with wide margin, and it rejects a factor
with ONE entry off by 1e-9 relative — so a subtly wrong kernel cannot pass
tests/test_gpu_cholesky.py."""
import numpy as np
import pytest

import cholesky_ref as cr

ORDERS = (66, 192, 1542)
KAPPAS = (1e2, 1e10)


def numpy_factor(A, rhs):
    """numpy's own factor (its diagonal blocks as they are: Higham's bound
    alone applies), z and y by float64 substitution."""
    n = A.shape[0]
    L0 = np.linalg.cholesky(A)
    z = np.zeros(n)
    for i in range(n):
        z[i] = (rhs[i] - L0[i, :i] @ z[:i]) / L0[i, i]
    y = np.zeros(n)
    for i in range(n - 1, -1, -1):
        y[i] = (z[i] - L0[i + 1:, i] @ y[i + 1:]) / L0[i, i]
    return np.vstack([L0, z[None, :]]), y


@pytest.mark.parametrize("kappa", KAPPAS)
@pytest.mark.parametrize("n", ORDERS)
def test_checker_accepts_correct_factors_and_rejects_one_wrong_entry(n, kappa):
    A, rhs = cr.system(n, kappa, n)
    ref = cr.system_reference(n, kappa, n)
    # numpy's own factor
    L, y = numpy_factor(A, rhs)
    fr = cr.factor_ratio(A, rhs, L)
    se, cond_l = cr.solve_error(L, L[n], y)
    print(f"numpy n={n} kappa={kappa:g}: factor_ratio {fr:.3g} solve_error {se:.3g} cond_L {cond_l:.3g}")
    assert fr <= 0.5
    assert se <= 4.0 * n * cr.U * cond_l
    assert np.linalg.norm(y - ref) / np.linalg.norm(ref) <= 4.0 * n * cr.U * kappa
    # the model of the kernels' algorithm, through the path the GPU tests take
    out = cr.blocked_model(A, rhs)
    assert out["ok"]
    c = cr.check(A, rhs, out)
    print(f"model n={n} kappa={kappa:g}: factor_ratio {c['factor_ratio']:.3g} solve_error "
          f"{c['solve_error']:.3g} cond_L {c['cond_L']:.3g}")
    assert c["factor_ratio"] <= 0.5
    assert c["solve_error"] <= 4.0 * n * cr.U * c["cond_L"]
    assert np.linalg.norm(out["y"] - ref) / np.linalg.norm(ref) <= 4.0 * n * cr.U * kappa
    # one wrong entry of the model's factor, 1e-9 relative: in an off-diagonal
    # tile (the last tile row, block column 0) and in the rhs row
    for i, j in ((n - 1, 5), (n, 37)):
        bad = dict(out)
        bad["L"] = out["L"].copy()
        assert bad["L"][i, j] != 0.0
        bad["L"][i, j] *= 1.0 + 1e-9
        assert cr.check(A, rhs, bad)["factor_ratio"] > 2.0, (i, j)


def test_gpu_test_scenes_have_the_wanted_orders():
    """The scenes tests/test_gpu_cholesky.py builds only fix the order: every
    camera observed, camera 0 alone constant, so n = 6 nvc."""
    import test_gpu_cholesky as g
    for nvc in g.NVC:
        p = g.scene(nvc)
        assert p.n_cams == nvc + 1 and p.cam_fixed[0] == 1 and p.cam_fixed[1:].sum() == 0
        assert np.bincount(p.obs_cam, minlength=p.n_cams).min() > 0, nvc


def test_make_indefinite_moves_exactly_one_pivot():
    A, _ = cr.system(66, 1e2, 66)
    L0 = np.linalg.cholesky(A)
    for j in (0, 17, 65):
        B = cr.make_indefinite(A, j)
        # LDL^T pivots by plain elimination
        W = B.copy()
        piv = np.empty(66)
        for k in range(66):
            piv[k] = W[k, k]
            W[k + 1:, k + 1:] -= np.outer(W[k + 1:, k], W[k + 1:, k]) / W[k, k]
        assert np.allclose(piv[:j], L0[np.arange(j), np.arange(j)] ** 2, rtol=1e-10)
        assert piv[j] == pytest.approx(-L0[j, j] ** 2, rel=1e-8)
        assert not cr.blocked_model(B, np.ones(66))["ok"]


def test_assemble_L_ignores_what_the_kernels_do_not_write():
    """Stale upper entries of V (the persistent form leaves them unwritten) and
    of the L rows must not reach the assembled factor."""
    A, rhs = cr.system(192, 1e2, 192)
    out = cr.blocked_model(A, rhs)
    L = cr.assemble_L(out["L"], out["V"], 192)
    V = out["V"].copy()
    V[:, np.triu_indices(64, 1)[0], np.triu_indices(64, 1)[1]] = np.nan
    assert np.array_equal(L, cr.assemble_L(out["L"], V, 192))
