"""ba_covariance on the GPU against the CPU reference (covariance_ref.py:
(J^T J)^-1 from the oracle's corrected Jacobian, scipy.sparse + numpy).

Error measure: e = max |got - ref| / sqrt(ref_ii ref_jj) over the entries of a
block, the normalisers being the reference variances of the two coordinates.
Tolerance: max(1e-12, 4 n eps cond2(S_ref)), eps = 2^-53, from the
reference's own S: the first-order bound for an inverse obtained through a
Cholesky factor.  LM damping left in at the default radius 1e4 would perturb
S by 1e-4 of its diagonal, orders above it.

Problems: make_synthetic(..., seed=7), cameras 0 and 1 constant, covariances
at the initial estimate (covariance_ref.CASES).
"""
import numpy as np
import pytest

import covariance_ref as R
from bundleadjustment_amd import Options, Solver
from bundleadjustment_amd._native import BAError

pytestmark = pytest.mark.gpu

INVALID, NO_PROBLEM, SINGULAR = 1, 4, 6


def check_case(oracle_lib, name):
    p, ref = R.case_reference(oracle_lib, name)
    pairs, points = R.case_requests(name)
    with Solver(0) as s:
        s.set_problem(p)
        cam_cov, pt_cov = s.covariance(pairs, points)
    tol = ref.tolerance()
    ec, ep = R.cam_errors(cam_cov, pairs, ref), R.pt_errors(pt_cov, points, ref)
    print(f"{name}: n = {ref.n}, cameras {ec:.3e}, points {ep:.3e}, tolerance {tol:.3e}")
    assert ec <= tol and ep <= tol
    const = ~(ref.cam_var[pairs[:, 0]] & ref.cam_var[pairs[:, 1]])
    assert const.any() and np.all(cam_cov[const] == 0.0)   # cameras 0 and 1: exact zeros
    return cam_cov, pt_cov


@pytest.mark.parametrize("name", list(R.CASES))
def test_covariance_matches_reference(oracle_lib, name):
    check_case(oracle_lib, name)


@pytest.mark.parametrize("name", ["n132", "n408"])
def test_covariance_with_the_per_step_factorisation(oracle_lib, monkeypatch, name):
    monkeypatch.setenv("BA_CHOL_PERSIST", "0")   # read when the dense structures are built
    check_case(oracle_lib, name)


def test_constant_and_unobserved_blocks(oracle_lib):
    p = R.make_case("n132").copy()
    lost = 5                                       # a variable camera that loses every observation
    keep = p.obs_cam != lost
    cnt = np.bincount(p.obs_pt[keep], minlength=p.n_pts)
    keep &= cnt[p.obs_pt] >= 2                     # (a point seen once has a singular 3x3 block)
    p.obs_cam, p.obs_pt, p.obs_uv = p.obs_cam[keep], p.obs_pt[keep], p.obs_uv[keep]
    p.pt_fixed = np.zeros(p.n_pts, np.uint8)
    p.pt_fixed[::7] = 1
    seen = np.bincount(p.obs_pt, minlength=p.n_pts) > 0
    points = np.flatnonzero(seen | (p.pt_fixed != 0)).astype(np.int32)
    cams = np.array([c for c in range(p.n_cams) if c != lost])
    i, j = np.meshgrid(cams, cams, indexing="ij")
    pairs = np.stack([i.ravel(), j.ravel()], 1).astype(np.int32)
    ref = R.reference(oracle_lib, p, points)
    assert not ref.cam_var[lost] and ref.n == 6 * (p.n_cams - 3)
    with Solver(0) as s:
        s.set_problem(p)
        with pytest.raises(BAError) as e:
            s.covariance(np.array([[2, lost]], np.int32), None)
        assert e.value.status == INVALID and f"camera {lost}" in str(e.value)
        unseen = np.flatnonzero(~seen & (p.pt_fixed == 0))
        if unseen.size:
            with pytest.raises(BAError) as e:
                s.covariance(np.zeros((0, 2), np.int32), unseen[:1])
            assert e.value.status == INVALID and f"point {unseen[0]}" in str(e.value)
        cam_cov, pt_cov = s.covariance(pairs, points)
    tol = ref.tolerance()
    ec, ep = R.cam_errors(cam_cov, pairs, ref), R.pt_errors(pt_cov, points, ref)
    print(f"constant / unobserved: cameras {ec:.3e}, points {ep:.3e}, tolerance {tol:.3e}")
    assert ec <= tol and ep <= tol
    const_pair = ~(ref.cam_var[pairs[:, 0]] & ref.cam_var[pairs[:, 1]])
    assert np.all(cam_cov[const_pair] == 0.0)
    const_pt = p.pt_fixed[points] != 0
    assert const_pt.any() and np.all(pt_cov[const_pt] == 0.0)
    assert np.all(np.einsum("kii->ki", pt_cov[~const_pt]) > 0.0)


def log_values(log):
    return [{k: v for k, v in r.items() if k != "iteration_time_s"} for r in log]


def test_reproducible_and_leaves_the_context_unchanged(oracle_lib):
    p, ref = R.case_reference(oracle_lib, "n132")
    pairs, points = R.case_requests("n132")
    opts = Options(max_num_iterations=6)
    with Solver(0) as s:
        s.set_problem(p)
        s.solve(opts)
        alone = log_values(s.iteration_log())
    with Solver(0) as s:
        s.set_problem(p)
        c0, p0 = s.params()
        a = s.covariance(pairs, points)
        b = s.covariance(pairs, points)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        c1, p1 = s.params()
        assert np.array_equal(c0, c1) and np.array_equal(p0, p1)
        s.solve(opts)
        assert log_values(s.iteration_log()) == alone
        s.set_params(p.cams, p.pts)
        s.covariance(pairs, points)
        s.solve(opts)
        assert log_values(s.iteration_log()) == alone
    cam_cov = a[0].reshape(p.n_cams, p.n_cams, 6, 6)
    tol = ref.tolerance()
    for i in range(2, p.n_cams):
        assert np.linalg.eigvalsh(0.5 * (cam_cov[i, i] + cam_cov[i, i].T)).min() > 0.0
        vi = np.diag(ref.cam_cov[i, i])
        for j in range(2, p.n_cams):
            assert R.block_error(cam_cov[i, j], cam_cov[j, i].T, vi, np.diag(ref.cam_cov[j, j])) <= tol
    for blk in a[1]:
        assert np.linalg.eigvalsh(0.5 * (blk + blk.T)).min() > 0.0


def test_covariance_at_the_minimum_after_a_solve(oracle_lib):
    p = R.make_case("n132")
    pairs, points = R.case_requests("n132")
    with Solver(0) as s:
        s.set_problem(p)
        s.solve(Options(max_num_iterations=20))
        cams, pts = s.params()
        cam_cov, pt_cov = s.covariance(pairs, points)
    q = p.copy()
    q.cams, q.pts = cams, pts
    ref = R.reference(oracle_lib, q, points)
    tol = ref.tolerance()
    ec, ep = R.cam_errors(cam_cov, pairs, ref), R.pt_errors(pt_cov, points, ref)
    print(f"after a solve: cond2(S) = {ref.cond_S:.3e}, cameras {ec:.3e}, points {ep:.3e}, tolerance {tol:.3e}")
    assert ref.cond_S < 1e6
    assert ec <= tol and ep <= tol


def test_errors_leave_the_context_usable(oracle_lib):
    p = R.make_case("n24")
    with Solver(0) as s:
        with pytest.raises(BAError) as e:
            s.covariance(np.array([[2, 2]], np.int32), None)
        assert e.value.status == NO_PROBLEM
        s.set_problem(p)
        for bad in (np.array([[0, p.n_cams]], np.int32), np.array([[-1, 0]], np.int32)):
            with pytest.raises(BAError) as e:
                s.covariance(bad, None)
            assert e.value.status == INVALID
        with pytest.raises(BAError) as e:
            s.covariance(None, np.array([p.n_pts], np.int32))
        assert e.value.status == INVALID
        assert s.solve(Options(max_num_iterations=3)).num_iterations > 0
    # a deterministic singular input: fx = fy = 0 (and cx = cy = 0: with a
    # principal point left in, (cx z) / z leaves 1e-15 of rounding in J) makes
    # every Jacobian entry exactly zero, so the first point pivot (and every
    # other) is zero
    z = p.copy()
    z.K = z.K.copy()
    z.K[:, [0, 4, 6, 7]] = 0.0
    _, J, _, ok = oracle_lib.linearize(z)
    assert ok and np.all(J == 0.0)
    with Solver(0) as s:
        s.set_problem(z)
        with pytest.raises(BAError) as e:
            s.covariance(None, np.arange(4, dtype=np.int32))
        assert e.value.status == SINGULAR
        s.solve(Options(max_num_iterations=3))     # (nothing to minimise; it must return)
        s.set_problem(p)
        cam_cov, _ = s.covariance()
        assert np.all(np.isfinite(cam_cov)) and np.all(np.einsum("kii->ki", cam_cov[2:]) > 0.0)
        assert s.solve(Options(max_num_iterations=3)).num_iterations > 0
    with Solver(0) as s:
        s.comm_init_host(lambda values, op: None, 1, 0)
        s.set_problem(p)
        with pytest.raises(BAError) as e:
            s.covariance()
        assert e.value.status == INVALID
        assert s.solve(Options(max_num_iterations=3)).num_iterations > 0
