"""ba_covariance_ex on the GPU against the CPU reference (covariance_full_ref.py
on top of covariance_ref.py: (J^T J)^-1 from the oracle's corrected Jacobian).

Cross blocks: e = max |got - ref| / sqrt(ref_ii ref_jj) over the entries of a
block, tolerance max(1e-12, 4 n eps cond2(S_ref)) (covariance_ref.tolerance()).

Leverages h_o = J_o Sigma J_o^T: per entry |got - ref|_rs <= (tolerance +
2e-11) g_r g_s with g_r = sum_k |J_o,rk| sqrt(Sigma_kk) from the reference: the
first-order bound |J| |dSigma| |J^T|, plus the 1e-11 relative parity of the
GPU's J with the oracle's, which enters twice.  g_r g_s <= 32 on these cases
(asserted).  The traces of all h_o must sum to the number of variable
parameters within the sum of the diagonal entries' tolerances; every h_o is
symmetric (bitwise: the kernel stores one off-diagonal value twice) with
eigenvalues in [-tol, 1 + tol], tol = tolerance + 2e-11 without the g factors.

Cov(p, q)^T and Cov(q, p) are bitwise equal for p != q: the kernel forms the
block of (min, max) and stores it transposed for p > q.  For p == q the block
is bitwise the marginal of ba_covariance, whose two triangles are summed in
different orders: symmetric to rounding only, checked within the tolerance.

Measured on an MI355X (every test prints its figures, "MEASURED ..."):

  case                              cam x pt   pt x pt    tolerance  leverage entry   sum tr(h) - N
                                                                     error / bound
  n24                               4.7e-15    1.2e-14    2.4e-12    6.7e-4           -1.1e-13 (N = 144)
  n132                              4.3e-14    3.7e-14    1.5e-10    1.0e-4           -6.8e-13 (1032)
  n192                              1.7e-14    1.7e-14    4.8e-10
  n1488                             1.6e-12    1.5e-12    7.2e-8     8.7e-7           6.5e-11 (16488)
  n24, one point with 80 obs.                                        6.7e-4           -4.5e-13 (144)
  n132, BA_WCOMPACT=0               4.1e-14    3.5e-14    1.5e-10    1.0e-4           -6.8e-13 (1032)
  72 cameras, all on every point    1.6e-13    1.6e-13    4.3e-9     5.1e-6           -2.3e-13 (870)
  n132 - camera 5 - point 3,
    constant points                 3.2e-15    8.5e-15    6.7e-12    5.7e-4           -1.3e-12 (894)
  n132, 37 shuffled observations                                     1.4e-5

The cross blocks sit four to five orders inside the tolerance, like the blocks
of ba_covariance; the leverages three to six orders inside their bound.
Eigenvalues of the h_o: 0 for two constant blocks, else 1.9e-4 ... 0.9926.
"""
import numpy as np
import pytest

import covariance_full_ref as F
import covariance_ref as R
from bundleadjustment_amd import Options, Solver, make_synthetic
from bundleadjustment_amd.problem import fix_camera
from bundleadjustment_amd._native import BAError

pytestmark = pytest.mark.gpu

INVALID, NO_PROBLEM, SINGULAR = 1, 4, 6
J_PARITY = 2e-11


def cross_requests(name, p):
    """(cam_pt [a, 2], pt_pairs [b, 2]) of a shared problem; the pairs end with
    the reversed copies of their first 50 and 20 pairs (q, q) of requested
    marginals."""
    rng = np.random.default_rng(23)
    _, points = R.case_requests(name)
    if name == "n24":
        c, q = np.meshgrid(np.arange(p.n_cams), np.arange(p.n_pts), indexing="ij")
        cam_pt = np.stack([c.ravel(), q.ravel()], 1)
        a, b = np.meshgrid(np.arange(p.n_pts), np.arange(p.n_pts), indexing="ij")
        pairs = np.stack([a.ravel(), b.ravel()], 1)
    elif name != "n1488":
        c, q = np.meshgrid(np.arange(p.n_cams), np.arange(p.n_pts), indexing="ij")
        cam_pt = np.stack([c.ravel(), q.ravel()], 1)
        pairs = rng.integers(0, p.n_pts, size=(2000, 2))
    else:
        cam_pt = np.stack([rng.integers(0, p.n_cams, 500), rng.integers(0, p.n_pts, 500)], 1)
        cam_pt[:4, 0] = [0, 1, 0, 1]                 # (the constant cameras)
        # half of the pairs share a camera: two points of one camera's observation list
        shared = []
        while len(shared) < 250:
            c = int(rng.integers(2, p.n_cams))
            seen = np.unique(p.obs_pt[p.obs_cam == c])
            if seen.size >= 2:
                shared.append(rng.choice(seen, size=2, replace=False))
        pairs = np.concatenate([np.array(shared), rng.integers(0, p.n_pts, size=(250, 2))])
    same = np.stack([points[:20], points[:20]], 1)
    pairs = np.concatenate([pairs, pairs[:50, ::-1], same])
    return cam_pt.astype(np.int32), pairs.astype(np.int32)


@pytest.mark.parametrize("name", ["n24", "n132", "n192", "n1488"])
def test_cross_blocks_match_reference(oracle_lib, name):
    p, full, _ = F.case_full(oracle_lib, name)
    ref = full.ref
    cam_pairs, points = R.case_requests(name)
    cam_pt, pairs = cross_requests(name, p)
    with Solver(0) as s:
        s.set_problem(p)
        out = s.covariance_ex(cam_pairs, points, cam_pt, pairs)
        base = s.covariance(cam_pairs, points)
    tol = ref.tolerance()
    ecp, epq = F.cross_errors(full, cam_pt, out["cam_pt_cov"], pairs, out["pt_pt_cov"])
    print(f"MEASURED {name}: n = {ref.n}, camera x point {ecp:.3e}, point x point {epq:.3e}, tolerance {tol:.3e}")
    assert ecp <= tol and epq <= tol
    # the base request: bitwise ba_covariance's output
    assert np.array_equal(out["cam_cov"], base[0]) and np.array_equal(out["pt_cov"], base[1])
    assert np.array_equal(out["leverage"], np.empty((0, 2, 2)))
    # constant cameras 0 and 1: exact zeros
    const = ~ref.cam_var[cam_pt[:, 0]]
    assert const.any() and np.all(out["cam_pt_cov"][const] == 0.0)
    assert np.all(np.abs(out["cam_pt_cov"][~const]).max(axis=(1, 2)) > 0.0)
    # Cov(p, q)^T == Cov(q, p), bitwise
    n0 = len(pairs) - 70
    assert np.array_equal(pairs[n0:n0 + 50], pairs[:50, ::-1])
    fwd, rev, diff = out["pt_pt_cov"][:50], out["pt_pt_cov"][n0:n0 + 50], pairs[:50, 0] != pairs[:50, 1]
    assert diff.any() and np.array_equal(rev[diff], fwd[diff].transpose(0, 2, 1))
    # (p == q is the marginal's own arithmetic, symmetric only to rounding)
    for blk in out["pt_cov"]:
        assert R.block_error(blk, blk.T, np.diag(blk), np.diag(blk)) <= tol
    # p == q: bitwise the marginal
    assert np.array_equal(out["pt_pt_cov"][n0 + 50:], out["pt_cov"][:20])


def check_leverages(tag, p, full, hg, got, obs=None):
    """got [l, 2, 2] for the observations obs (None: all, in order)."""
    h, g = hg
    if obs is not None:
        h, g = h[obs], g[obs]
    tol = full.tolerance() + J_PARITY
    gg = np.einsum("or,os->ors", g, g)
    assert gg.max() <= 32.0
    ratio = np.abs(got - h) / np.where(gg > 0.0, tol * gg, 1.0)
    assert np.all(got[gg == 0.0] == 0.0)           # no variable block: exact zeros
    ratio[gg == 0.0] = 0.0
    assert np.array_equal(got, got.transpose(0, 2, 1))
    ev = np.linalg.eigvalsh(got)
    print(f"MEASURED {tag}: {len(got)} leverages, worst entry error / bound {ratio.max():.3e} (bound factor {tol:.3e}), "
          f"max g_r g_s {gg.max():.3f}, eigenvalues [{ev.min():.3e}, {ev.max():.6f}]")
    assert ratio.max() <= 1.0
    assert ev.min() >= -tol and ev.max() <= 1.0 + tol
    if obs is None:
        trace, n_par = float(np.einsum("oii->", got)), full.n_params()
        bound = float(tol * np.einsum("orr->", gg))
        print(f"MEASURED {tag}: sum tr(h) - {n_par} = {trace - n_par:.3e} (bound {bound:.3e})")
        assert abs(trace - n_par) <= bound


@pytest.mark.parametrize("name", ["n24", "n132", "n1488"])
def test_leverages_match_reference(oracle_lib, name):
    p, full, hg = F.case_full(oracle_lib, name)
    with Solver(0) as s:
        s.set_problem(p)
        got = s.covariance_ex(leverage_obs="all")["leverage"]
        check_leverages(name, p, full, hg, got)
        if name == "n132":
            # a shuffled subset with repeats: the scatter through perm and the grouping by point
            rng = np.random.default_rng(5)
            obs = rng.choice(p.n_obs, size=30, replace=False)
            obs = rng.permutation(np.concatenate([obs, obs[:7]])).astype(np.int32)
            assert obs.size == 37
            sub = s.covariance_ex(leverage_obs=obs)["leverage"]
            assert np.array_equal(sub, got[obs])
            check_leverages("n132 subset", p, full, hg, sub, obs)


def test_leverages_of_a_point_with_80_observations(oracle_lib):
    p = R.make_case("n24").copy()
    pt = 7
    mine = np.flatnonzero(p.obs_pt == pt)
    assert 0 < mine.size < 80 and 80 % mine.size == 0
    rep = np.tile(mine, 80 // mine.size - 1)
    p.obs_cam = np.concatenate([p.obs_cam, p.obs_cam[rep]])
    p.obs_pt = np.concatenate([p.obs_pt, p.obs_pt[rep]])
    p.obs_uv = np.concatenate([p.obs_uv, p.obs_uv[rep]])
    assert np.count_nonzero(p.obs_pt == pt) == 80
    full = F.full_reference(oracle_lib, p)          # the reference of the same duplicated problem
    hg = full.leverages(p)
    with Solver(0) as s:
        s.set_problem(p)
        got = s.covariance_ex(leverage_obs="all")["leverage"]
    check_leverages("n24 + 80 observations of one point", p, full, hg, got)
    dup = np.flatnonzero(p.obs_pt == pt)
    assert np.all(np.einsum("oii->o", got[dup]) > 0.0)


def test_points_seen_by_more_than_64_cameras(oracle_lib):
    # 72 cameras on a ring, every point seen by (nearly) all of them: more than
    # 64 distinct cameras in a point's chunk sequence of k_cov_leverage, and
    # more than 64 terms per row in k_cov_cam_pt / k_cov_pt_pairs
    p = fix_camera(make_synthetic(72, 150, 72, seed=7), 1)
    per_pt = [np.unique(p.obs_cam[p.obs_pt == q]).size for q in range(p.n_pts)]
    assert min(per_pt) > 64
    full = F.full_reference(oracle_lib, p)
    hg = full.leverages(p)
    rng = np.random.default_rng(17)
    cam_pt = np.stack([rng.integers(0, p.n_cams, 200), rng.integers(0, p.n_pts, 200)], 1).astype(np.int32)
    pairs = rng.integers(0, p.n_pts, size=(200, 2)).astype(np.int32)
    with Solver(0) as s:
        s.set_problem(p)
        out = s.covariance_ex(cam_pt=cam_pt, pt_pairs=pairs, leverage_obs="all")
    check_leverages("72 cameras per point", p, full, hg, out["leverage"])
    ecp, epq = F.cross_errors(full, cam_pt, out["cam_pt_cov"], pairs, out["pt_pt_cov"])
    print(f"MEASURED 72 cameras per point: n = {full.ref.n}, camera x point {ecp:.3e}, point x point {epq:.3e}, "
          f"tolerance {full.tolerance():.3e}")
    assert ecp <= full.tolerance() and epq <= full.tolerance()


def test_leverages_with_the_18_double_w_records(oracle_lib, monkeypatch):
    monkeypatch.setenv("BA_WCOMPACT", "0")   # read when the step's W storage is chosen
    p, full, hg = F.case_full(oracle_lib, "n132")
    cam_pt, pairs = cross_requests("n132", p)
    with Solver(0) as s:
        s.set_problem(p)
        out = s.covariance_ex(cam_pt=cam_pt, pt_pairs=pairs, leverage_obs="all")
    check_leverages("n132 BA_WCOMPACT=0", p, full, hg, out["leverage"])
    ecp, epq = F.cross_errors(full, cam_pt, out["cam_pt_cov"], pairs, out["pt_pt_cov"])
    print(f"MEASURED n132 BA_WCOMPACT=0: camera x point {ecp:.3e}, point x point {epq:.3e}, "
          f"tolerance {full.tolerance():.3e}")
    assert ecp <= full.tolerance() and epq <= full.tolerance()


def test_constant_and_unobserved_blocks(oracle_lib):
    p = R.make_case("n132").copy()
    lost = 5                                       # a variable camera that loses every observation
    keep = p.obs_cam != lost
    cnt = np.bincount(p.obs_pt[keep], minlength=p.n_pts)
    keep &= cnt[p.obs_pt] >= 2                     # (a point seen once has a singular 3x3 block)
    gone = 3                                       # a variable point that loses every observation
    keep &= p.obs_pt != gone
    p.obs_cam, p.obs_pt, p.obs_uv = p.obs_cam[keep], p.obs_pt[keep], p.obs_uv[keep]
    p.pt_fixed = np.zeros(p.n_pts, np.uint8)
    p.pt_fixed[::7] = 1
    seen = np.bincount(p.obs_pt, minlength=p.n_pts) > 0
    assert not seen[gone] and not p.pt_fixed[gone]
    usable = np.flatnonzero(seen | (p.pt_fixed != 0)).astype(np.int32)
    cams = np.array([c for c in range(p.n_cams) if c != lost])
    c, q = np.meshgrid(cams, usable, indexing="ij")
    cam_pt = np.stack([c.ravel(), q.ravel()], 1).astype(np.int32)
    rng = np.random.default_rng(3)
    pairs = rng.choice(usable, size=(600, 2)).astype(np.int32)
    full = F.full_reference(oracle_lib, p)
    ref = full.ref
    hg = full.leverages(p)
    unseen = np.flatnonzero(~seen & (p.pt_fixed == 0))
    with Solver(0) as s:
        s.set_problem(p)
        for kw in ({"cam_pt": np.array([[lost, usable[1]]], np.int32)},):
            with pytest.raises(BAError) as e:
                s.covariance_ex(**kw)
            assert e.value.status == INVALID and f"camera {lost}" in str(e.value)
        assert gone in unseen
        for u in {gone, int(unseen[0])}:
            for kw in ({"cam_pt": np.array([[2, u]], np.int32)}, {"pt_pairs": np.array([[usable[1], u]], np.int32)},
                       {"pt_pairs": np.array([[u, u]], np.int32)}, {"points": np.array([u], np.int32)}):
                with pytest.raises(BAError) as e:
                    s.covariance_ex(**kw)
                assert e.value.status == INVALID and f"point {u}" in str(e.value), kw
        for kw in ({"cam_pt": np.array([[p.n_cams, 0]], np.int32)}, {"cam_pt": np.array([[2, p.n_pts]], np.int32)},
                   {"cam_pt": np.array([[-1, 0]], np.int32)}, {"pt_pairs": np.array([[0, p.n_pts]], np.int32)},
                   {"pt_pairs": np.array([[-1, 0]], np.int32)}, {"leverage_obs": np.array([p.n_obs], np.int32)},
                   {"leverage_obs": np.array([-1], np.int32)}):
            with pytest.raises(BAError) as e:
                s.covariance_ex(**kw)
            assert e.value.status == INVALID, kw
        out = s.covariance_ex(points=usable, cam_pt=cam_pt, pt_pairs=pairs, leverage_obs="all")
    tol = ref.tolerance()
    ecp, epq = F.cross_errors(full, cam_pt, out["cam_pt_cov"], pairs, out["pt_pt_cov"])
    print(f"MEASURED constant / unobserved: camera x point {ecp:.3e}, point x point {epq:.3e}, tolerance {tol:.3e}")
    assert ecp <= tol and epq <= tol
    const_cp = ~ref.cam_var[cam_pt[:, 0]] | (p.pt_fixed[cam_pt[:, 1]] != 0)
    assert (~ref.cam_var[cam_pt[:, 0]]).any() and (p.pt_fixed[cam_pt[:, 1]] != 0).any()
    assert np.all(out["cam_pt_cov"][const_cp] == 0.0)
    const_pq = (p.pt_fixed[pairs[:, 0]] != 0) | (p.pt_fixed[pairs[:, 1]] != 0)
    assert const_pq.any() and np.all(out["pt_pt_cov"][const_pq] == 0.0)
    check_leverages("constant / unobserved", p, full, hg, out["leverage"])
    # an observation of a constant camera: h = Jp Sigma_pp Jp^T; both blocks constant: zeros
    lev = out["leverage"]
    cam_const, pt_const = ~ref.cam_var[p.obs_cam], p.pt_fixed[p.obs_pt] != 0
    only_pt = np.flatnonzero(cam_const & ~pt_const)
    assert only_pt.size > 0
    where = {int(q): i for i, q in enumerate(usable)}
    Jp = full.J[only_pt][:, :, 6:]
    Spp = out["pt_cov"][[where[int(q)] for q in p.obs_pt[only_pt]]]
    want = np.einsum("ork,okl,osl->ors", Jp, Spp, Jp)
    g = hg[1][only_pt]
    assert np.all(np.abs(lev[only_pt] - want) <= (tol + J_PARITY) * np.einsum("or,os->ors", g, g))
    both = cam_const & pt_const
    assert both.any() and np.all(lev[both] == 0.0)


def test_errors_leave_the_context_usable(oracle_lib):
    p = R.make_case("n24")
    some = {"cam_pt": np.array([[2, 3]], np.int32), "leverage_obs": "all"}
    with Solver(0) as s:
        with pytest.raises(BAError) as e:
            s.covariance_ex(cam_pt=some["cam_pt"])
        assert e.value.status == NO_PROBLEM
        s.set_problem(p)
        assert s.solve(Options(max_num_iterations=3)).num_iterations > 0
    # the singular problem of test_covariance.py: every Jacobian entry exactly zero
    z = p.copy()
    z.K = z.K.copy()
    z.K[:, [0, 4, 6, 7]] = 0.0
    with Solver(0) as s:
        s.set_problem(z)
        with pytest.raises(BAError) as e:
            s.covariance_ex(**some)
        assert e.value.status == SINGULAR
        s.set_problem(p)
        out = s.covariance_ex(**some)
        assert np.all(np.isfinite(out["leverage"])) and np.all(np.isfinite(out["cam_pt_cov"]))
        assert s.solve(Options(max_num_iterations=3)).num_iterations > 0
    with Solver(0) as s:
        s.comm_init_host(lambda values, op: None, 1, 0)
        s.set_problem(p)
        with pytest.raises(BAError) as e:
            s.covariance_ex(**some)
        assert e.value.status == INVALID
        assert s.solve(Options(max_num_iterations=3)).num_iterations > 0


def log_values(log):
    return [{k: v for k, v in r.items() if k != "iteration_time_s"} for r in log]


def test_reproducible_and_leaves_the_context_unchanged(oracle_lib):
    p, full, _ = F.case_full(oracle_lib, "n132")
    cam_pairs, points = R.case_requests("n132")
    cam_pt, pairs = cross_requests("n132", p)
    req = dict(cam_pairs=cam_pairs, points=points, cam_pt=cam_pt, pt_pairs=pairs, leverage_obs="all")
    opts = Options(max_num_iterations=6)
    with Solver(0) as s:
        s.set_problem(p)
        s.solve(opts)
        alone = log_values(s.iteration_log())
    with Solver(0) as s:
        s.set_problem(p)
        r0, J0, c0 = s.linearize()
        cams0, pts0 = s.params()
        a = s.covariance_ex(**req)
        b = s.covariance_ex(**req)
        for k in a:
            assert a[k].size > 0 and np.array_equal(a[k], b[k]), k
        cams1, pts1 = s.params()
        assert np.array_equal(cams0, cams1) and np.array_equal(pts0, pts1)
        r1, J1, c1 = s.linearize()
        assert np.array_equal(r0, r1) and np.array_equal(J0, J1) and c0 == c1
        base = s.covariance(cam_pairs, points)
        assert np.array_equal(a["cam_cov"], base[0]) and np.array_equal(a["pt_cov"], base[1])
    with Solver(0) as s:
        s.set_problem(p)
        s.solve(opts)
        assert log_values(s.iteration_log()) == alone
        s.covariance_ex(**req)
        s.set_params(p.cams, p.pts)
        s.solve(opts)
        assert log_values(s.iteration_log()) == alone
