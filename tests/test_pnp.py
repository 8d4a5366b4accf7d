"""GPU tests for ba_pnp_ransac / ba_pnp_hypotheses against the numpy reference
(tests/pnp_ref.py): the pinned sampler, the device P3P on noise-free scenes,
the vote end to end, the refinement against solve_pose_batch bit for bit, the
prior, mixed batches, the context / staging contract and the error contract.

Measured on the device (MI355X), noise-free scenes n in {7, 64, 65, 257}, 1000
samples each: worst distance to the truth 1.7e-13,
2.5e-11, 1.7e-11, 4.3e-12 (reference 3.1e-11), worst sample reprojection
4.4e-12, 2.9e-11, 2.0e-10, 2.9e-10 px (reference 4.9e-10 px)."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import pnp_ref as R
from bundleadjustment_amd import Options, Solver, make_synthetic
from bundleadjustment_amd import _native as N
from bundleadjustment_amd._native import BAError

pytestmark = pytest.mark.gpu

MARGIN = 16.0      # a different root-finder at the same conditioning (see test_pnp_cpu.py)
THR = 8.0
SHAPES = [(7, 0.0, 64), (9, 0.3, 65), (64, 0.3, 256), (65, 0.6, 1000), (257, 0.5, 1000)]
SUMM_FIELDS = ["initial_cost", "final_cost", "num_iterations", "num_successful_steps", "num_unsuccessful_steps",
               "termination_type"]


@pytest.fixture(scope="module")
def solver():
    s = Solver(0)
    yield s
    s.close()


def batch_of(scenes, priors=None):
    """(obs_offset, cams, K, pts, obs_uv) of a list of scenes; priors: one [w, t] per scene or None."""
    off = np.concatenate([[0], np.cumsum([len(s.pts) for s in scenes])]).astype(np.int32)
    cams = None if priors is None else np.array(priors, np.float64).reshape(len(scenes), 6)
    K = np.stack([s.K for s in scenes]).astype(np.float32)
    pts = np.concatenate([s.pts for s in scenes]).reshape(-1, 3)
    uv = np.concatenate([s.uv for s in scenes]).reshape(-1, 2).astype(np.float32)
    return off, cams, K, pts, uv


@lru_cache(maxsize=None)
def e2e_scene(n, frac):
    return R.scene(n, frac, 0.5, 11 + n)


@lru_cache(maxsize=None)
def e2e_vote(n, frac, H):
    sc = e2e_scene(n, frac)
    return R.vote(sc.K, sc.pts, sc.uv, H, seed=0, thr=THR)


def summ_tuple(s):
    return tuple(getattr(s, f) for f in SUMM_FIELDS)


def result_bits(cams, inl, res, i, sl):
    r = res[i]
    return (cams[i].tobytes(), inl[sl].tobytes(), r.status, r.n_inliers, r.n_inliers_ransac, r.best_hypothesis,
            r.cam_ransac.tobytes(), summ_tuple(r.refine))


# ---------------------------------------------------------------------------
# 1. sampler
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 7, 64, 65])
def test_sampler_equals_the_reference(solver, n):
    sc = R.scene(n, 0.0, 0.0, 5)
    for seed in (0, 99):
        for use_prior in (0, 1):
            b = batch_of([sc], [sc.cam])
            for h0 in (0, 63, 64):
                hyp = solver.pnp_hypotheses(*b, 0, h0, 70, use_prior=use_prior, max_hypotheses=200, seed=seed)
                want = R.samples(seed, n, h0 + 70, bool(use_prior), h0=h0)
                assert np.array_equal(hyp["sample"], want), (seed, use_prior, h0)
                if use_prior and h0 == 0:
                    assert hyp["n_sol"][0] == 1 and np.all(hyp["sample"][0] == -1)
                    assert np.allclose(hyp["R"][0, 0], sc.R, atol=1e-15) and np.array_equal(hyp["t"][0, 0], sc.t)
                    assert hyp["count"][0, 0] == n


# ---------------------------------------------------------------------------
# 2. solver
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SOLVER_NS)
def test_solver_finds_the_truth_and_counts_like_numpy(solver, n):
    """Every returned solution is a rotation with positive sample depths and
    reprojects its sample within 16 x the reference's worst; the truth is among
    the solutions of EVERY hypothesis within 16 x the reference's worst; the
    counts equal the predicate in numpy at the returned (R, t).
    Measured device values: DESIGN.md section 20."""
    wd_ref, wr_ref = R.yardstick()
    sc = R.solver_scene(n)
    H = R.SOLVER_H
    hyp = solver.pnp_hypotheses(*batch_of([sc]), 0, 0, H, use_prior=0, max_hypotheses=H, threshold_px=THR)
    assert np.array_equal(hyp["sample"], R.samples(0, n, H, False))
    ns, Rm, t, cnt = hyp["n_sol"], hyp["R"], hyp["t"], hyp["count"]
    assert ns.min() >= 1 and ns.max() <= 4
    valid = np.arange(4)[None, :] < ns[:, None]
    assert np.all(Rm[~valid] == 0.0) and np.all(t[~valid] == 0.0) and np.all(cnt[~valid] == 0)
    Rv, tv = Rm[valid], t[valid]
    assert np.max(np.abs(np.einsum("kij,klj->kil", Rv, Rv) - np.eye(3))) <= 1e-12
    assert np.max(np.abs(np.linalg.det(Rv) - 1.0)) <= 1e-12
    Km = sc.K.astype(np.float64).reshape(3, 3).T
    uv = sc.uv.astype(np.float64)
    # every solution against every point: the predicate
    p = np.einsum("hjrc,nc->hjnr", Rm, sc.pts) + t[:, :, None, :]
    q = p @ Km.T
    with np.errstate(divide="ignore", invalid="ignore"):
        e2 = (q[..., 0] / q[..., 2] - uv[:, 0]) ** 2 + (q[..., 1] / q[..., 2] - uv[:, 1]) ** 2
    want = np.sum((q[..., 2] > 0.0) & (e2 <= THR * THR), axis=2) * valid
    assert np.array_equal(cnt, want)
    # the sample: depth and reprojection; the truth
    smp = hyp["sample"]
    hh = np.arange(H)[:, None, None]
    zs = p[hh, np.arange(4)[None, :, None], smp[:, None, :], 2]
    assert np.all(zs[valid] > 0.0)
    es = np.sqrt(e2[hh, np.arange(4)[None, :, None], smp[:, None, :]])
    wr = float(np.max(es[valid]))
    dist = np.maximum(np.max(np.abs(Rm - sc.R), axis=(2, 3)), np.max(np.abs(t - sc.t), axis=2))
    dist[~valid] = np.inf
    wd = float(np.max(np.min(dist, axis=1)))
    print(f"n = {n}: device worst distance to the truth {wd:.3g} (reference {wd_ref:.3g}), worst sample "
          f"reprojection {wr:.3g} px (reference {wr_ref:.3g}), solutions {np.bincount(ns, minlength=5)[1:]}")
    assert wr <= MARGIN * wr_ref
    assert wd <= MARGIN * wd_ref


# ---------------------------------------------------------------------------
# 3. end to end, 4. refinement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,frac,H", SHAPES)
def test_end_to_end_vote_and_refinement(solver, n, frac, H):
    sc, v = e2e_scene(n, frac), e2e_vote(n, frac, H)
    # the conditions, on the reference first
    assert np.array_equal(v.consensus, sc.inlier) and v.best_count == int(sc.inlier.sum())
    assert v.margin > 1e-6, v.margin
    b = batch_of([sc])
    opts = Options(max_num_iterations=20)
    cams, inl, res = solver.pnp_ransac(*b, use_prior=0, max_hypotheses=H, threshold_px=THR, options=opts)
    r = res[0]
    assert r.status == N.PNP_OK and r.best_hypothesis == v.best_h
    cons = R.inliers_cam(r.cam_ransac, sc.K, sc.pts, sc.uv, THR)
    assert np.array_equal(cons, sc.inlier) and r.n_inliers_ransac == int(cons.sum())
    # the same solution of the same sample (distinct P3P solutions are orders of magnitude further apart)
    assert np.max(np.abs(r.cam_ransac - v.cam_ransac)) <= 1e-6
    # refinement: solve_pose_batch on the consensus subset from cam_ransac, bit for bit
    k = int(cons.sum())
    want, ws = solver.solve_pose_batch(np.array([0, k], np.int32), r.cam_ransac[None], sc.K[None], sc.pts[cons],
                                       sc.uv[cons], opts)
    assert cams[0].tobytes() == want[0].tobytes()
    assert summ_tuple(r.refine) == summ_tuple(ws[0]) and r.refine.termination_type != "FAILURE"
    assert np.array_equal(inl, R.inliers_cam(cams[0], sc.K, sc.pts, sc.uv, THR)) and r.n_inliers == int(inl.sum())
    # without refinement: cams_out is cam_ransac, the mask the consensus
    cams0, inl0, res0 = solver.pnp_ransac(*b, use_prior=0, max_hypotheses=H, threshold_px=THR, refine=0)
    assert cams0[0].tobytes() == r.cam_ransac.tobytes() == res0[0].cam_ransac.tobytes()
    assert np.array_equal(inl0, cons) and res0[0].n_inliers == res0[0].n_inliers_ransac == k
    assert summ_tuple(res0[0].refine) == (0.0, 0.0, 0, 0, 0, "CONVERGENCE") and res0[0].refine.total_time_s == 0.0


# ---------------------------------------------------------------------------
# 5. prior
# ---------------------------------------------------------------------------
def test_prior_is_hypothesis_zero_and_a_bad_prior_is_survived(solver):
    sc = R.scene(64, 0.3, 0.5, 75)
    rng = np.random.default_rng(8)
    near = sc.cam + 1e-3 * rng.normal(size=6)
    b = batch_of([sc], [near])
    cams, inl, res = solver.pnp_ransac(*b, max_hypotheses=1, refine=0)
    r = res[0]
    assert r.status == N.PNP_OK and r.best_hypothesis == 0
    assert r.cam_ransac.tobytes() == near.tobytes() == cams[0].tobytes()
    cons = R.inliers_cam(near, sc.K, sc.pts, sc.uv, THR)
    assert np.array_equal(inl, cons) and r.n_inliers_ransac == int(cons.sum())
    # a prior 0.5 rad from the truth
    axis = rng.normal(size=3)
    far = sc.cam.copy()
    far[:3] += 0.5 * axis / np.linalg.norm(axis)
    b = batch_of([sc], [far])
    cams, inl, res = solver.pnp_ransac(*b)
    assert res[0].status == N.PNP_OK and res[0].best_hypothesis > 0
    assert np.array_equal(inl, sc.inlier) and res[0].n_inliers == int(sc.inlier.sum())
    assert np.max(np.abs(cams[0] - sc.cam)) < 0.05
    # for the record (no assertion): the local LM alone from that prior
    lm, ls = solver.solve_pose_batch(*b)
    n_lm = int(R.inliers_cam(lm[0], sc.K, sc.pts, sc.uv, THR).sum())
    print(f"bad prior: pnp_ransac |cam - truth| = {np.max(np.abs(cams[0] - sc.cam)):.3g} with {int(inl.sum())} inliers; "
          f"solve_pose_batch alone |cam - truth| = {np.max(np.abs(lm[0] - sc.cam)):.3g} with {n_lm} of "
          f"{int(sc.inlier.sum())} true inliers within {THR} px ({ls[0].termination_type})")


# ---------------------------------------------------------------------------
# 6. mixed batch
# ---------------------------------------------------------------------------
def mixed_scenes():
    good = [R.scene(n, 0.0 if n == 7 else 0.3, 0.5, 200 + n) for n in (7, 64, 65, 257)]
    few = [R.scene(7, 0.0, 0.5, 300 + k) for k in (0, 3, 6)]
    for s, k in zip(few, (0, 3, 6)):
        s.pts, s.uv, s.inlier = s.pts[:k], s.uv[:k], s.inlier[:k]
    junk = R.scene(12, 1.0, 0.5, 2)
    return good, few, junk


def test_mixed_batch_statuses_and_independence(solver):
    good, few, junk = mixed_scenes()
    order = [good[0], few[0], good[1], few[1], good[2], few[2], junk, good[3]]
    rng = np.random.default_rng(9)
    priors = [s.cam + 0.05 * rng.normal(size=6) for s in order]
    # the reference: 12 pure outliers hold no model of 6
    vj = R.vote(junk.K, junk.pts, junk.uv, 1000, prior=priors[6])
    assert vj.best_count < 6 and vj.margin > 1e-6
    b = batch_of(order, priors)
    off = b[0]
    cams, inl, res = solver.pnp_ransac(*b)
    cams2, inl2, res2 = solver.pnp_ransac(*b)
    sl = [slice(off[i], off[i + 1]) for i in range(len(order))]
    bits = [result_bits(cams, inl, res, i, sl[i]) for i in range(len(order))]
    assert bits == [result_bits(cams2, inl2, res2, i, sl[i]) for i in range(len(order))]
    assert [r.status for r in res] == [N.PNP_OK, N.PNP_FEW_POINTS, N.PNP_OK, N.PNP_FEW_POINTS, N.PNP_OK,
                                       N.PNP_FEW_POINTS, N.PNP_NO_MODEL, N.PNP_OK]
    for i in (1, 3, 5, 6):
        r = res[i]
        assert cams[i].tobytes() == priors[i].tobytes() == r.cam_ransac.tobytes()
        assert not inl[sl[i]].any() and (r.n_inliers, r.n_inliers_ransac, r.best_hypothesis) == (0, 0, -1)
        assert summ_tuple(r.refine) == (0.0, 0.0, 0, 0, 0, "CONVERGENCE")
    for i in (0, 2, 4, 7):
        assert np.array_equal(inl[sl[i]], order[i].inlier), i
    # each good problem alone, and the batch in another order
    for i in (0, 2, 4, 7):
        c1, i1, r1 = solver.pnp_ransac(*batch_of([order[i]], [priors[i]]))
        assert result_bits(c1, i1, r1, 0, slice(None)) == bits[i], i
    perm = [7, 6, 0, 5, 4, 1, 2, 3]
    bp = batch_of([order[j] for j in perm], [priors[j] for j in perm])
    cp, ip, rp = solver.pnp_ransac(*bp)
    for k, j in enumerate(perm):
        assert result_bits(cp, ip, rp, k, slice(bp[0][k], bp[0][k + 1])) == bits[j], j
    # without a prior the failed problems return zeros
    b0 = batch_of(order)
    c0, i0, r0 = solver.pnp_ransac(*b0, use_prior=0)
    assert [r.status for r in r0] == [r.status for r in res]
    for i in (1, 3, 5, 6):
        assert not c0[i].any() and not r0[i].cam_ransac.any() and not i0[sl[i]].any() and r0[i].best_hypothesis == -1
    for i in (0, 2, 4, 7):
        assert np.array_equal(i0[sl[i]], order[i].inlier), i


# ---------------------------------------------------------------------------
# 7. context and staging
# ---------------------------------------------------------------------------
def test_solve_is_untouched_by_a_pnp_in_between(solver):
    p = make_synthetic(6, 300, 4, seed=31)
    sc = R.scene(64, 0.3, 0.5, 75)
    b = batch_of([sc], [sc.cam])
    fields = ["iteration", "step_is_valid", "step_is_successful", "cost", "cost_change", "gradient_max_norm",
              "gradient_norm", "step_norm", "relative_decrease", "trust_region_radius", "model_cost_change"]

    def solve(between):
        solver.set_problem(p)
        if between:
            solver.pnp_ransac(*b)
        solver.solve(Options(max_num_iterations=6))
        cams, pts = solver.params()
        return [[r[f] for f in fields] for r in solver.iteration_log()], cams, pts

    log0, c0, x0 = solve(False)
    log1, c1, x1 = solve(True)
    assert log0 == log1 and c0.tobytes() == c1.tobytes() and x0.tobytes() == x1.tobytes()
    solver.set_problem(p)
    solver.solve(Options(max_num_iterations=6))
    solver.pnp_ransac(*b)
    solver.pnp_hypotheses(*b, 0, 0, 64)
    c2, x2 = solver.params()
    assert c2.tobytes() == c0.tobytes() and x2.tobytes() == x0.tobytes()


def test_staging_arenas_grow_shrink_and_interleave_bitwise():
    """One context through pnp small -> large -> small interleaved with pose
    batches, a triangulation and the inspection entry: every result equals,
    bit for bit, the same call on a fresh context."""
    import triangulate_ref as T

    small = batch_of([R.scene(9, 0.3, 0.5, 20)], [R.scene(9, 0.3, 0.5, 20).cam])
    ls = [R.scene(40 + 13 * i, 0.3, 0.5, 400 + i) for i in range(12)]
    large = batch_of(ls, [s.cam for s in ls])
    tb = T.scene(2, 2, 11)
    opts = Options(max_num_iterations=10)

    def pnp(b, **kw):
        def call(s):
            cams, inl, res = s.pnp_ransac(*b, options=opts, **kw)
            off = b[0]
            return [result_bits(cams, inl, res, i, slice(off[i], off[i + 1])) for i in range(len(off) - 1)]
        return call

    def pose(b):
        def call(s):
            out, summ = s.solve_pose_batch(*b, opts)
            return [out.tobytes(), [summ_tuple(x) for x in summ]]
        return call

    def tri(s):
        pts, status, _ = s.triangulate(tb.extr, tb.K, tb.obs_offset, tb.obs_cam, tb.obs_uv, cam_center=tb.cam_center)
        return [pts.tobytes(), status.tobytes()]

    def hyp(s):
        h = s.pnp_hypotheses(*large, 3, 60, 10, max_hypotheses=100)
        return [h[k].tobytes() for k in ("sample", "n_sol", "R", "t", "count")]

    calls = {"small": pnp(small, max_hypotheses=65), "large": pnp(large, max_hypotheses=300), "pose_large": pose(large),
             "pose_small": pose(small), "tri": tri, "hyp": hyp}
    fresh = {}
    for name, call in calls.items():
        with Solver(0) as s:
            fresh[name] = call(s)
    with Solver(0) as reused:
        for name in ("small", "large", "small", "pose_large", "hyp", "large", "tri", "pose_small", "small"):
            assert calls[name](reused) == fresh[name], name


# ---------------------------------------------------------------------------
# 8. errors
# ---------------------------------------------------------------------------
def test_errors_leave_the_context_usable(solver):
    sc = [R.scene(9, 0.3, 0.5, 20), R.scene(64, 0.3, 0.5, 75)]
    good = batch_of(sc, [s.cam for s in sc])

    def call(match, batch=good, **kw):
        with pytest.raises(BAError, match=match) as e:
            solver.pnp_ransac(*batch, **kw)
        assert e.value.status == 1      # BA_ERR_INVALID_ARGUMENT

    off = good[0].copy()
    off[2] = off[1] - 1
    call("decreases at problem 1", batch=(off,) + good[1:])
    off = good[0].copy()
    off[0] = 1
    call(r"obs_offset\[0\]", batch=(off,) + good[1:])
    call("max_hypotheses", max_hypotheses=0)
    call("max_hypotheses", max_hypotheses=65537)
    call("min_points", min_points=-1)
    call("min_inliers", min_inliers=-1)
    call("use_prior", use_prior=2)
    call("refine", refine=2)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        call("threshold_px", threshold_px=bad)
    call("cams is null", batch=(good[0], None) + good[2:])
    call("BA_DENSE_SCHUR", options=Options(linear_solver_type="ITERATIVE_SCHUR"))
    call("BA_FP64", options=Options(precision="MIXED_FP32"))
    # refine off: the LM options are not read
    solver.pnp_ransac(*good, refine=0, options=Options(precision="MIXED_FP32"))
    # NULL required arrays, through the C ABI
    lib, h = solver.lib, solver.h
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    out, inl = np.zeros((2, 6)), np.zeros(len(good[3]), np.uint8)

    def raw(**null):
        f = dict(obs_offset=p(good[0]), cams=p(good[1]), K=p(good[2]), pts=p(good[3]), obs_uv=p(good[4]))
        f.update({k: v for k, v in null.items() if k in f})
        pb = N.ba_pose_batch(n_problems=2, reserved=0, huber_a=0.0, **f)
        return lib.ba_pnp_ransac(h, C.byref(pb), None, None, null.get("cams_out", p(out)), null.get("inlier", p(inl)),
                                 None)

    assert raw() == 0
    for name in ("obs_offset", "cams", "K", "pts", "obs_uv", "cams_out", "inlier"):
        assert raw(**{name: None}) == 1, name
        assert b"null" in lib.ba_last_error(h)
    assert lib.ba_pnp_ransac(h, None, None, None, p(out), p(inl), None) == 1
    # the inspection entry: ranges
    for kw, match in ((dict(problem=2), "problem 2 out of range"), (dict(h0=990, n=20), "outside max_hypotheses")):
        a = dict(problem=0, h0=0, n=4)
        a.update(kw)
        with pytest.raises(BAError, match=match):
            solver.pnp_hypotheses(*good, a["problem"], a["h0"], a["n"])
    # the context still works, and an empty batch is BA_OK
    cams, mask, res = solver.pnp_ransac(*good)
    assert [r.status for r in res] == [N.PNP_OK, N.PNP_OK] and np.array_equal(mask, np.concatenate([s.inlier for s in sc]))
    e_c, e_i, e_r = solver.pnp_ransac(np.zeros(1, np.int32), np.zeros((0, 6)), np.zeros((0, 9), np.float32),
                                      np.zeros((0, 3)), np.zeros((0, 2), np.float32))
    assert e_c.shape == (0, 6) and e_i.shape == (0,) and e_r == []
    times = solver.pnp_times()
    assert times.shape == (3,) and np.all(times >= 0) and times[2] >= times[0]
