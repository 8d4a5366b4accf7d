"""GPU tests for ba_two_view_ransac / ba_two_view_hypotheses against the numpy
reference (tests/two_view_ref.py): the pinned sampler, both minimal solvers on
noise-free scenes, the integer vote, the per-pair stage end to end, the model
choice on noisy scenes, mixed batches, the context / staging contract, the
error contract and the composition with ba_triangulate and ba_solve.

Measured device values: DESIGN.md section 21.3."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import two_view_ref as R
from bundleadjustment_amd import Options, Problem, Solver, make_synthetic
from bundleadjustment_amd import _native as N
from bundleadjustment_amd._native import BAError
from bundleadjustment_amd.problem import angle_axis_to_rotation, fix_camera

pytestmark = pytest.mark.gpu

MARGIN = 16.0      # a different null-vector method / SVD at the same conditioning (see test_two_view_cpu.py)
THR2 = 1.0
RES_FIELDS = ["status", "model", "n_inliers", "n_good", "n_good_second", "best_hypothesis_e", "best_hypothesis_h",
              "votes_e", "votes_h", "score_e", "score_h"]


@pytest.fixture(scope="module")
def solver():
    s = Solver(0)
    yield s
    s.close()


def batch_of(scenes):
    """(match_offset, K1, K2, uv1, uv2) of a list of scenes"""
    off = np.concatenate([[0], np.cumsum([len(s.uv1) for s in scenes])]).astype(np.int32)
    K = np.stack([s.K for s in scenes]).astype(np.float32).reshape(len(scenes), 9)
    uv1 = np.concatenate([s.uv1 for s in scenes]).reshape(-1, 2).astype(np.float32)
    uv2 = np.concatenate([s.uv2 for s in scenes]).reshape(-1, 2).astype(np.float32)
    return off, K, None, uv1, uv2


def result_bits(inl, res, i, sl):
    r = res[i]
    return (inl[sl].tobytes(),) + tuple(getattr(r, f) for f in RES_FIELDS) + \
        (r.E.tobytes(), r.H.tobytes(), r.cam.tobytes(), r.normal.tobytes())


@lru_cache(maxsize=None)
def device_models(n, planar):
    """All 1000 hypotheses of a solver case, once (the cached arrays are read-only)"""
    with Solver(0) as s:
        hyp = s.two_view_hypotheses(*batch_of([R.solver_scene(n, planar)]), 0, 0, R.SOLVER_H, max_hypotheses=R.SOLVER_H)
    for a in hyp.values():
        a.setflags(write=False)
    return hyp


# ---------------------------------------------------------------------------
# 1. sampler
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 9, 64, 65])
def test_sampler_equals_the_reference(solver, n):
    b = batch_of([R.scene(n, 0.0, 0.0, 5, False)])
    for seed in (0, 99):
        for h0 in (0, 63, 64):
            hyp = solver.two_view_hypotheses(*b, 0, h0, 70, max_hypotheses=200, seed=seed)
            assert np.array_equal(hyp["sample"], R.samples(seed, n, h0 + 70, h0=h0)), (seed, h0)


# ---------------------------------------------------------------------------
# 2. solvers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("n", R.SOLVER_NS)
def test_solvers_within_the_reference_yardstick(n, planar):
    """E on the general scene, H on the planar one: every model fits its own
    samples within 16 x the reference's worst residual, and lies within 16 x
    the reference's own distance to the truth (+ 1e-12) of the reference's
    model of the same sample."""
    ref_worst = max(float(R.solver_reference(m, planar)[2].max()) for m in R.SOLVER_NS)
    sc = R.solver_scene(n, planar)
    smp, mdl, _, dist = R.solver_reference(n, planar)
    hyp = device_models(n, planar)
    assert np.array_equal(hyp["sample"], smp)
    k = 1 if planar else 0
    Ms = hyp["H" if planar else "E"]
    assert np.all(hyp["valid"][:, k] == 1)
    assert np.max(np.abs(np.linalg.norm(Ms, axis=(1, 2)) - 1.0)) <= 1e-14
    worst_res, worst_ratio = 0.0, 0.0
    for h in range(R.SOLVER_H):
        res = R.h_sample_residual(Ms[h], sc, smp[h]) if planar else R.e_sample_residual(Ms[h], sc, smp[h])
        d = R.sign_free_dist(Ms[h], mdl[h])
        if planar:
            assert np.linalg.norm(Ms[h] - mdl[h]) == d      # the pinned sign
        worst_res = max(worst_res, res)
        worst_ratio = max(worst_ratio, d / (MARGIN * dist[h] + 1e-12))
    print(f"n = {n} {'H' if planar else 'E'}: device worst sample residual {worst_res:.3g} (reference {ref_worst:.3g}), "
          f"worst distance / bound {worst_ratio:.3g}")
    assert worst_res <= MARGIN * ref_worst
    assert worst_ratio <= 1.0


# ---------------------------------------------------------------------------
# 3. counts
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("n", R.SOLVER_NS)
def test_counts_equal_the_predicate_at_the_device_models(n, planar):
    sc = R.solver_scene(n, planar)
    hyp = device_models(n, planar)
    border = 0
    for k, which in ((0, R.ESSENTIAL), (1, R.HOMOGRAPHY)):
        valid = hyp["valid"][:, k] == 1
        cnt, brd, _, _ = R.vote(hyp["H" if k else "E"], valid, which, sc, THR2)
        got = hyp["count"][:, k]
        assert np.all(got[~valid] == 0)
        assert np.all(hyp["H" if k else "E"][~valid] == 0.0)
        assert np.all((got >= cnt) & (got <= cnt + brd)), which
        border += int(brd.sum())
    assert border <= 1e-3 * 2 * R.SOLVER_H * n


@pytest.mark.parametrize("cnt", [1, 63, 64, 65])
def test_hypothesis_ranges_are_slices_of_the_whole(solver, cnt):
    full = device_models(64, False)
    b = batch_of([R.solver_scene(64, False)])
    for h0 in (0, 63, 700):
        part = solver.two_view_hypotheses(*b, 0, h0, cnt, max_hypotheses=R.SOLVER_H)
        for key in ("sample", "E", "H", "valid", "count"):
            assert part[key].tobytes() == full[key][h0:h0 + cnt].tobytes(), (key, h0)


# ---------------------------------------------------------------------------
# 4. end to end, noise-free inliers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 63, 64, 65])
def test_winner_for_small_hypothesis_counts(solver, H):
    """The wave argmax and the select stage at hypothesis counts around a wave"""
    sc = R.e2e_scene(64, 0.0, False)
    b = batch_of([sc])
    hyp = solver.two_view_hypotheses(*b, 0, 0, H, max_hypotheses=H)
    inl, res = solver.two_view_ransac(*b, max_hypotheses=H, min_good=8, model=N.TV_ESSENTIAL)
    r = res[0]
    _, brd, full, win = R.vote(hyp["E"], hyp["valid"][:, 0] == 1, R.ESSENTIAL, sc, THR2)
    assert brd.sum() == 0
    assert r.status == N.TV_OK and r.best_hypothesis_e == win and r.votes_e == full[win] >= 8
    assert np.array_equal(inl, R.final_mask_e(r.E, sc.uv1, sc.uv2, THR2)[0]) and r.n_inliers == r.n_good == int(inl.sum())
    if H >= 63:
        assert inl.all()


@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("n,frac", R.E2E_CASES)
def test_end_to_end_on_noise_free_inliers(solver, n, frac, planar):
    sc = R.e2e_scene(n, frac, planar)
    b = batch_of([sc])
    hyp = solver.two_view_hypotheses(*b, 0, 0, R.E2E_H, max_hypotheses=R.E2E_H)
    inl, res = solver.two_view_ransac(*b, max_hypotheses=R.E2E_H, min_good=8)
    r = res[0]
    assert r.status == N.TV_OK and r.model == (N.TV_HOMOGRAPHY if planar else N.TV_ESSENTIAL)
    # the vote: numpy's predicate over the device's models
    for k, which, bh, votes in ((0, R.ESSENTIAL, r.best_hypothesis_e, r.votes_e),
                                (1, R.HOMOGRAPHY, r.best_hypothesis_h, r.votes_h)):
        _, brd, full, win = R.vote(hyp["H" if k else "E"], hyp["valid"][:, k] == 1, which, sc, THR2)
        assert brd.sum() == 0                                   # a condition on the scene, not on the device
        assert (bh, votes) == (win if full[win] >= 8 else -1, full[win]), which
    assert np.array_equal(r.H, hyp["H"][r.best_hypothesis_h] if r.best_hypothesis_h >= 0 else np.zeros((3, 3)))
    assert r.best_hypothesis_e >= 0
    Ep = R.project_e(hyp["E"][r.best_hypothesis_e])[0]
    assert R.sign_free_dist(r.E, Ep) <= MARGIN * 1e-15 and np.sum(r.E * Ep) > 0.0
    # the mask: the final predicate at the returned model
    if planar:
        want, score = R.final_mask_h(r.H, sc.uv1, sc.uv2, THR2)
    else:
        want, score = R.final_mask_e(r.E, sc.uv1, sc.uv2, THR2)
    assert np.array_equal(inl, want) and np.all(inl[sc.inlier]) and r.n_inliers == int(inl.sum())
    got = r.score_h if planar else r.score_e
    assert abs(got - score) <= 1e-9 * max(score, 1.0)
    assert (np.float32(r.score_h / (r.score_h + r.score_e)) > 0.4) == planar
    assert r.n_good == r.n_inliers and r.n_good_second <= r.n_good
    # the pose: within 16 x the reference's error for the same winning sample
    smp = hyp["sample"][r.best_hypothesis_h if planar else r.best_hypothesis_e]
    Mref = R.models_of(sc, smp)[1 if planar else 0]
    ref = R.pose_from(R.HOMOGRAPHY if planar else R.ESSENTIAL, Mref, sc.uv1, sc.uv2, THR2)
    Rm = angle_axis_to_rotation(r.cam[:3])
    assert abs(np.linalg.norm(r.cam[3:]) - 1.0) <= 1e-14
    errs = R.truth_errors(sc, Rm, r.cam[3:], r.normal if planar else None)
    ref_errs = R.truth_errors(sc, ref[0], ref[1], ref[2] if planar else None)
    print(f"n={n} outliers={frac} planar={planar}: errors (rad) {errs}, reference {ref_errs}, "
          f"good {r.n_good}/{r.n_good_second}")
    for e, re_ in zip(errs, ref_errs):
        assert e <= max(MARGIN * re_, 1e-9)
    if not planar:
        assert not r.normal.any()


# ---------------------------------------------------------------------------
# 5. noisy scenes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("planar", [False, True])
def test_noisy_scene_model_choice_and_forced_models(solver, planar):
    sc = R.e2e_scene(200, 0.3, planar, 0.3)
    b = batch_of([sc])
    inl, res = solver.two_view_ransac(*b, min_good=8)
    r = res[0]
    auto = N.TV_HOMOGRAPHY if planar else N.TV_ESSENTIAL
    ratio = r.score_h / (r.score_h + r.score_e)
    print(f"planar={planar}: ratio {ratio:.3f}, inliers {r.n_inliers} of {int(sc.inlier.sum())}, good {r.n_good}/"
          f"{r.n_good_second}, errors {R.truth_errors(sc, angle_axis_to_rotation(r.cam[:3]), r.cam[3:], None)}")
    assert r.status == N.TV_OK and r.model == auto
    assert r.n_inliers >= 0.5 * int(sc.inlier.sum())
    if planar:                # (a match displaced along its epipolar line is an honest E-inlier; a transfer error is not fooled)
        assert not inl[~sc.inlier].any()
    for forced in (N.TV_ESSENTIAL, N.TV_HOMOGRAPHY):
        fi, fr = solver.two_view_ransac(*b, min_good=8, model=forced)
        if forced == auto:
            assert result_bits(fi, fr, 0, slice(None)) == result_bits(inl, res, 0, slice(None))
        assert fr[0].model == (forced if fr[0].status in (N.TV_OK, N.TV_NO_POSE) else 0)
        assert (fr[0].votes_e, fr[0].votes_h) == (r.votes_e, r.votes_h) or fr[0].status == N.TV_NO_MODEL


# ---------------------------------------------------------------------------
# 6. mixed batch
# ---------------------------------------------------------------------------
def mixed_scenes():
    few = R.scene(7, 0.0, 0.0, 41, False)
    junk = R.scene(12, 1.0, 0.0, 42, False)                    # 12 displaced matches hold no model of 8
    small = R.scene(64, 0.0, 0.3, 43, False)                   # 64 matches cannot reach min_good = 101
    return [few, R.e2e_scene(200, 0.3, False, 0.3), junk, R.e2e_scene(200, 0.3, True, 0.3), small]


def test_mixed_batch_statuses_and_independence(solver):
    order = mixed_scenes()
    b = batch_of(order)
    off = b[0]
    sl = [slice(off[i], off[i + 1]) for i in range(len(order))]
    # every eight-point model holds its own eight samples, so NO_MODEL needs a floor above 8: with 12, all of junk's
    kw = dict(min_inliers=12)
    inl, res = solver.two_view_ransac(*b, **kw)
    inl2, res2 = solver.two_view_ransac(*b, **kw)
    bits = [result_bits(inl, res, i, sl[i]) for i in range(len(order))]
    assert bits == [result_bits(inl2, res2, i, sl[i]) for i in range(len(order))]
    assert [r.status for r in res] == [N.TV_FEW_POINTS, N.TV_OK, N.TV_NO_MODEL, N.TV_OK, N.TV_NO_POSE]
    assert [r.model for r in res] == [0, N.TV_ESSENTIAL, 0, N.TV_HOMOGRAPHY, N.TV_ESSENTIAL]
    for i in (0, 2, 4):
        r = res[i]
        assert not inl[sl[i]].any() and not r.cam.any() and not r.normal.any() and r.n_inliers == 0
        assert (r.best_hypothesis_e, r.best_hypothesis_h) == (-1, -1)
    for i in (0, 2):
        r = res[i]
        assert not r.E.any() and not r.H.any() and (r.votes_e, r.votes_h, r.n_good, r.score_e, r.score_h) == (0, 0, 0, 0, 0)
    assert 12 <= res[4].n_good <= 64 and res[4].votes_e >= 12
    # each pair alone (8 lanes per hypothesis instead of 1), and the batch in another order
    for i in range(len(order)):
        i1, r1 = solver.two_view_ransac(*batch_of([order[i]]), **kw)
        assert result_bits(i1, r1, 0, slice(None)) == bits[i], i
    perm = [3, 0, 4, 2, 1]
    bp = batch_of([order[j] for j in perm])
    ip, rp = solver.two_view_ransac(*bp, **kw)
    for k, j in enumerate(perm):
        assert result_bits(ip, rp, k, slice(bp[0][k], bp[0][k + 1])) == bits[j], j
    # K2 given explicitly equals K2 = NULL
    ik, rk = solver.two_view_ransac(b[0], b[1], b[1].copy(), b[3], b[4], **kw)
    assert [result_bits(ik, rk, i, sl[i]) for i in range(len(order))] == bits


# ---------------------------------------------------------------------------
# 7., 8. context and staging
# ---------------------------------------------------------------------------
def test_solve_is_untouched_by_a_two_view_call_in_between(solver):
    p = make_synthetic(6, 300, 4, seed=31)
    b = batch_of([R.e2e_scene(65, 0.3, False)])
    fields = ["iteration", "step_is_valid", "step_is_successful", "cost", "cost_change", "gradient_max_norm",
              "gradient_norm", "step_norm", "relative_decrease", "trust_region_radius", "model_cost_change"]

    def solve(between):
        solver.set_problem(p)
        if between:
            solver.two_view_ransac(*b)
        solver.solve(Options(max_num_iterations=6))
        cams, pts = solver.params()
        return [[r[f] for f in fields] for r in solver.iteration_log()], cams, pts

    log0, c0, x0 = solve(False)
    log1, c1, x1 = solve(True)
    assert log0 == log1 and c0.tobytes() == c1.tobytes() and x0.tobytes() == x1.tobytes()
    solver.two_view_ransac(*b)
    solver.two_view_hypotheses(*b, 0, 0, 64)
    c2, x2 = solver.params()
    assert c2.tobytes() == c0.tobytes() and x2.tobytes() == x0.tobytes()


def test_staging_arenas_interleave_bitwise():
    """One context through two-view small -> large -> small interleaved with a
    PnP call, a triangulation and the inspection entry: every result equals,
    bit for bit, the same call on a fresh context."""
    import pnp_ref as P
    import triangulate_ref as T

    small = batch_of([R.e2e_scene(65, 0.3, False)])
    large = batch_of([R.scene(40 + 13 * i, 0.3, 0.0, 600 + i, bool(i & 1)) for i in range(12)])
    ps = P.scene(64, 0.3, 0.5, 75)
    pb = (np.array([0, 64], np.int32), ps.cam[None], ps.K[None], ps.pts, ps.uv)
    tb = T.scene(2, 2, 11)

    def tv(b, **kw):
        def call(s):
            inl, res = s.two_view_ransac(*b, min_good=8, **kw)
            off = b[0]
            return [result_bits(inl, res, i, slice(off[i], off[i + 1])) for i in range(len(off) - 1)]
        return call

    def pnp(s):
        cams, inl, res = s.pnp_ransac(*pb, options=Options(max_num_iterations=10))
        return [cams.tobytes(), inl.tobytes(), res[0].status, res[0].best_hypothesis]

    def tri(s):
        pts, status, _ = s.triangulate(tb.extr, tb.K, tb.obs_offset, tb.obs_cam, tb.obs_uv, cam_center=tb.cam_center)
        return [pts.tobytes(), status.tobytes()]

    def hyp(s):
        h = s.two_view_hypotheses(*large, 3, 60, 10, max_hypotheses=100)
        return [h[k].tobytes() for k in ("sample", "E", "H", "valid", "count")]

    calls = {"small": tv(small, max_hypotheses=65), "large": tv(large, max_hypotheses=300), "pnp": pnp, "tri": tri,
             "hyp": hyp}
    fresh = {}
    for name, call in calls.items():
        with Solver(0) as s:
            fresh[name] = call(s)
    with Solver(0) as reused:
        for name in ("small", "large", "small", "pnp", "hyp", "large", "tri", "pnp", "small"):
            assert calls[name](reused) == fresh[name], name


# ---------------------------------------------------------------------------
# 9. errors
# ---------------------------------------------------------------------------
def test_errors_leave_the_context_usable(solver):
    sc = [R.e2e_scene(64, 0.0, False), R.e2e_scene(65, 0.3, True)]
    good = batch_of(sc)

    def call(match, batch=good, **kw):
        with pytest.raises(BAError, match=match) as e:
            solver.two_view_ransac(*batch, **kw)
        assert e.value.status == 1      # BA_ERR_INVALID_ARGUMENT

    off = good[0].copy()
    off[2] = off[1] - 1
    call("decreases at pair 1", batch=(off,) + good[1:])
    off = good[0].copy()
    off[0] = 1
    call(r"match_offset\[0\]", batch=(off,) + good[1:])
    call("max_hypotheses", max_hypotheses=0)
    call("max_hypotheses", max_hypotheses=65537)
    call("min_points", min_points=-1)
    call("min_inliers", min_inliers=-1)
    call("min_good", min_good=-1)
    call("unknown model", model=3)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        call("threshold_px", threshold_px=bad)
    for bad in (-0.1, 1.5, float("nan")):
        call("h_ratio", h_ratio=bad)
    # NULL required arrays, through the C ABI
    lib, h = solver.lib, solver.h
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    inl = np.zeros(len(good[3]), np.uint8)
    out = (N.ba_two_view_result * 2)()

    def raw(**null):
        f = dict(match_offset=p(good[0]), K1=p(good[1]), K2=None, uv1=p(good[3]), uv2=p(good[4]))
        f.update({k: v for k, v in null.items() if k in f})
        pb = N.ba_two_view_batch(n_pairs=2, reserved=0, **f)
        return lib.ba_two_view_ransac(h, C.byref(pb), None, null.get("inlier", p(inl)),
                                      null["results"] if "results" in null else out)

    assert raw() == 0
    for name in ("match_offset", "K1", "uv1", "uv2", "inlier", "results"):
        assert raw(**{name: None}) == 1, name
        assert b"null" in lib.ba_last_error(h)
    assert lib.ba_two_view_ransac(h, None, None, p(inl), out) == 1
    # the inspection entry: ranges, and a pair too small to sample
    for kw, match in ((dict(pair=2), "pair 2 out of range"), (dict(h0=990, n=20), "outside max_hypotheses")):
        a = dict(pair=0, h0=0, n=4)
        a.update(kw)
        with pytest.raises(BAError, match=match):
            solver.two_view_hypotheses(*good, a["pair"], a["h0"], a["n"])
    with pytest.raises(BAError, match="fewer than 8 matches"):
        solver.two_view_hypotheses(*batch_of([R.scene(7, 0.0, 0.0, 41, False)]), 0, 0, 4)
    # the context still works, and an empty batch is BA_OK
    mask, res = solver.two_view_ransac(*good, min_good=8)
    assert [r.status for r in res] == [N.TV_OK, N.TV_OK] and np.array_equal(mask, np.concatenate([s.inlier for s in sc]))
    e_i, e_r = solver.two_view_ransac(np.zeros(1, np.int32), np.zeros((0, 9), np.float32), None,
                                      np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32))
    assert e_i.shape == (0,) and e_r == []
    times = solver.two_view_times()
    assert times.shape == (3,) and np.all(times >= 0) and times[2] >= times[0]


# ---------------------------------------------------------------------------
# 10. composition: matches -> pose -> points -> BA
# ---------------------------------------------------------------------------
def test_composition_with_triangulate_and_solve(solver):
    sc = R.e2e_scene(200, 0.3, False, 0.3)
    inl, res = solver.two_view_ransac(*batch_of([sc]))
    r = res[0]
    assert r.status == N.TV_OK and r.model == N.TV_ESSENTIAL
    k = int(inl.sum())
    Rm, t = angle_axis_to_rotation(r.cam[:3]), r.cam[3:]
    ext = np.stack([np.eye(4), np.block([[Rm, t[:, None]], [np.zeros((1, 3)), np.ones((1, 1))]])])
    extr = ext.transpose(0, 2, 1).reshape(2, 16).astype(np.float32)            # column-major world -> camera
    ctr = np.stack([np.zeros(3), -Rm.T @ t]).astype(np.float32)
    K = np.stack([sc.K, sc.K])
    uv = np.stack([sc.uv1[inl], sc.uv2[inl]], 1).reshape(-1, 2)
    pts, status, _ = solver.triangulate(extr, K, 2 * np.arange(k + 1, dtype=np.int32), np.tile([0, 1], k).astype(np.int32),
                                        uv, cam_center=ctr)
    ok = status == N.TRI_OK
    print(f"composition: {k} inliers, {int(ok.sum())} triangulated ({np.bincount(status, minlength=6)})")
    assert ok.sum() >= 0.9 * k
    m = int(ok.sum())
    p = Problem(cams=np.stack([np.zeros(6), r.cam]), K=K, pts=pts[ok],
                obs_cam=np.tile([0, 1], m).astype(np.int32), obs_pt=np.repeat(np.arange(m), 2).astype(np.int32),
                obs_uv=uv.reshape(k, 2, 2)[ok].reshape(-1, 2))
    solver.set_problem(fix_camera(p, 0))
    summ = solver.solve(Options(max_num_iterations=20))
    print(f"composition: BA cost {summ.initial_cost:.6g} -> {summ.final_cost:.6g} ({summ.termination_type})")
    assert summ.termination_type != "FAILURE" and summ.final_cost <= summ.initial_cost
