"""GPU tests for the five-point essential solver of ba_two_view_ransac
(e_solver = TV_E_FIVE_POINT) and ba_two_view_hypotheses_e5 against the numpy
reference (tests/two_view_e5_ref.py): the solver yardstick, the integer vote
of every solution, slices, the winner and its tie rule, the pose end to end,
the noisy scenes the eight-point vote loses, the model choice, the
independence of the homography half from the mode, and the contract.

Measured device values: DESIGN.md section 22.3."""
from functools import lru_cache

import numpy as np
import pytest

import two_view_e5_ref as F
import two_view_ref as R
from bundleadjustment_amd import Options, Solver, make_synthetic
from bundleadjustment_amd import _native as N
from bundleadjustment_amd._native import BAError
from bundleadjustment_amd.problem import angle_axis_to_rotation
from test_two_view import RES_FIELDS, batch_of, mixed_scenes, result_bits
from test_two_view_cpu import MARGIN, REF_DIR_RAD, REF_ROT_RAD, THR2

pytestmark = pytest.mark.gpu

FIVE = dict(e_solver=N.TV_E_FIVE_POINT)


@pytest.fixture(scope="module")
def solver():
    s = Solver(0)
    yield s
    s.close()


@lru_cache(maxsize=None)
def device_solutions(n, planar):
    """All 1000 hypotheses of a solver case, once (the cached arrays are read-only)"""
    with Solver(0) as s:
        hyp = s.two_view_hypotheses_e5(*batch_of([R.solver_scene(n, planar)]), 0, 0, F.SOLVER_H, max_hypotheses=F.SOLVER_H)
    for a in hyp.values():
        a.setflags(write=False)
    return hyp


def bits5(inl, res, i, sl):
    return result_bits(inl, res, i, sl) + (res[i].best_solution_e,)


# ---------------------------------------------------------------------------
# 1. yardstick
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("n", F.SOLVER_NS)
def test_solver_within_the_yardstick(n, planar):
    hyp = device_solutions(n, planar)
    assert np.array_equal(hyp["sample"], F.solver_reference(n, planar)["smp"])
    F.check_yardstick(n, planar, hyp["n_sol"], hyp["E"], MARGIN)


# ---------------------------------------------------------------------------
# 2. counts
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("n", F.SOLVER_NS)
def test_counts_equal_the_predicate_at_the_device_solutions(n, planar):
    sc = R.solver_scene(n, planar)
    hyp = device_solutions(n, planar)
    border = 0
    for s in range(10):
        valid = hyp["n_sol"] > s
        cnt, brd, _, _ = R.vote(hyp["E"][:, s], valid, R.ESSENTIAL, sc, THR2)
        got = hyp["count"][:, s]
        assert np.all(got[~valid] == 0) and np.all(hyp["E"][~valid, s] == 0.0)
        assert np.all((got >= cnt) & (got <= cnt + brd)), s
        assert np.all(got[valid] >= 5)                    # a solution holds its own five samples
        border += int(brd.sum())
    assert border <= 1e-3 * int(hyp["n_sol"].sum()) * n


# ---------------------------------------------------------------------------
# 3. slices
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("cnt", [1, 63, 64, 65])
def test_hypothesis_ranges_are_slices_of_the_whole(solver, cnt):
    full = device_solutions(64, False)
    b = batch_of([R.solver_scene(64, False)])
    for h0 in (0, 63, 700):
        part = solver.two_view_hypotheses_e5(*b, 0, h0, cnt, max_hypotheses=F.SOLVER_H)
        for key in ("sample", "n_sol", "E", "count"):
            assert part[key].tobytes() == full[key][h0:h0 + cnt].tobytes(), (key, h0)


# ---------------------------------------------------------------------------
# 4. winner
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 63, 64, 65])
def test_winner_is_the_first_maximum_of_the_inspection_counts(solver, H):
    sc = R.e2e_scene(64, 0.0, False)
    b = batch_of([sc])
    hyp = solver.two_view_hypotheses_e5(*b, 0, 0, H, max_hypotheses=H)
    inl, res = solver.two_view_ransac(*b, max_hypotheses=H, min_good=8, model=N.TV_ESSENTIAL, **FIVE)
    r = res[0]
    cnt = hyp["count"]
    assert hyp["n_sol"].sum() > 0
    best = int(cnt.max())
    h = int(np.flatnonzero(cnt.max(axis=1) == best)[0])
    s = int(np.flatnonzero(cnt[h] == best)[0])
    assert best >= 8 and r.status == N.TV_OK
    assert (r.votes_e, r.best_hypothesis_e, r.best_solution_e) == (best, h, s)
    Ep = R.project_e(hyp["E"][h, s])[0]
    assert R.sign_free_dist(r.E, Ep) <= MARGIN * 1e-15 and np.sum(r.E * Ep) > 0.0
    assert np.array_equal(inl, R.final_mask_e(r.E, sc.uv1, sc.uv2, THR2)[0]) and r.n_inliers == int(inl.sum())


def test_ties_go_to_the_lower_hypothesis_then_the_lower_solution(solver):
    """With eight matches every sample is a permutation of the same eight, and many (h, s) tie at the top count"""
    sc = R.solver_scene(8, False)
    b = batch_of([sc])
    hyp = solver.two_view_hypotheses_e5(*b, 0, 0, 200, max_hypotheses=200)
    _, res = solver.two_view_ransac(*b, max_hypotheses=200, min_good=1, model=N.TV_ESSENTIAL, **FIVE)
    cnt = hyp["count"]
    best = int(cnt.max())
    assert int(np.sum(cnt == best)) > 1
    h = int(np.flatnonzero(cnt.max(axis=1) == best)[0])
    s = int(np.flatnonzero(cnt[h] == best)[0])
    assert (res[0].votes_e, res[0].best_hypothesis_e, res[0].best_solution_e) == (best, h, s)


# ---------------------------------------------------------------------------
# 5. end to end, noise-free inliers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,frac", R.E2E_CASES)
def test_end_to_end_on_noise_free_inliers(solver, n, frac):
    sc = R.e2e_scene(n, frac, False)
    inl, res = solver.two_view_ransac(*batch_of([sc]), max_hypotheses=R.E2E_H, min_good=8, **FIVE)
    r = res[0]
    errs = R.truth_errors(sc, angle_axis_to_rotation(r.cam[:3]), r.cam[3:], None)
    print(f"five-point n={n} outliers={frac}: votes {r.votes_e}, errors (rad) {errs}, good {r.n_good}/{r.n_good_second}")
    assert r.status == N.TV_OK and r.model == N.TV_ESSENTIAL
    assert r.votes_e == int(sc.inlier.sum()) and np.array_equal(inl, sc.inlier) and r.n_inliers == r.votes_e
    assert errs[0] <= REF_ROT_RAD and errs[1] <= REF_DIR_RAD
    assert abs(np.linalg.norm(r.cam[3:]) - 1.0) <= 1e-14 and not r.normal.any()


# ---------------------------------------------------------------------------
# 6. the scenes the eight-point vote loses
# ---------------------------------------------------------------------------
def test_projection_keeps_the_votes_on_the_noisy_scene(solver):
    sc = R.e2e_scene(200, 0.3, False, 0.3)
    b = batch_of([sc])
    _, res = solver.two_view_ransac(*b, min_good=8, **FIVE)
    _, res8 = solver.two_view_ransac(*b, min_good=8, model=N.TV_ESSENTIAL)
    r = res[0]
    print(f"noisy 200: five-point votes {r.votes_e} -> inliers {r.n_inliers}; eight-point {res8[0].votes_e} -> {res8[0].n_inliers}")
    assert r.status == N.TV_OK and r.n_inliers >= 0.9 * r.votes_e


def test_thousand_match_noisy_pairs_end_ok(solver):
    scenes = [R.scene(1000, 0.3, 0.3, 9100 + s, False) for s in range(8)]
    _, res = solver.two_view_ransac(*batch_of(scenes), **FIVE)                     # the default min_good = 101
    for s, r in enumerate(res):
        errs = R.truth_errors(scenes[s], angle_axis_to_rotation(r.cam[:3]), r.cam[3:], None)
        print(f"scene {s}: status {r.status} model {r.model} votes {r.votes_e} inliers {r.n_inliers} good {r.n_good} errors {errs}")
    for r in res:
        assert r.status == N.TV_OK
        assert r.n_inliers >= 0.9 * r.votes_e
        assert r.n_good >= 0.9 * r.n_inliers


# ---------------------------------------------------------------------------
# 7. model choice
# ---------------------------------------------------------------------------
def test_model_choice_with_the_five_point_score(solver):
    for planar in (False, True):
        _, res = solver.two_view_ransac(*batch_of([R.e2e_scene(200, 0.3, planar, 0.3)]), min_good=8, **FIVE)
        r = res[0]
        print(f"planar={planar}: ratio {r.score_h / (r.score_h + r.score_e):.3f}")
        assert r.status == N.TV_OK and r.model == (N.TV_HOMOGRAPHY if planar else N.TV_ESSENTIAL)
    for n, frac in R.E2E_CASES:
        _, res = solver.two_view_ransac(*batch_of([R.e2e_scene(n, frac, True)]), max_hypotheses=R.E2E_H, min_good=8, **FIVE)
        assert res[0].status == N.TV_OK and res[0].model == N.TV_HOMOGRAPHY, (n, frac)


# ---------------------------------------------------------------------------
# 8. the homography half does not see the mode
# ---------------------------------------------------------------------------
def test_homography_outputs_are_bitwise_those_of_the_default_mode(solver):
    scenes = mixed_scenes() + [R.scene(0, 0.0, 0.0, 44, False), R.e2e_scene(65, 0.3, True)]
    b = batch_of(scenes)
    _, r8 = solver.two_view_ransac(*b, min_good=8)
    _, r5 = solver.two_view_ransac(*b, min_good=8, **FIVE)
    assert len(scenes[5].uv1) == 0 and r5[5].status == N.TV_FEW_POINTS
    for a, c in zip(r8, r5):
        if a.status in (N.TV_OK, N.TV_NO_POSE) and c.status in (N.TV_OK, N.TV_NO_POSE):
            assert (a.votes_h, a.score_h) == (c.votes_h, c.score_h) and a.H.tobytes() == c.H.tobytes()
        if a.status == N.TV_OK and c.status == N.TV_OK:
            assert a.best_hypothesis_h == c.best_hypothesis_h
        assert a.best_solution_e == 0
    assert [r.status for r in r5][1] == N.TV_OK and r5[3].model == N.TV_HOMOGRAPHY


# ---------------------------------------------------------------------------
# 9. contract
# ---------------------------------------------------------------------------
def test_mixed_batch_statuses_independence_and_repeatability(solver):
    order = mixed_scenes()
    b = batch_of(order)
    off = b[0]
    sl = [slice(off[i], off[i + 1]) for i in range(len(order))]
    kw = dict(min_inliers=12, **FIVE)
    inl, res = solver.two_view_ransac(*b, **kw)
    inl2, res2 = solver.two_view_ransac(*b, **kw)
    bits = [bits5(inl, res, i, sl[i]) for i in range(len(order))]
    assert bits == [bits5(inl2, res2, i, sl[i]) for i in range(len(order))]
    assert [r.status for r in res] == [N.TV_FEW_POINTS, N.TV_OK, N.TV_NO_MODEL, N.TV_OK, N.TV_NO_POSE]
    assert [r.model for r in res] == [0, N.TV_ESSENTIAL, 0, N.TV_HOMOGRAPHY, N.TV_ESSENTIAL]
    assert 12 <= res[4].n_good <= 64 and res[4].votes_e >= 12      # 64 matches cannot reach min_good = 101; NO_POSE keeps its diagnostics
    for i in (0, 2, 4):
        r = res[i]
        assert not inl[sl[i]].any() and not r.cam.any() and not r.normal.any() and r.n_inliers == 0
        assert (r.best_hypothesis_e, r.best_hypothesis_h, r.best_solution_e) == (-1, -1, 0)
    for i in (0, 2):
        r = res[i]
        assert not r.E.any() and not r.H.any() and (r.votes_e, r.votes_h, r.n_good, r.score_e, r.score_h) == (0, 0, 0, 0, 0)
    for i in range(len(order)):                                    # alone: 8 lanes per slot instead of 1
        i1, r1 = solver.two_view_ransac(*batch_of([order[i]]), **kw)
        assert bits5(i1, r1, 0, slice(None)) == bits[i], i
    perm = [3, 0, 4, 2, 1]
    bp = batch_of([order[j] for j in perm])
    ip, rp = solver.two_view_ransac(*bp, **kw)
    for k, j in enumerate(perm):
        assert bits5(ip, rp, k, slice(bp[0][k], bp[0][k + 1])) == bits[j], j


def test_unknown_solver_is_an_error_and_the_context_stays_usable(solver):
    sc = [R.e2e_scene(64, 0.0, False), R.e2e_scene(65, 0.3, True)]
    good = batch_of(sc)
    for call in (lambda: solver.two_view_ransac(*good, e_solver=2),
                 lambda: solver.two_view_ransac(*good, e_solver=-1),
                 lambda: solver.two_view_hypotheses(*good, 0, 0, 4, e_solver=2),
                 lambda: solver.two_view_hypotheses_e5(*good, 0, 0, 4, e_solver=2)):
        with pytest.raises(BAError, match="unknown e_solver") as e:
            call()
        assert e.value.status == 1      # BA_ERR_INVALID_ARGUMENT
    for kw, match in ((dict(pair=2), "pair 2 out of range"), (dict(h0=990, n=20), "outside max_hypotheses")):
        a = dict(pair=0, h0=0, n=4)
        a.update(kw)
        with pytest.raises(BAError, match=match):
            solver.two_view_hypotheses_e5(*good, a["pair"], a["h0"], a["n"])
    with pytest.raises(BAError, match="fewer than 8 matches"):
        solver.two_view_hypotheses_e5(*batch_of([R.scene(7, 0.0, 0.0, 41, False)]), 0, 0, 4)
    mask, res = solver.two_view_ransac(*good, min_good=8, **FIVE)
    assert [r.status for r in res] == [N.TV_OK, N.TV_OK] and np.array_equal(mask, np.concatenate([s.inlier for s in sc]))
    # the old inspection entry reports the eight-point E whatever the selector
    h8 = solver.two_view_hypotheses(*good, 0, 0, 70)
    h5 = solver.two_view_hypotheses(*good, 0, 0, 70, **FIVE)
    assert all(h8[k].tobytes() == h5[k].tobytes() for k in h8)


def test_solve_is_untouched_by_a_five_point_call_in_between(solver):
    p = make_synthetic(6, 300, 4, seed=31)
    b = batch_of([R.e2e_scene(65, 0.3, False)])
    fields = ["iteration", "step_is_valid", "step_is_successful", "cost", "cost_change", "gradient_max_norm",
              "gradient_norm", "step_norm", "relative_decrease", "trust_region_radius", "model_cost_change"]

    def solve(between):
        solver.set_problem(p)
        if between:
            solver.two_view_ransac(*b, **FIVE)
        solver.solve(Options(max_num_iterations=6))
        cams, pts = solver.params()
        return [[r[f] for f in fields] for r in solver.iteration_log()], cams, pts

    log0, c0, x0 = solve(False)
    log1, c1, x1 = solve(True)
    assert log0 == log1 and c0.tobytes() == c1.tobytes() and x0.tobytes() == x1.tobytes()
    solver.two_view_ransac(*b, **FIVE)
    solver.two_view_hypotheses_e5(*b, 0, 0, 64)
    c2, x2 = solver.params()
    assert c2.tobytes() == c0.tobytes() and x2.tobytes() == x0.tobytes()
    assert RES_FIELDS[0] == "status"
