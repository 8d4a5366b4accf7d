"""ba_triangulate on the device: the DLT against the SVD, the per-point LM
against the oracle on the equivalent one-point problem (test_pose_batch's
tolerances), the statuses against the float32 restatement evaluated at the
device's own point, a cross-check against ba_solve_window_batch, bitwise
reproducibility, the error contract, and the staging arenas of the batch entry
points across growing, shrinking and interleaved calls.  Reference:
tests/triangulate_ref.py."""
import ctypes as C

import numpy as np
import pytest

import triangulate_ref as R
from bundleadjustment_amd import Options, Solver, make_synthetic
from bundleadjustment_amd import _native as N
from bundleadjustment_amd._native import BAError
from conftest import assert_close

pytestmark = pytest.mark.gpu

ALL_SCENES = R.SCENES + ["ragged"]


def get_scene(sc):
    return R.ragged_scene() if sc == "ragged" else R.scene(*sc)


@pytest.fixture(scope="module")
def solver():
    s = Solver(0)
    yield s
    s.close()


def run(solver, b, **kw):
    kw.setdefault("cam_center", b.cam_center)
    return solver.triangulate(b.extr, b.K, b.obs_offset, b.obs_cam, b.obs_uv, huber_a=kw.pop("huber_a", b.huber_a), **kw)


_svd = {}


def svd_points(sc):
    """The SVD point and beta of every point with >= 2 views (computed once)."""
    if sc not in _svd:
        b = get_scene(sc)
        P = R.proj_matrices(b.extr, b.K)
        X, beta = np.zeros((len(b.pts), 3)), np.full(len(b.pts), np.nan)
        for q in range(len(b.pts)):
            cams, uv = R.views(b, q)
            if len(cams) >= 2:
                A = R.dlt_rows(P, cams, uv)
                X[q], beta[q] = R.dlt_svd(A), R.dlt_beta(A)
        _svd[sc] = (X, beta)
    return _svd[sc]


_oracle = {}


def oracle_solves(oracle_lib, sc, start, **opt):
    """oracle_lib.solve on the one-point problem of every point with >= 2
    views, started at `start` ("given": the scene's points, "svd")."""
    key = (sc, start, tuple(sorted(opt.items())))
    if key not in _oracle:
        b = get_scene(sc)
        X0 = b.pts if start == "given" else svd_points(sc)[0]
        huber = opt.pop("huber_a", None)
        o = oracle_lib.default_options(**opt)
        out = {}
        for q in range(len(b.pts)):
            if b.obs_offset[q + 1] - b.obs_offset[q] >= 2:
                _, op, osum, _ = oracle_lib.solve(R.one_point_problem(b, q, X0[q], huber_a=huber), o)
                out[q] = (op[0], osum)
        _oracle[key] = out
    return _oracle[key]


# ---------------------------------------------------------------------------
# 1. DLT against the SVD
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sc", ALL_SCENES)
def test_dlt_matches_svd_within_the_perturbation_bound(solver, sc):
    b = get_scene(sc)
    pts, status, summ = run(solver, b)
    assert summ is None
    Xs, beta = svd_points(sc)
    worst = 0.0
    for q in range(len(b.pts)):
        if b.obs_offset[q + 1] - b.obs_offset[q] < 2:
            assert status[q] == R.FEW_VIEWS and np.all(pts[q] == 0.0)
            continue
        assert beta[q] <= 1e-9, (q, beta[q])            # (never skip a point: choose another seed)
        err = R.dlt_error(pts[q], Xs[q])
        worst = max(worst, err / beta[q])
        assert err <= 256 * beta[q], (q, err, beta[q])
    print(f"scene {sc}: worst DLT error {worst:.3g} beta")


# ---------------------------------------------------------------------------
# 2. refinement against the oracle, same start bits
# ---------------------------------------------------------------------------
def check_point(q, X, s, ref, counts=True):
    ox, osum = ref
    if counts:
        assert s.termination_type == osum["termination_type"], (q, s, osum)
        assert s.num_iterations == osum["num_iterations"], (q, s, osum)
        assert s.num_successful_steps == osum["num_successful_steps"], (q, s, osum)
        assert s.initial_cost == pytest.approx(osum["initial_cost"], rel=1e-12), q
    assert s.final_cost == pytest.approx(osum["final_cost"], rel=1e-10), q
    assert_close(X, ox, 1e-8, 1e-10, f"point {q}")


@pytest.mark.parametrize("sc", ALL_SCENES)
def test_refinement_matches_oracle(solver, oracle_lib, sc):
    b = get_scene(sc)
    pts, status, summ = run(solver, b, pts_init=b.pts, refine=True, options=Options(max_num_iterations=20))
    ref = oracle_solves(oracle_lib, sc, "given", max_num_iterations=20)
    its, terms = set(), set()
    for q in range(len(b.pts)):
        if q not in ref:
            assert status[q] == R.FEW_VIEWS and np.array_equal(pts[q], b.pts[q])
            assert summ[q].termination_type == "CONVERGENCE" and summ[q].num_iterations == 0
            continue
        check_point(q, pts[q], summ[q], ref[q])
        its.add(summ[q].num_iterations)
        terms.add(summ[q].termination_type)
    print(f"scene {sc}: iterations {min(its)}..{max(its)}, terminations {sorted(terms)}")


def test_refinement_no_loss_no_scaling_and_iteration_cap(solver, oracle_lib):
    sc = (6, 4, 12)
    b = get_scene(sc)
    pts, _, summ = run(solver, b, pts_init=b.pts, refine=True, huber_a=0.0,
                       options=Options(max_num_iterations=3, jacobi_scaling=False))
    ref = oracle_solves(oracle_lib, sc, "given", max_num_iterations=3, jacobi_scaling=0, huber_a=0.0)
    for q in ref:
        check_point(q, pts[q], summ[q], ref[q])


# ---------------------------------------------------------------------------
# 3. DLT + refine: cost and point against the oracle started at the SVD point
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sc", ALL_SCENES)
def test_dlt_then_refine_matches_oracle_from_the_svd_point(solver, oracle_lib, sc):
    b = get_scene(sc)
    pts, _, summ = run(solver, b, refine=True, options=Options(max_num_iterations=20))
    ref = oracle_solves(oracle_lib, sc, "svd", max_num_iterations=20)
    for q in ref:
        check_point(q, pts[q], summ[q], ref[q], counts=False)


# ---------------------------------------------------------------------------
# 4. statuses: exactly the float32 restatement at the device's own point
# ---------------------------------------------------------------------------
def degenerate_batch():
    """Scene (6, 4, 12) plus one point seen twice by the same camera at the
    same pixel: identical centres and rays, no point is determined."""
    b = R.scene(6, 4, 12)
    cam, uv = b.obs_cam[:1], b.obs_uv[:1]
    return dict(extr=b.extr, K=b.K, cam_center=b.cam_center,
                obs_offset=np.append(b.obs_offset, b.obs_offset[-1] + 2).astype(np.int32),
                obs_cam=np.concatenate([b.obs_cam, cam, cam]), obs_uv=np.concatenate([b.obs_uv, uv, uv]))


def test_statuses_equal_the_float_restatement_at_the_device_point(solver):
    seen = np.zeros(6, int)
    for sc in ALL_SCENES:
        b = get_scene(sc)
        scale = R.octave_scales(b, 99)
        for refine in (False, True):
            for rule in (0, 1):
                pts, status, summ = run(solver, b, obs_scale=scale, refine=refine, behind_rule=rule,
                                        options=Options(max_num_iterations=20), with_summaries=True)
                failed = [s.termination_type == "FAILURE" for s in summ]
                want = R.batch_statuses(pts, b, scale, failed=failed, behind_rule=rule)
                assert np.array_equal(status, want), (sc, refine, rule, np.flatnonzero(status != want))
                seen += np.bincount(status, minlength=6)
        # the tests one by one, and without octave scales
        for checks in (R.CHECK_CHEIRALITY, R.CHECK_CHI2, R.CHECK_SCALE, 0):
            pts, status, _ = run(solver, b, checks=checks)
            assert np.array_equal(status, R.batch_statuses(pts, b, None, checks=checks)), (sc, checks)
    d = degenerate_batch()
    pts, status, _ = solver.triangulate(d["extr"], d["K"], d["obs_offset"], d["obs_cam"], d["obs_uv"],
                                        cam_center=d["cam_center"])
    assert status[-1] == R.DEGENERATE and not np.all(np.isfinite(pts[-1]))
    pts, status, summ = solver.triangulate(d["extr"], d["K"], d["obs_offset"], d["obs_cam"], d["obs_uv"],
                                           cam_center=d["cam_center"], refine=True)
    assert status[-1] == R.DEGENERATE and summ[-1].termination_type == "FAILURE"
    seen += np.bincount(status[-1:], minlength=6)
    assert np.all(seen > 0), seen      # every class occurred: the test cannot pass empty


def test_min_views(solver):
    b = R.ragged_scene()
    _, status, _ = run(solver, b, min_views=8)
    nv = np.diff(b.obs_offset)
    assert np.all((status == R.FEW_VIEWS) == (nv < 8))


# ---------------------------------------------------------------------------
# 5. device cross-check: one-point windows through ba_solve_window_batch
# ---------------------------------------------------------------------------
def test_matches_window_batch_on_one_point_windows(solver):
    b = R.scene(6, 4, 12)
    opts = Options(max_num_iterations=20)
    pts, _, summ = run(solver, b, pts_init=b.pts, refine=True, options=opts)
    probs = [R.one_point_problem(b, q, b.pts[q]) for q in range(32)]
    out, wsum = solver.solve_window_batch(probs, opts)
    for q in range(32):
        assert (summ[q].termination_type, summ[q].num_iterations, summ[q].num_successful_steps) == \
               (wsum[q].termination_type, wsum[q].num_iterations, wsum[q].num_successful_steps), q
        assert summ[q].final_cost == pytest.approx(wsum[q].final_cost, rel=1e-10)
        assert_close(pts[q], out[q][1][0], 1e-8, 1e-10, f"point {q} vs window")


# ---------------------------------------------------------------------------
# 6. bits
# ---------------------------------------------------------------------------
TERMS = ["CONVERGENCE", "NO_CONVERGENCE", "FAILURE"]


def summ_array(summ):
    return np.array([[s.initial_cost, s.final_cost, s.num_iterations, s.num_successful_steps,
                      s.num_unsuccessful_steps, TERMS.index(s.termination_type)] for s in summ])


@pytest.mark.parametrize("refine", [False, True])
def test_bits_do_not_depend_on_the_place_in_the_batch(solver, refine):
    b = R.scene(12, 12, 13)
    scale = R.octave_scales(b, 7)
    kw = dict(refine=refine, options=Options(max_num_iterations=20), with_summaries=True)
    pts, status, summ = run(solver, b, obs_scale=scale, **kw)
    pts2, status2, summ2 = run(solver, b, obs_scale=scale, **kw)
    assert pts.tobytes() == pts2.tobytes() and status.tobytes() == status2.tobytes()
    assert summ_array(summ).tobytes() == summ_array(summ2).tobytes()
    # a permuted batch (the points in another order, each keeping its views' order)
    perm = np.random.default_rng(4).permutation(len(b.pts))
    nv = np.diff(b.obs_offset)
    idx = np.concatenate([np.arange(b.obs_offset[q], b.obs_offset[q + 1]) for q in perm])
    off = np.concatenate([[0], np.cumsum(nv[perm])]).astype(np.int32)
    ptsp, statusp, summp = solver.triangulate(b.extr, b.K, off, b.obs_cam[idx], b.obs_uv[idx], cam_center=b.cam_center,
                                              obs_scale=scale[idx], huber_a=b.huber_a, **kw)
    assert ptsp.tobytes() == pts[perm].tobytes() and statusp.tobytes() == status[perm].tobytes()
    assert summ_array(summp).tobytes() == summ_array(summ)[perm].tobytes()
    # other neighbours: the first 37 points alone (a last wave that is partly empty)
    pt3, st3, _ = solver.triangulate(b.extr, b.K, b.obs_offset[:38], b.obs_cam, b.obs_uv, cam_center=b.cam_center,
                                     obs_scale=scale, huber_a=b.huber_a, **kw)
    assert pt3.tobytes() == pts[:37].tobytes() and st3.tobytes() == status[:37].tobytes()


def test_solve_is_untouched_by_a_triangulate_in_between(solver):
    p = make_synthetic(6, 300, 4, seed=31)
    b = R.scene(6, 4, 12)
    fields = ["iteration", "step_is_valid", "step_is_successful", "cost", "cost_change", "gradient_max_norm",
              "gradient_norm", "step_norm", "relative_decrease", "trust_region_radius", "model_cost_change"]

    def solve(between):
        solver.set_problem(p)
        if between:
            run(solver, b, refine=True)
        solver.solve(Options(max_num_iterations=6))
        cams, pts = solver.params()
        return [[r[f] for f in fields] for r in solver.iteration_log()], cams, pts

    log0, c0, x0 = solve(False)
    log1, c1, x1 = solve(True)
    assert log0 == log1 and c0.tobytes() == c1.tobytes() and x0.tobytes() == x1.tobytes()
    # ... and between set_problem + solve and get_params
    solver.set_problem(p)
    solver.solve(Options(max_num_iterations=6))
    run(solver, b)
    c2, x2 = solver.params()
    assert c2.tobytes() == c0.tobytes() and x2.tobytes() == x0.tobytes()


# ---------------------------------------------------------------------------
# 7. errors
# ---------------------------------------------------------------------------
def test_errors_name_the_culprit_and_leave_the_context_usable(solver):
    b = R.scene(2, 2, 11)
    good = dict(extr=b.extr, K=b.K, obs_offset=b.obs_offset, obs_cam=b.obs_cam, obs_uv=b.obs_uv)

    def call(match, **kw):
        a = dict(good, cam_center=b.cam_center)
        a.update(kw)
        with pytest.raises(BAError, match=match) as e:
            solver.triangulate(a.pop("extr"), a.pop("K"), a.pop("obs_offset"), a.pop("obs_cam"), a.pop("obs_uv"), **a)
        assert e.value.status == 1      # BA_ERR_INVALID_ARGUMENT

    off = b.obs_offset.copy()
    off[5] = off[4] - 1
    call("decreases at point 4", obs_offset=off)
    off = b.obs_offset.copy()
    off[0] = 1
    call(r"obs_offset\[0\]", obs_offset=off)
    cam = b.obs_cam.copy()
    cam[17] = 2
    call(r"obs_cam\[17\] = 2 out of range", obs_cam=cam)
    cam[17] = -1
    call(r"obs_cam\[17\] = -1 out of range", obs_cam=cam)
    call("pts_init is null", init=N.TRI_INIT_GIVEN)
    call("cam_center is null", cam_center=None)
    call("unknown init", init=2)
    call("unknown refine", refine=2)
    call("unknown behind_rule", behind_rule=2)
    call("unknown checks", checks=8)
    call("min_views", min_views=-1)
    call("BA_DENSE_SCHUR", refine=True, options=Options(linear_solver_type="ITERATIVE_SCHUR"))
    call("BA_FP64", refine=True, options=Options(precision="MIXED_FP32"))
    # NULL required arrays, through the C ABI
    lib, h = solver.lib, solver.h
    pts, st = np.zeros((len(b.pts), 3)), np.zeros(len(b.pts), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def raw(**null):
        f = dict(extr=p(b.extr), cam_center=p(b.cam_center), K=p(b.K), obs_offset=p(b.obs_offset), obs_cam=p(b.obs_cam),
                 obs_uv=p(b.obs_uv))
        f.update(null)
        tb = N.ba_tri_batch(n_cams=2, n_pts=len(b.pts), obs_scale=None, pts_init=None, huber_a=b.huber_a, **f)
        return lib.ba_triangulate(h, C.byref(tb), None, None, null.get("pts_out", p(pts)), null.get("status", p(st)),
                                  None)

    assert raw() == 0
    for name in ("extr", "K", "obs_offset", "obs_cam", "obs_uv"):
        assert raw(**{name: None}) == 1, name
        assert b"null" in lib.ba_last_error(h)
    tb = N.ba_tri_batch(n_cams=2, n_pts=len(b.pts), extr=p(b.extr), cam_center=p(b.cam_center), K=p(b.K),
                        obs_offset=p(b.obs_offset), obs_cam=p(b.obs_cam), obs_uv=p(b.obs_uv), huber_a=b.huber_a)
    assert lib.ba_triangulate(h, C.byref(tb), None, None, None, p(st), None) == 1
    assert lib.ba_triangulate(h, C.byref(tb), None, None, p(pts), None, None) == 1
    assert lib.ba_triangulate(h, None, None, None, p(pts), p(st), None) == 1
    # the scale test off: cam_center may be NULL
    solver.triangulate(**good, checks=R.CHECK_CHEIRALITY | R.CHECK_CHI2)
    # the context still solves, and an empty batch is BA_OK
    pts, status, _ = run(solver, b)
    assert np.all(np.isfinite(pts))
    e_pts, e_st, e_sum = solver.triangulate(b.extr, b.K, np.zeros(1, np.int32), b.obs_cam[:0], b.obs_uv[:0],
                                            cam_center=b.cam_center, refine=True)
    assert e_pts.shape == (0, 3) and e_st.shape == (0,) and e_sum == []
    tb0 = N.ba_tri_batch(n_cams=0, n_pts=0)
    assert lib.ba_triangulate(h, C.byref(tb0), None, None, None, None, None) == 0
    times = solver.triangulate_times()
    assert times.shape == (3,) and np.all(times >= 0) and times[2] >= times[0]


# ---------------------------------------------------------------------------
# 8. the staging arenas of the batch entry points
# ---------------------------------------------------------------------------
def test_staging_arenas_grow_shrink_and_interleave_bitwise():
    """One context through triangulate small -> large -> small, a window
    batch, pose batches large -> small, a prune and the small triangulate
    again: each arena grows, is reused for a smaller call, and the features
    interleave.  Every result equals, bit for bit, the same call on a fresh
    context."""
    from bundleadjustment_amd import problem as bp
    from test_pose_batch import batch_of, f2f_problem

    def tri_scene(nc, npts, k, seed):
        return R.triangulation_batch(R.all_fixed(make_synthetic(nc, npts, k, seed=seed, perturb=None, anchor=False)))

    small, large = tri_scene(2, 3, 2, 41), tri_scene(8, 300, 4, 42)
    windows = [bp.fix_camera(make_synthetic(4, 60, 3, seed=43), 1), bp.fix_camera(make_synthetic(3, 40, 3, seed=44), 1)]
    pose40 = batch_of([f2f_problem(20 + 7 * i, seed=500 + i) for i in range(40)])
    pose5 = batch_of([f2f_problem(30 + i, seed=600 + i) for i in range(5)])
    pt_of_obs = np.repeat(np.arange(len(large.pts)), np.diff(large.obs_offset))[:50]
    uv50 = large.obs_uv[:50].copy()
    uv50[::7] += 50.0                           # (gross keypoints: both verdicts occur)
    prune50 = (large.extr, large.cam_center, large.K, large.obs_cam[:50], large.pts[pt_of_obs].astype(np.float32),
               uv50, np.ones(50, np.float32), np.tile(np.float32([0.0, 100.0]), (50, 1)))
    opts = Options(max_num_iterations=10)

    def tri(b):
        def call(s):
            pts, status, summ = run(s, b, refine=True, options=opts)
            return [pts.tobytes(), status.tobytes(), summ_array(summ).tobytes()]
        return call

    def window(s):
        out, summ = s.solve_window_batch(windows, opts)
        logs = [[r[f] for r in s.window_iteration_log(i) for f in sorted(r)] for i in range(len(windows))]
        return [a.tobytes() for cp in out for a in cp] + [summ_array(summ).tobytes(), np.float64(sum(logs, [])).tobytes()]

    def pose(batch):
        def call(s):
            out, summ = s.solve_pose_batch(*batch, opts)
            return [out.tobytes(), summ_array(summ).tobytes()]
        return call

    def prune(s):
        return [s.prune(*prune50).tobytes()]

    calls = {"tri3": tri(small), "tri300": tri(large), "window": window, "pose40": pose(pose40), "pose5": pose(pose5),
             "prune": prune}
    fresh = {}
    for name, call in calls.items():
        with Solver(0) as s:
            fresh[name] = call(s)
    assert len(set(fresh["prune"][0])) > 1
    with Solver(0) as reused:                   # (its arenas start empty: the second call has to grow)
        for name in ("tri3", "tri300", "tri3", "window", "pose40", "pose5", "prune", "tri3"):
            assert calls[name](reused) == fresh[name], name
