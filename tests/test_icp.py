"""GPU tests for ba_icp / ba_icp_nn: the correspondence pass equals the
brute-force float32 restatement (tests/icp_ref.py, itself checked against the
host program in test_icp_cpu.py) in index and in d2 bits, whatever the route,
the cell size and the sizes; the loop follows the restatement's states and
counts and meets its transforms and fitness within tolerances worked out from
the restatement's own sensitivity; a pair's bits do not depend on the batch;
gates, guesses, scale, the empty batch, argument errors and the reconstruction
error built on top."""
from functools import lru_cache

import numpy as np
import pytest

import icp_ref as R
from bundleadjustment_amd import Options, Solver, make_synthetic
from bundleadjustment_amd import reconstruction
from bundleadjustment_amd._native import BAError
from bundleadjustment_amd.io import write_ply_vertices

pytestmark = pytest.mark.gpu

HUGE_CELL, TINY_CELL = 1.0e6, 0.125          # one cell; at most one distinct lattice point per cell
ROUTES = (("GRID", HUGE_CELL), ("GRID", 0.0), ("GRID", TINY_CELL), ("BRUTE", 0.0), ("AUTO", 0.0))
N_SRC = (3, 63, 64, 65, 257)
N_TGT = (1, 2, 64, 65, 1000, 4000)


@pytest.fixture(scope="module")
def solver():
    s = Solver(0)
    yield s
    s.close()


def same_bits(a, b) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@lru_cache(maxsize=None)
def noisy():
    return R.noisy_scene()


@lru_cache(maxsize=None)
def noisy_ref():
    sc = noisy()
    return R.icp(sc.src, sc.tgt), R.icp(sc.src, sc.tgt, perturb=True)


@lru_cache(maxsize=None)
def clean_ref(scale=1.0):
    sc = R.clean_scene(scale=scale)
    return sc, R.icp(sc.src, sc.tgt, with_scale=int(scale != 1.0))


# ---------------------------------------------------------------------------
# 1. the correspondence pass
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.COARSE_KINDS)
@pytest.mark.parametrize("n_tgt", N_TGT)
def test_icp_nn_equals_the_restatement_on_the_coarse_scene(solver, kind, n_tgt):
    for n_src in N_SRC:
        sc = R.coarse_scene(n_src, n_tgt, kind)
        idx, d2 = R.nn_brute(sc.src, sc.tgt)
        assert (idx >= 0).all()
        for route, cell in ROUTES:
            gi, gd = solver.icp_nn([sc.src, sc.tgt], [[0, 1]], route=route, cell=cell)
            assert np.array_equal(gi, idx), (n_src, route, cell, np.flatnonzero(gi != idx)[:8])
            assert same_bits(gd, d2), (n_src, route, cell)


@pytest.mark.parametrize("shape", [(700, 1900), (257, 4000)])
def test_icp_nn_equals_the_restatement_on_the_noisy_scene(solver, shape):
    sc = R.noisy_scene(*shape)
    idx, d2 = R.nn_brute(sc.src, sc.tgt)
    for n_src in (*N_SRC, shape[0]):
        for route, cell in (*ROUTES, ("GRID", 0.01)):
            gi, gd = solver.icp_nn([sc.src[:n_src], sc.tgt], [[0, 1]], route=route, cell=cell)
            assert np.array_equal(gi, idx[:n_src]) and same_bits(gd, d2[:n_src]), (n_src, route, cell)


def test_icp_nn_gate_and_guess(solver):
    sc = noisy()
    guess = R.rigid(2.0, (1, 0, 0), (0.0, 0.01, -0.02)).astype(np.float32)
    cur = R.apply(guess[:3, :3], guess[:3, 3], sc.src)
    for dist in (np.inf, 0.05, 0.03):
        idx, d2 = R.nn_brute(cur, sc.tgt, np.float32(dist) * np.float32(dist))
        assert dist == np.inf or 0 < (idx < 0).sum() < idx.size
        for route, cell in ROUTES:
            gi, gd = solver.icp_nn([sc.src, sc.tgt], [[0, 1]], guess=[guess], route=route, cell=cell, max_corr_dist=dist)
            assert np.array_equal(gi, idx) and same_bits(gd, d2), (dist, route, cell)


# ---------------------------------------------------------------------------
# 2. the loop
# ---------------------------------------------------------------------------
def test_clean_scene_end_to_end(solver):
    sc, ref = clean_ref()
    for route in ("AUTO", "GRID"):
        res, mse = solver.icp([sc.src, sc.tgt], [[0, 1]], route=route)
        r = res[0]
        print(f"clean scene ({route}): state {r['state']}, iterations {r['iterations']}, fitness {r['fitness']:.3g}, "
              f"mse {mse[0, :r['iterations']]}")
        assert (r["state"], r["iterations"], r["n_corr"], r["converged"]) == (ref.state, ref.iterations, ref.n_corr, 1)
        assert ref.state == R.ABS_MSE
        for k in range(ref.iterations):
            if ref.mse[k] > 1e-10:
                assert mse[0, k] == pytest.approx(ref.mse[k], rel=1e-6)
        assert not mse[0, ref.iterations:].any()
        assert r["fitness"] < 1e-12
        assert np.abs(r["final"].astype(np.float64) - sc.truth).max() < 1e-6


def test_noisy_scene_end_to_end(solver):
    sc = noisy()
    a, b = noisy_ref()
    tol_fit, tol_fin = 10 * abs(a.fitness - b.fitness), 10 * float(np.abs(a.final - b.final).max())
    assert tol_fit > 0 and tol_fin > 0
    for route in ("AUTO", "GRID"):
        res, mse = solver.icp([sc.src, sc.tgt], [[0, 1]], route=route)
        r = res[0]
        print(f"noisy scene ({route}): fitness {r['fitness']:.9g} vs {a.fitness:.9g} (tolerance {tol_fit:.3g}), "
              f"final off by {np.abs(r['final'] - a.final).max():.3g} (tolerance {tol_fin:.3g})")
        assert r["state"] == R.ITERATIONS and r["converged"] == 1 and r["iterations"] == 10
        assert abs(r["fitness"] - a.fitness) <= tol_fit
        assert np.abs(r["final"] - a.final).max() <= tol_fin
        assert mse[0] == pytest.approx(a.mse, rel=1e-4)


def test_result_bits_do_not_depend_on_batch_order_sharing_route_or_cell(solver):
    n, c = noisy(), R.clean_scene()
    big = R.noisy_scene(900, 4000, seed=12)
    sets = [n.src, n.tgt, c.src, c.tgt, big.src, big.tgt, n.src[:300]]
    alone = {}
    for ps in ((0, 1), (2, 3), (4, 5), (6, 1), (2, 5)):
        res, mse = solver.icp([sets[ps[0]], sets[ps[1]]], [[0, 1]])
        alone[ps] = (res.tobytes(), mse.tobytes())
        assert res[0]["converged"] == 1
    order = [(4, 5), (0, 1), (6, 1), (2, 3), (2, 5), (0, 1)]
    for pairs in (order, order[::-1]):
        for kw in ({}, dict(route="GRID"), dict(route="BRUTE"), dict(route="GRID", cell=0.02), dict(route="GRID", cell=5.0)):
            res, mse = solver.icp(sets, pairs, **kw)
            for i, ps in enumerate(pairs):
                assert (res[i:i + 1].tobytes(), mse[i:i + 1].tobytes()) == alone[ps], (pairs, kw, i)
    again = solver.icp(sets, order)
    assert again[0].tobytes() == solver.icp(sets, order)[0].tobytes()


def test_max_corr_dist(solver):
    sc = noisy()
    res, mse = solver.icp([sc.src, sc.tgt], [[0, 1]], max_corr_dist=1e-6)
    r = res[0]
    assert R.icp(sc.src, sc.tgt, max_corr_dist=1e-6).state == R.NO_CORRESPONDENCES
    assert r["state"] == R.NO_CORRESPONDENCES and r["converged"] == 0 and r["iterations"] == 0 and r["n_corr"] < 3
    assert r["fitness"] == R.DBL_MAX and np.array_equal(r["final"], np.eye(4, dtype=np.float32)) and not mse.any()
    for dist in (0.03, 0.01):
        ref = R.icp(sc.src, sc.tgt, max_corr_dist=dist, max_iterations=1)
        assert 3 <= ref.n_corr < 700
        for route in ("GRID", "BRUTE"):
            res, mse = solver.icp([sc.src, sc.tgt], [[0, 1]], max_corr_dist=dist, max_iterations=1, route=route)
            assert res[0]["n_corr"] == ref.n_corr and res[0]["state"] == R.ITERATIONS
            assert mse[0, 0] == pytest.approx(ref.mse[0], rel=1e-12)
            assert np.abs(res[0]["final"] - ref.final).max() < 1e-6
    # the fitness range gates the fitness alone; a point at the range's edge may fall either side, and each
    # such point moves the mean by at most range / kept
    ref = R.icp(sc.src, sc.tgt, fitness_max_range=1e-3)
    kept = int((ref.idx >= 0).sum())
    res, _ = solver.icp([sc.src, sc.tgt], [[0, 1]], fitness_max_range=1e-3)
    assert 100 < kept < 700 and res[0]["iterations"] == 10 and ref.fitness < 1e-3
    assert abs(res[0]["fitness"] - ref.fitness) <= 2 * 1e-3 / kept
    res, _ = solver.icp([sc.src, sc.tgt], [[0, 1]], fitness_max_range=0.0)
    assert res[0]["converged"] == 1 and res[0]["fitness"] == R.DBL_MAX


def test_guess_is_honoured(solver):
    sc, _ = clean_ref()
    guess = sc.truth.astype(np.float32)
    ref = R.icp(sc.src, sc.tgt, guess=guess)
    res, mse = solver.icp([sc.src, sc.tgt], [[0, 1]], guess=[guess])
    r = res[0]
    assert ref.iterations < clean_ref()[1].iterations and ref.mse[0] < 1e-10       # it starts at the answer
    assert (r["state"], r["iterations"], r["n_corr"]) == (ref.state, ref.iterations, ref.n_corr)
    assert r["fitness"] < 1e-12 and np.abs(r["final"].astype(np.float64) - sc.truth).max() < 1e-6
    # a guess far from the answer leads elsewhere than no guess
    off = R.rigid(40.0, (0, 1, 0), (0.3, 0.0, 0.0)).astype(np.float32)
    res2, _ = solver.icp([sc.src, sc.tgt], [[0, 1], [0, 1]], guess=[off, np.eye(4)])
    ref2 = R.icp(sc.src, sc.tgt, guess=off)
    assert res2[0]["iterations"] == ref2.iterations and res2[0]["state"] == ref2.state
    assert np.abs(res2[0]["final"] - ref2.final).max() < 1e-3
    assert res2[1:].tobytes() == solver.icp([sc.src, sc.tgt], [[0, 1]])[0].tobytes()


def test_with_scale_recovers_a_known_scale(solver):
    sc, ref = clean_ref(1.25)
    res, _ = solver.icp([sc.src, sc.tgt], [[0, 1]], with_scale=1)
    r = res[0]
    M = r["final"][:3, :3].astype(np.float64)
    assert r["converged"] == 1 and r["state"] == ref.state and r["iterations"] == ref.iterations
    assert np.cbrt(np.linalg.det(M)) == pytest.approx(1.25, abs=1e-6)
    assert np.abs(r["final"].astype(np.float64) - sc.truth).max() < 2e-6 and r["fitness"] < 1e-11
    # without the option the scale stays 1 and the fit is poor
    res, _ = solver.icp([sc.src, sc.tgt], [[0, 1]])
    assert np.linalg.det(res[0]["final"][:3, :3].astype(np.float64)) == pytest.approx(1.0, abs=1e-5)
    assert res[0]["fitness"] > 1e-4


def test_empty_batch_and_times(solver):
    res, mse = solver.icp([], np.zeros((0, 2)))
    assert res.shape == (0,) and mse.shape[0] == 0
    res, mse = solver.icp([noisy().src], np.zeros((0, 2)))
    assert res.shape == (0,)
    sc = noisy()
    solver.icp([sc.src, sc.tgt], [[0, 1]])
    t = solver.icp_times()
    assert t.shape == (4,) and (t > 0).all() and t[1] <= t[2] and t[3] == pytest.approx(t[1] / 11)


# ---------------------------------------------------------------------------
# 3. errors and the context
# ---------------------------------------------------------------------------
def test_errors_name_the_culprit_and_leave_a_following_solve_untouched(solver):
    p = make_synthetic(6, 300, 4, seed=31)
    solver.set_problem(p)
    solver.solve(Options(max_num_iterations=6))
    want = solver.params()
    sc = noisy()
    good = dict(sets=[sc.src, sc.tgt], pairs=[[0, 1]])

    def refused(what, sets=good["sets"], pairs=good["pairs"], guess=None, **kw):
        for call in (solver.icp, solver.icp_nn):
            with pytest.raises(BAError) as e:
                call(sets, pairs, guess, **kw)
            assert e.value.status == 1 and what in str(e.value), str(e.value)

    solver.set_problem(p)
    bad = sc.src.copy()
    bad[5, 0] = np.nan
    refused("set 0 point 5 is not finite", sets=[bad, sc.tgt])
    refused("source set 0 has fewer than 3 points", sets=[sc.src[:2], sc.tgt])
    refused("target set 1 is empty", sets=[sc.src, sc.tgt[:0]])
    refused("pair 1 names a set out of range", pairs=[[0, 1], [2, 1]])
    g = np.eye(4, dtype=np.float32)
    g[0, 0] = np.inf
    refused("guess is not finite", guess=[g])
    for kw, what in ((dict(max_iterations=0), "max_iterations"), (dict(min_correspondences=1), "min_correspondences"),
                     (dict(max_corr_dist=-1.0), "max_corr_dist"), (dict(fitness_max_range=np.nan), "fitness_max_range"),
                     (dict(cell=-1.0), "cell"), (dict(with_scale=3), "with_scale"), (dict(route=7), "route"),
                     (dict(mse_abs_eps=np.nan), "epsilon")):
        refused(what, **kw)
    with pytest.raises(BAError) as e:
        solver.icp_nn(good["sets"], good["pairs"], pair=1)
    assert e.value.status == 1 and "pair 1" in str(e.value)
    with pytest.raises(TypeError):
        solver.icp(good["sets"], good["pairs"], nonsense=1)
    solver.icp(**good)                      # a good call in between
    solver.solve(Options(max_num_iterations=6))
    got = solver.params()
    assert want[0].tobytes() == got[0].tobytes() and want[1].tobytes() == got[1].tobytes()


# ---------------------------------------------------------------------------
# 4. the reconstruction error
# ---------------------------------------------------------------------------
def test_reconstruction_error_against_a_ply(solver, tmp_path):
    sc = noisy()
    a, b = noisy_ref()
    pose = R.rigid(25.0, (0.2, 1.0, -0.4), (1.5, -0.7, 3.0))
    world = (1.7 * sc.src.astype(np.float64) @ pose[:3, :3].T + pose[:3, 3]).astype(np.float32)   # the map: posed and off scale
    for binary in (True, False):
        ply = tmp_path / f"target{int(binary)}.ply"
        write_ply_vertices(ply, sc.tgt, binary=binary)
        want, ref = R.reconstruction_error(world, sc.tgt, pose)
        got = reconstruction.reconstruction_error(world, ply, pose, solver=solver)
        print(f"reconstruction error {got['error']:.9g} vs {want:.9g}; scale {got['scale']:.6g}")
        assert got["converged"] and got["state"] == ref.state and got["iterations"] == ref.iterations
        assert (got["n_source"], got["n_target"]) == (700, 1900)
        # the same tolerance as the noisy scene, scaled to this pair's fitness
        assert abs(got["error"] - want) <= 10 * abs(a.fitness - b.fitness) * max(want / a.fitness, 1.0)
        assert np.abs(got["final"] - ref.final).max() <= 10 * float(np.abs(a.final - b.final).max())
    fail = reconstruction.reconstruction_error(world, sc.tgt, pose, solver=solver, max_corr_dist=1e-7)
    assert not fail["converged"] and fail["error"] == R.FLT_MAX
