"""GPU parity on irregular visibility: mixed track lengths, banded or uneven
reduced systems, fixed points among variable ones (structured_problems.py).

Every other GPU test solves a make_synthetic problem: one track length per
problem and an (almost) full co-visibility graph.  The scenes here are a few
thousand observations each and reach the branches those never do — the
memset of a sparse S before every step, the list of empty blocks, a diagonal
pair block beside a sparse S, the data-driven PCG fallback for tracks longer
than 64, lane groups of one wave finishing their points in different rounds,
pair blocks of one pair beside blocks of hundreds, an unobserved variable
camera inside the index range.  Solver.debug_plan() states which branch ran,
so a test asserts the branch instead of assuming it.

References: the oracle (oracle.linearize / reduced_system / solve), at the
bounds of test_gpu_blocks.py and test_gpu_parity.py.  The oracle's own
sensitivity to the observation order on these scenes
(test_structured_problems_cpu.py; the table in structured_problems.py) is
<= 2e-13 on a DENSE_SCHUR cost (compared at 1e-10), <= 6e-12 on an
ITERATIVE_SCHUR cost (1e-9), <= 7e-14 on S (1e-10) and <= 9e-11 (rtol at atol
1e-10) on the parameters after 6 iterations (1e-8): every figure >= 100 x
below the bound it is compared at, and no bound here is wider than the
project's default.
"""
import numpy as np
import pytest

from bundleadjustment_amd import Options, Solver
from bundleadjustment_amd._native import BAError
from conftest import assert_close, compare_logs
from structured_problems import SCENES, plan_conditions, scene
from test_gpu_blocks import close_to_scale, oracle_blocks

pytestmark = pytest.mark.gpu

RADIUS = 1e4
PRECONDITIONERS = ["JACOBI", "SCHUR_JACOBI"]
ORACLE_KW = {"DENSE_SCHUR": dict(), "JACOBI": dict(linear_solver=1, preconditioner_type=0),
             "SCHUR_JACOBI": dict(linear_solver=1, preconditioner_type=1)}


@pytest.fixture(scope="module")
def solver():
    s = Solver(0)
    yield s
    s.close()


_oracle_runs: dict = {}
_oracle_systems: dict = {}
_default_runs: dict = {}


def oracle_run(oracle_lib, name, kind, iters):
    """(cams, pts, summary, log) of the oracle on the shuffled scene: computed
    once per module, never modified."""
    key = (name, kind, iters)
    if key not in _oracle_runs:
        _oracle_runs[key] = oracle_lib.solve(scene(name), oracle_lib.default_options(max_num_iterations=iters,
                                                                                     **ORACLE_KW[kind]))
    return _oracle_runs[key]


def oracle_system(oracle_lib, name):
    if name not in _oracle_systems:
        p = scene(name)
        _oracle_systems[name] = (oracle_blocks(oracle_lib, p), oracle_lib.reduced_system(p, radius=RADIUS))
    return _oracle_systems[name]


def run_gpu(s, p, opts):
    s.set_problem(p)
    summ = s.solve(opts)
    cams, pts = s.params()
    return cams, pts, summ, s.iteration_log()


def gpu_options(kind, iters):
    if kind == "DENSE_SCHUR":
        return Options(max_num_iterations=iters)
    return Options(max_num_iterations=iters, linear_solver_type="ITERATIVE_SCHUR", preconditioner_type=kind)


def default_run(name, iters=6):
    """The DENSE_SCHUR trajectory of a fresh Solver with no switch set (call
    before any monkeypatch.setenv)."""
    if (name, iters) not in _default_runs:
        with Solver(0) as s:
            _default_runs[(name, iters)] = run_gpu(s, scene(name), Options(max_num_iterations=iters))
    return _default_runs[(name, iters)]


def assert_summaries_equal(summ, osum):
    assert summ.termination_type == osum["termination_type"]
    assert summ.num_iterations == osum["num_iterations"]
    assert summ.num_successful_steps == osum["num_successful_steps"]
    assert summ.num_unsuccessful_steps == osum["num_unsuccessful_steps"]


def assert_bitwise(a, b, what):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), what
    for f in ("cost", "step_is_successful", "step_is_valid", "gradient_max_norm", "trust_region_radius"):
        assert [x[f] for x in a[3]] == [x[f] for x in b[3]], (what, f)


def assert_blocks_match_oracle(got, ref, p):
    (Hpp, gp, Hcc, gc), (lhs, rhs) = ref
    close_to_scale(got["Hpp"], Hpp, 1e-11, "Hpp")
    close_to_scale(got["gp"], gp, 1e-11, "gp")
    close_to_scale(got["Hcc"], Hcc, 1e-11, "Hcc")
    close_to_scale(got["gc"], gc, 1e-11, "gc")
    n = got["n"]
    assert lhs.shape == (n, n) and got["S"].shape == (n, n)
    tril = np.tril_indices(n)
    close_to_scale(got["S"][tril], lhs[tril], 1e-10, "S (lower)")
    d = np.arange(n)
    assert np.allclose(got["S"][d, d], lhs[d, d], rtol=1e-11, atol=0), "S diagonal"
    close_to_scale(got["rhs"], rhs, 1e-10, "rhs")
    # camera pairs with no common variable point: nothing may be left there
    covis = plan_conditions(p)["covis"]
    assert n == 6 * covis.shape[0]
    blocks = got["S"].reshape(n // 6, 6, n // 6, 6).transpose(0, 2, 1, 3)
    I, J = np.nonzero(np.tril(~covis, -1))
    assert np.all(blocks[I, J] == 0.0), "an S block without a co-observed point is not exactly zero"
    # constant and unobserved points carry no block
    fixed = np.zeros(p.n_pts, bool) if p.pt_fixed is None else p.pt_fixed != 0
    dead = fixed | (np.bincount(p.obs_pt, minlength=p.n_pts) == 0)
    assert np.all(got["Hpp"][dead] == 0.0) and np.all(got["gp"][dead] == 0.0)


def test_debug_plan_statuses_and_laziness():
    """No problem: BA_ERR_NO_PROBLEM; a NULL out: BA_ERR_INVALID_ARGUMENT;
    after set_problem alone nothing is built (the call builds nothing
    itself), and a short n writes only the first values."""
    import ctypes as C
    with Solver(0) as s:
        with pytest.raises(BAError) as e:
            s.debug_plan()
        assert e.value.status == 4
        s.set_problem(scene("band40x"))
        assert s.lib.ba_debug_plan(s.h, None, 4) == 1
        plan = s.debug_plan()
        assert plan["nvc"] == 38 and plan["jrfree"] == 1
        assert plan["have_dense"] == plan["have_pcg"] == plan["nblocks"] == plan["s_memset"] == plan["npchunks"] == 0
        out = (C.c_int32 * 3)(-7, -7, -7)
        assert s.lib.ba_debug_plan(s.h, out, 1) == 0 and list(out) == [38, -7, -7]
        assert s.debug_plan() == plan


# ---------------------------------------------------------------------------
# the blocks of one step, before and after a solve on the same context
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_blocks_match_oracle_and_survive_a_solve(oracle_lib, name):
    """Hpp, gp, Hcc, gc, S and rhs against the oracle (the bounds of
    test_gpu_blocks.py; the sums here are shorter than C3's), exact zeros
    where no pair writes, and the same blocks bit for bit after six LM
    iterations have factored S in place on the same context: a stale region
    of S, a counter or a flag left by the factorisation would show."""
    p = scene(name)
    cond = plan_conditions(p)
    with Solver(0) as s:
        s.set_problem(p)
        a = s.debug_blocks(RADIUS)
        plan = s.debug_plan()
        s.solve(Options(max_num_iterations=6))
        s.set_params(p.cams, p.pts)
        b = s.debug_blocks(RADIUS)
    assert_blocks_match_oracle(a, oracle_system(oracle_lib, name), p)
    for k in ("Hpp", "gp", "Hcc", "gc", "S", "rhs"):
        assert np.array_equal(a[k], b[k]), f"{k} differs after a solve on the same context"
    # the host plan is the one the structure calls for ...
    assert plan["have_dense"] == 1 and plan["jrfree"] == 1 and plan["wcompact"] == 1
    assert plan["nvc"] == cond["nvc"]
    assert plan["s_memset"] == int(cond["s_memset"]) and plan["dup_diag"] == int(cond["dup_diag"])
    assert plan["neblocks"] == (0 if cond["s_memset"] else cond["nempty"])
    assert plan["nblocks"] >= cond["nfull"]
    # ... and the branch the scene is meant for
    if name in ("band40", "band40x", "band40dup", "band201"):
        assert plan["s_memset"] == 1 and plan["ov_ok"] == 0
    if name == "band230":
        assert plan["neblocks"] > 0 and plan["s_memset"] == 0
    if name == "band40dup":
        assert plan["dup_diag"] == 1 and plan["nblocks"] > cond["nfull"]
    if cond["nvc"] <= 200:
        assert plan["chol_persist"] == 1


@pytest.mark.parametrize("name", ["mixed70", "mixed66"])
def test_overlapped_pass_on_uneven_blocks_is_bitwise_the_separate_passes(monkeypatch, name):
    """Every camera pair co-observed, tracks from 1 or 2 to every camera: the
    overlapped form applies (ov_ok), and the reduced system its work items
    form (BA_DEBUG_OV_PASS=1, twice: cumulative counters) is bitwise the
    separate passes'."""
    p = scene(name)
    with Solver(0) as s:
        s.set_problem(p)
        a = s.debug_blocks(RADIUS)
        assert s.debug_plan()["ov_ok"] == 1
        monkeypatch.setenv("BA_DEBUG_OV_PASS", "1")
        b = s.debug_blocks(RADIUS)
        c = s.debug_blocks(3e2)
        monkeypatch.delenv("BA_DEBUG_OV_PASS")
        d = s.debug_blocks(3e2)
    tril = np.tril_indices(a["n"])
    assert np.array_equal(a["S"][tril], b["S"][tril]) and np.array_equal(a["rhs"], b["rhs"])
    assert np.array_equal(c["S"][tril], d["S"][tril]) and np.array_equal(c["rhs"], d["rhs"])


# ---------------------------------------------------------------------------
# per-observation r and J in the caller's (shuffled) order
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed70", "band230", "ptfix40"])
def test_linearize_in_caller_order_matches_oracle(solver, oracle_lib, name):
    p = scene(name)
    solver.set_problem(p)
    r, J, cost = solver.linearize()
    ro, Jo, costo, ok = oracle_lib.linearize(p)
    assert ok
    assert_close(r, ro, 1e-12, 1e-9, "corrected residual")
    assert_close(J, Jo, 1e-11, 1e-9, "corrected jacobian")
    assert cost == pytest.approx(costo, rel=1e-12)
    rr, _ = solver.residuals()
    assert_close(rr, oracle_lib.residuals(p), 1e-12, 1e-9, "raw residual")


# ---------------------------------------------------------------------------
# DENSE_SCHUR trajectories
# ---------------------------------------------------------------------------
def assert_untouched(name, p, cams, pts):
    if name != "ptfix40":
        return
    fixed = p.pt_fixed != 0
    unseen = np.bincount(p.obs_pt, minlength=p.n_pts) == 0
    assert fixed.any() and np.array_equal(pts[fixed], p.pts[fixed]), "a constant point moved"
    assert np.array_equal(pts[unseen], p.pts[unseen]), "an unobserved point moved"
    assert np.array_equal(cams[20], p.cams[20]), "the unobserved camera moved"
    assert np.array_equal(cams[p.cam_fixed != 0], p.cams[p.cam_fixed != 0])


@pytest.mark.parametrize("name,iters", [("band40x", 6), ("band40dup", 6), ("mixed66", 6), ("band201", 6),
                                        ("band230", 6), ("ptfix40", 6), ("band40", 1), ("mixed70", 1)])
def test_dense_trajectory_matches_oracle(solver, oracle_lib, name, iters):
    """compare_logs at its defaults (costs 1e-10), equal summaries, parameters
    at the project's rtol 1e-8 / atol 1e-10 (the oracle-vs-oracle parameter
    sensitivity of every scene is <= 9e-11 < 1e-10, so the default holds).
    The scenes with 1-tracks take one step: the back substitution of points
    seen once."""
    p = scene(name)
    cams, pts, summ, glog = run_gpu(solver, p, Options(max_num_iterations=iters))
    oc, op, osum, olog = oracle_run(oracle_lib, name, "DENSE_SCHUR", iters)
    assert len(glog) == len(olog) == iters + 1
    compare_logs(glog, olog)
    assert_summaries_equal(summ, osum)
    assert summ.final_cost == pytest.approx(osum["final_cost"], rel=1e-10)
    assert_close(cams, oc, 1e-8, 1e-10, "cameras")
    assert_close(pts, op, 1e-8, 1e-10, "points")
    if name in ("band201", "band230"):
        assert any(not r["step_is_successful"] for r in glog), "no rejected step: the re-linearise path did not run"
    assert_untouched(name, p, cams, pts)


# ---------------------------------------------------------------------------
# ITERATIVE_SCHUR trajectories and the data-driven plan
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pc", PRECONDITIONERS)
@pytest.mark.parametrize("name", ["mixed66", "mixed70", "band201", "band230", "band40dup", "ptfix40"])
def test_iterative_trajectory_matches_oracle(solver, oracle_lib, name, pc):
    p = scene(name)
    cams, pts, summ, glog = run_gpu(solver, p, gpu_options(pc, 6))
    plan = solver.debug_plan()
    oc, op, osum, olog = oracle_run(oracle_lib, name, pc, 6)
    assert len(glog) == len(olog) == 7
    compare_logs(glog, olog, rtol_cost=1e-9)
    assert [r["linear_solver_iterations"] for r in glog] == [r["linear_solver_iterations"] for r in olog]
    assert_untouched(name, p, cams, pts)
    assert plan["have_pcg"] == 1 and plan["wcompact"] == 0 and plan["jdiag"] == 1
    on = (plan["pcgc"], plan["pacc"], plan["pcgjf"])
    if name == "mixed66":       # the longest track is exactly 64: still chunked
        assert plan["npchunks"] > 0 and on[:2] == (1, 1)
    elif name == "mixed70":     # a track of 65 and one of 70: the data-driven fallback
        assert plan["npchunks"] == 0 and on == (0, 0, 0)
    elif name == "band201":     # beyond the LDS camera table, short tracks
        assert plan["npchunks"] > 0 and plan["pcgjf"] == 1
    elif name == "band230":     # beyond the table, tracks of 100
        assert plan["npchunks"] == 0 and plan["pcgjf"] == 0
    elif name == "band40dup":   # duplicate (camera, point) pairs keep the 18-value records
        assert plan["pcg_ndup"] == plan_conditions(p)["ndup"] > 0 and plan["pcgc"] == 0


@pytest.mark.parametrize("pc", PRECONDITIONERS)
def test_iterative_value_pair_passes_on_mixed_tracks(oracle_lib, pc, monkeypatch):
    """mixed66 with BA_PCG_SEG=0 (the fallback mixed70 takes because of its
    data): the same accept sequence as the chunked passes, costs within 1e-9."""
    p = scene("mixed66")
    with Solver(0) as s:
        ref = run_gpu(s, p, gpu_options(pc, 6))
        assert s.debug_plan()["npchunks"] > 0
    monkeypatch.setenv("BA_PCG_SEG", "0")
    with Solver(0) as s:
        got = run_gpu(s, p, gpu_options(pc, 6))
        plan = s.debug_plan()
    assert plan["npchunks"] == 0 and (plan["pcgc"], plan["pacc"], plan["pcgjf"]) == (0, 0, 0)
    assert [r["step_is_successful"] for r in got[3]] == [r["step_is_successful"] for r in ref[3]]
    np.testing.assert_allclose([r["cost"] for r in got[3]], [r["cost"] for r in ref[3]], rtol=1e-9)


# ---------------------------------------------------------------------------
# switches stay neutral on irregular structure
# ---------------------------------------------------------------------------
SPEC_OFF = {"BA_SPEC_LIN": "0", "BA_SCAL_SPIN": "0", "BA_NORMS_FOLD": "0"}


@pytest.mark.parametrize("env,name", [({"BA_CHOL_PERSIST": "0"}, "band40x"), ({"BA_CHOL_PERSIST": "0"}, "mixed70"),
                                      ({"BA_CHOL_OVERLAP": "0"}, "mixed70"),
                                      ({"BA_DIAG_IN_PAIRS": "0"}, "band40x"), ({"BA_DIAG_IN_PAIRS": "0"}, "band230"),
                                      ({"BA_PAIRS_DMA": "0"}, "band230"), (SPEC_OFF, "band201")],
                         ids=lambda v: "+".join(v) if isinstance(v, dict) else v)
def test_switch_is_bitwise_neutral(monkeypatch, env, name):
    """What the C3 / C4 tests claim for these switches, on a sparse S
    (band40x, band201), on uneven pair blocks (mixed70) and on the list of
    empty blocks beyond the LDS camera table (band230): fresh contexts, six
    iterations, the same trajectory bit for bit."""
    ref = default_run(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with Solver(0) as s:
        got = run_gpu(s, scene(name), Options(max_num_iterations=6))
        plan = s.debug_plan()
    if "BA_CHOL_PERSIST" in env:
        assert plan["chol_persist"] == 0
    if env is SPEC_OFF:
        assert any(not r["step_is_successful"] for r in ref[3]), "no rejected step: the path is not exercised"
    assert_bitwise(ref, got, f"{name} {env}")


@pytest.mark.parametrize("name", ["band40x", "band230"])
def test_compact_w_records_match_full_blocks_on_bands(monkeypatch, name):
    """BA_WCOMPACT=0 (18-double W) associates the products differently: the
    same accept sequence, costs 1e-10, parameters 1e-8 / 1e-10."""
    a = default_run(name)
    monkeypatch.setenv("BA_WCOMPACT", "0")
    with Solver(0) as s:
        b = run_gpu(s, scene(name), Options(max_num_iterations=6))
        assert s.debug_plan()["wcompact"] == 0
    assert [r["step_is_successful"] for r in a[3]] == [r["step_is_successful"] for r in b[3]]
    np.testing.assert_allclose([r["cost"] for r in b[3]], [r["cost"] for r in a[3]], rtol=1e-10)
    np.testing.assert_allclose(b[0], a[0], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(b[1], a[1], rtol=1e-8, atol=1e-10)


# ---------------------------------------------------------------------------
# BA_JR=1: the kernels that store r and J (bench.py can select them)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed70", "band230"])
def test_stored_jacobian_kernels_match_oracle(oracle_lib, monkeypatch, name):
    """BA_JR=1, read when the problem is set: the blocks and a six-iteration
    trajectory against the oracle at the bounds of the J-free path."""
    p = scene(name)
    monkeypatch.setenv("BA_JR", "1")
    with Solver(0) as s:
        s.set_problem(p)
        got = s.debug_blocks(RADIUS)
        plan = s.debug_plan()
        cams, pts, summ, glog = run_gpu(s, p, Options(max_num_iterations=6))
    assert plan["jrfree"] == 0 and plan["wcompact"] == 0 and plan["jdiag"] == 0
    assert_blocks_match_oracle(got, oracle_system(oracle_lib, name), p)
    oc, op, osum, olog = oracle_run(oracle_lib, name, "DENSE_SCHUR", 6)
    compare_logs(glog, olog)
    assert_summaries_equal(summ, osum)
    assert_close(cams, oc, 1e-8, 1e-10, "cameras")
    assert_close(pts, op, 1e-8, 1e-10, "points")
