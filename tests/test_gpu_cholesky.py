"""Direct tests of the dense Cholesky + back substitution behind DENSE_SCHUR
(ba_chol*.hip, k_back_flow) through ba_debug_factor: a seeded SPD system of a
chosen order and conditioning is injected into the solver's own dispatch and
the factor, the block inverses and the solution that come back are checked
against the backward-error bounds of tests/cholesky_ref.py — at the orders
where the kernels change path (one partial tile, every 16-column sub-panel
boundary of the last block, n % 64 == 0 with its rhs-only tile row, the last
persistent and the first split orders) and in every form of the factorisation.

The scene only fixes the order n = 6 x variable observed cameras.

Bounds (cholesky_ref's module docstring derives them):
  factor_ratio <= 2
  solve_error  <= 4 n u cond_2(L)            (u = 2^-53)
  |y - y_ref| / |y_ref| <= 4 n u kappa       (covariance_ref.Reference.tolerance)

Measured on an MI355X (worst over the orders of each form; each test prints
its figures, `pytest -s`):
                          kappa = 1e2                    kappa = 1e10
  form          factor_ratio  solve_error      factor_ratio  solve_error
  persistent    0.083 (n=12)  5.7e-16 (n=1470) 0.033 (n=384) 1.7e-15
  per_step      0.083 (n=12)  5.7e-16 (n=1470) 0.033 (n=384) 1.7e-15
  flow          0.0032        6.0e-16 (n=1542) 0.0099        3.6e-15
  fused         0.0032        6.0e-16          0.0099        3.6e-15
  panels        0.0032        6.0e-16          0.0099        3.6e-15
(solve_error bounds: 6.5e-12 at n = 1470, 6.9e-8 at n = 1542 with kappa =
1e10.)  The forms of one family give identical figures: they are bitwise
equal (test_forms_agree_bitwise_on_injected_systems).
"""
import functools

import numpy as np
import pytest

import cholesky_ref as cr
from bundleadjustment_amd import Options, Solver, make_config, make_synthetic
from bundleadjustment_amd import problem as bp
from conftest import assert_close, compare_logs

pytestmark = pytest.mark.gpu

CB = 64
SPLIT_BLOCKS = 24   # kCholSplitBlocks (ba_chol.hip)
KNOBS = ("BA_CHOL_PERSIST", "BA_CHOL_FLOW", "BA_CHOL_FUSE", "BA_CHOL_SPIN_MAX", "BA_CHOL_OVERLAP")

# variable cameras -> order n = 6 nvc; T = ceil(n / 64) block columns, b = the last block's width
NVC = (1, 2, 3, 5, 8, 10,   # one partial tile: 6, 12, 18 (crosses sub-panel 0), 30, 48 (b % 16 == 0, m = 49), 60
       11, 13, 16, 21,      # T = 2: b = 2 (the floor of tile_fetch's clamp), 14, 32, 62 (m = 63)
       32, 43, 64,          # n % 64 == 0 (T = 3, 6: the rhs row a tile row of its own), T = 5 with b = 2
       245, 246, 256, 257)  # T = 23 (largest persistent), 24 (first split, b = 4), 24 with n % 64 == 0, 25 (b = 6)

FORMS_SMALL = {"persistent": {}, "per_step": {"BA_CHOL_PERSIST": "0"}}
FORMS_SPLIT = {"flow": {}, "fused": {"BA_CHOL_FLOW": "0"}, "panels": {"BA_CHOL_FLOW": "0", "BA_CHOL_FUSE": "0"}}


def forms_of(n):
    return FORMS_SMALL if (n + CB - 1) // CB < SPLIT_BLOCKS else FORMS_SPLIT


def cases(orders):
    return [pytest.param(n, f, id=f"{n}-{f}") for n in orders for f in forms_of(n)]


@functools.lru_cache(maxsize=None)
def scene(nvc):
    """nvc variable cameras, each observed; camera 0 is constant."""
    return make_synthetic(nvc + 1, max(4 * nvc, 48), 8, seed=0xC401 + nvc)


def set_form(monkeypatch, env):
    # (the BA_CHOL_* knobs are read when the dense structures are built: before the Solver)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def factor(monkeypatch, n, form, systems):
    """debug_factor of each (A, rhs) of `systems` on one fresh context of order n."""
    assert n % 6 == 0
    set_form(monkeypatch, forms_of(n)[form])
    with Solver(0) as s:
        s.set_problem(scene(n // 6))
        outs = [s.debug_factor(A, rhs) for A, rhs in systems]
    for o in outs:
        assert o["n"] == n == 6 * (n // 6)
    return outs


def check_v(V, n, form):
    """V_k is lower triangular where the form writes it, and the identity
    beyond the last block's order.  The persistent form stores only the 16x16
    blocks on and below the block diagonal of a FULL 64-block (the rest is
    never read); every other form, and the persistent form's partial last
    block, writes the whole 64 x 64."""
    T = (n + CB - 1) // CB
    assert V.shape == (T, CB, CB)
    iu = np.triu_indices(CB, 1)
    for k in range(T):
        b = min(CB, n - k * CB)
        if form == "persistent" and b == CB:
            for q in range(4):
                blk = V[k][16 * q:16 * q + 16, 16 * q:16 * q + 16]
                assert np.all(blk[np.triu_indices(16, 1)] == 0.0), (k, q)
        else:
            assert np.all(V[k][iu] == 0.0), k
        assert np.all(np.isfinite(np.tril(V[k])))
        if b < CB:
            pad = V[k].copy()
            pad[:b, :b] = np.eye(b)
            assert np.array_equal(pad, np.eye(CB)), k


def check_system(n, kappa, form, out):
    A, rhs = cr.system(n, kappa, n)
    ref = cr.system_reference(n, kappa, n)
    assert out["ok"]
    check_v(out["V"], n, form)
    c = cr.check(A, rhs, out)
    err = float(np.linalg.norm(out["y"] - ref) / np.linalg.norm(ref))
    # (for the record: the ratio with Higham's denominator alone, which has no
    # room for the explicit inverses: cholesky_ref's docstring)
    print(f"MEASURED n={n} kappa={kappa:g} form={form}: without E {cr.factor_ratio(A, rhs, c['L']):.3g}")
    print(f"MEASURED n={n} kappa={kappa:g} form={form}: factor_ratio {c['factor_ratio']:.3g} solve_error "
          f"{c['solve_error']:.3g} (bound {4.0 * n * cr.U * c['cond_L']:.3g}) y_error {err:.3g} "
          f"(bound {4.0 * n * cr.U * kappa:.3g})")
    assert c["factor_ratio"] <= 2.0
    assert c["solve_error"] <= 4.0 * n * cr.U * c["cond_L"]
    assert err <= 4.0 * n * cr.U * kappa


@pytest.mark.parametrize("n,form", cases([6 * v for v in NVC]))
def test_factor_and_solution_at_boundary_orders(monkeypatch, n, form):
    out, = factor(monkeypatch, n, form, [cr.system(n, 1e2, n)])
    check_system(n, 1e2, form, out)


@pytest.mark.parametrize("n,form", cases([384, 1542]))
def test_ill_conditioned_system(monkeypatch, n, form):
    out, = factor(monkeypatch, n, form, [cr.system(n, 1e10, n)])
    check_system(n, 1e10, form, out)


def bitwise_cases():
    out = []
    for n in (192, 1536):
        names = list(forms_of(n))
        out += [pytest.param(n, names[0], f, id=f"{n}-{f}") for f in names[1:]]
    return out


@pytest.mark.parametrize("n,ref_form,form", bitwise_cases())
def test_forms_agree_bitwise_on_injected_systems(monkeypatch, n, ref_form, form):
    """The forms run the same arithmetic in the same order per tile: on an
    injected dense system (not the scene-shaped matrices of the trajectory
    tests) the stored L rows, the lower triangles of V and y are bitwise
    equal: per-step against persistent at n = 192, fused / panels against
    flow at n = 1536."""
    sysm = [cr.system(n, 1e2, n)]
    a, = factor(monkeypatch, n, ref_form, sysm)
    b, = factor(monkeypatch, n, form, sysm)
    assert a["ok"] and b["ok"]
    dl = int(np.sum(a["L"] != b["L"]))
    dv = int(np.sum(np.tril(a["V"]) != np.tril(b["V"])))
    dy = int(np.sum(a["y"] != b["y"]))
    print(f"MEASURED bitwise n={n} {ref_form} vs {form}: differing entries L {dl} V {dv} y {dy}; "
          f"max |dL| {np.abs(a['L'] - b['L']).max():.3g} max |dy| {np.abs(a['y'] - b['y']).max():.3g}")
    assert dl == 0 and dv == 0 and dy == 0


@pytest.mark.parametrize("n,form", [(132, "per_step"), (132, "persistent"), (1542, "flow"), (1542, "panels")])
def test_non_positive_pivot_is_reported_at_every_position(monkeypatch, n, form):
    """A non-positive pivot (pivot j exactly -L0[j,j]^2, every earlier pivot
    untouched) is reported wherever it falls: both columns of a pivot pair of
    the paired sweep, every 16-column sub-panel, a later block column, the
    partial last block; so is a NaN on and off the diagonal.  The call itself
    succeeds (a non-positive-definite S is an ordinary event in LM: the step is
    invalid), and the context factors the next system as if nothing happened."""
    A, rhs = cr.system(n, 1e2, n)
    L0 = np.linalg.cholesky(A)
    js = [j for j in (0, 1, 15, 16, 17, 47, 63, 64, 65, 128, n - 2, n - 1) if j < n]
    systems = [(A, rhs)]
    for j in js:
        B = A.copy()
        B[j, j] -= 2.0 * L0[j, j] ** 2          # (cholesky_ref.make_indefinite, with L0 shared)
        systems.append((B, rhs))
    assert np.array_equal(systems[3][0], cr.make_indefinite(A, js[2]))
    for i, j in ((17, 17), (70, 3)):
        B = A.copy()
        B[i, j] = np.nan
        systems.append((B, rhs))
    systems.append((A, rhs))
    outs = factor(monkeypatch, n, form, systems)
    assert outs[0]["ok"]
    for what, o in zip([f"pivot {j}" for j in js] + ["nan diagonal", "nan off-diagonal"], outs[1:-1]):
        assert not o["ok"], what
    last = outs[-1]
    assert last["ok"]
    assert np.array_equal(last["L"], outs[0]["L"]) and np.array_equal(last["y"], outs[0]["y"])
    assert np.array_equal(np.tril(last["V"]), np.tril(outs[0]["V"]))


def run_solve(s, p, opts):
    s.set_problem(p)
    summ = s.solve(opts)
    cams, pts = s.params()
    return cams, pts, [(r["cost"], r["step_is_successful"]) for r in s.iteration_log()], summ


def test_debug_factor_leaves_the_context_unchanged(monkeypatch):
    set_form(monkeypatch, {})
    p = bp.fix_camera(make_config("c2", scale=0.25), 1)
    opts = Options(max_num_iterations=6)
    with Solver(0) as s:
        fresh = run_solve(s, p, opts)
    with Solver(0) as s:
        first = run_solve(s, p, opts)
        n = s.reduced_order()
        assert n == 6 * (p.n_cams - 2)
        A, rhs = cr.system(n, 1e2, n)
        blocks0 = s.debug_blocks()
        cov0 = s.covariance()
        f1 = s.debug_factor(A, rhs)
        f2 = s.debug_factor(A, rhs)
        f3 = s.debug_factor(cr.make_indefinite(A, n // 2), rhs)
        blocks1 = s.debug_blocks()
        cov1 = s.covariance()
        again = run_solve(s, p, opts)
    with Solver(0) as s:   # the dense structures built by debug_factor itself, before any solve
        s.set_problem(p)
        f4 = s.debug_factor(A, rhs)
        early = run_solve(s, p, opts)
    assert f1["ok"] and f2["ok"] and f4["ok"] and not f3["ok"] and f1["n"] == n
    for f in (f2, f4):
        assert np.array_equal(f1["L"], f["L"]) and np.array_equal(f1["y"], f["y"])
        assert np.array_equal(np.tril(f1["V"]), np.tril(f["V"]))
    assert blocks0["n"] == blocks1["n"] == n
    for k in ("Hpp", "gp", "Hcc", "gc", "S", "rhs"):
        assert np.array_equal(blocks0[k], blocks1[k]), k
    assert np.array_equal(cov0[0], cov1[0]) and np.array_equal(cov0[1], cov1[1])
    for r in (first, again, early):
        assert np.array_equal(fresh[0], r[0]) and np.array_equal(fresh[1], r[1])
        assert fresh[2] == r[2]
    assert len(fresh[2]) >= 2


def test_debug_factor_refuses_what_it_cannot_do():
    from bundleadjustment_amd._native import BAError
    with Solver(0) as s:
        with pytest.raises(BAError) as e:
            s._check(s.lib.ba_debug_factor(s.h, None, None, None, None, None, None), "ba_debug_factor")
        assert e.value.status == 4                     # BA_ERR_NO_PROBLEM
        p = make_synthetic(3, 48, 3, seed=5)
        for c in (1, 2):                               # every camera constant: n == 0
            bp.fix_camera(p, c)
        s.set_problem(p)
        assert s.reduced_order() == 0
        with pytest.raises(BAError) as e:
            s.debug_factor(np.zeros((0, 0)), np.zeros(0))
        assert e.value.status == 1                     # BA_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("form", ["persistent", "persistent_serial", "per_step"])
def test_one_step_of_a_solve_at_a_multiple_of_64(monkeypatch, oracle_lib, form):
    """End to end at n % 64 == 0 (32 variable cameras: n = 192): the rhs row is
    a tile row of its own, k_back_flow forms z_K = V_K A_{n,K}^T itself.  The
    LM trajectory against the oracle, in the persistent form (as a solve
    selects it: overlapped where it applies; and with the separate passes) and
    the per-step form."""
    set_form(monkeypatch, {"persistent": {}, "persistent_serial": {"BA_CHOL_OVERLAP": "0"},
                           "per_step": {"BA_CHOL_PERSIST": "0"}}[form])
    p = bp.fix_camera(make_synthetic(34, 1200, 8, seed=0xBA5E0192), 1)
    with Solver(0) as s:
        s.set_problem(p)
        assert s.reduced_order() == 192
        summ = s.solve(Options(max_num_iterations=4))
        cams, pts = s.params()
        glog = s.iteration_log()
    oc, op, osum, olog = oracle_lib.solve(p, oracle_lib.default_options(max_num_iterations=4))
    assert len(glog) >= 3
    compare_logs(glog, olog, rtol_cost=1e-10)
    assert_close(cams, oc, 1e-8, 1e-10, "cameras")
    assert_close(pts, op, 1e-8, 1e-10, "points")
