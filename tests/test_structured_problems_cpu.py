"""CPU tests of the structured scenes (structured_problems.py): each scene has
the structure its GPU test relies on, the shuffled and unshuffled builds are
one problem, and the oracle's own sensitivity to the observation order — the
yardstick for the GPU parity tolerances — stays far below them.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from bundleadjustment_amd import _native as N
from structured_problems import SCENES, plan_conditions, scene

K_LIN_LDS_CAMS = 200    # ba_kernels.h kLinLdsCams: the LDS camera table's capacity
ORACLE_KINDS = {"dense": dict(), "iter": dict(linear_solver=1, preconditioner_type=1)}


def test_scene_list_is_the_documented_one():
    assert list(SCENES) == ["band40", "band40x", "band40dup", "mixed70", "mixed66", "band201", "band230", "ptfix40"]


@pytest.mark.parametrize("name", list(SCENES))
def test_scene_reaches_its_branch(name):
    """The path conditions of ensure_dense / ensure_pcg, recomputed in numpy."""
    p = scene(name)
    c = plan_conditions(p)
    track = np.bincount(p.obs_pt, minlength=p.n_pts)
    assert p.cam_fixed[0] and p.cam_fixed[1], "cameras 0 and 1 anchored: no free gauge"
    if name == "band40":
        assert (c["nvc"], c["nfull"], c["nlow"]) == (38, 247, 703)
        assert c["s_memset"] and not c["dup_diag"] and (track == 1).any()
    elif name == "band40x":
        assert c["nvc"] == 38 and c["s_memset"] and not c["dup_diag"]
        assert track[track > 0].min() >= 2
    elif name == "band40dup":
        assert c["s_memset"] and c["dup_diag"] and c["ndup"] > 0
    elif name == "mixed70":
        assert c["nvc"] == 67 and (c["nfull"], c["nlow"]) == (2211, 2211)
        assert not c["s_memset"] and c["nempty"] == 0 and not c["dup_diag"]
        assert c["max_track"] > 64 and not c["chunks_ok"] and (track == 1).any()
    elif name == "mixed66":
        assert c["nfull"] == c["nlow"] == 2016 and not c["dup_diag"]
        assert c["max_track"] == 64 and c["chunks_ok"]
    elif name == "band201":
        assert c["nc"] > K_LIN_LDS_CAMS and c["nvc"] == 199 <= K_LIN_LDS_CAMS
        assert (c["nfull"], c["nlow"]) == (2112, 19701) and c["s_memset"]
        assert c["max_track"] <= 64 and c["chunks_ok"]
    elif name == "band230":
        assert c["nc"] > K_LIN_LDS_CAMS and c["nvc"] > K_LIN_LDS_CAMS
        assert (c["nfull"], c["nlow"]) == (22260, 25878)
        assert not c["s_memset"] and c["nempty"] > 0, "the empty blocks go through the eblocks list"
        assert c["max_track"] > 64 and not c["chunks_ok"]
    elif name == "ptfix40":
        fixed = p.pt_fixed != 0
        seen = track > 0
        assert (fixed & seen).any() and (~fixed & seen).any(), "fixed and variable points, both observed"
        assert not p.cam_fixed[20] and 20 not in p.obs_cam, "camera 20: variable, unobserved"
        vcs = c["cam_of_vc"]
        assert 20 not in vcs and (vcs < 20).any() and (vcs > 20).any(), "a hole inside cam_of_vc's range"
        assert c["nvc"] == 37
    else:
        raise AssertionError(f"no property listed for {name}")


@pytest.mark.parametrize("name", ["band40x", "band230"])
def test_band_scenes_have_uneven_pair_blocks(name):
    """Pair blocks of a single pair beside blocks of 50 x as many (the uniform
    problems hold about the mean everywhere; measured 1 .. 73 and 1 .. 200)."""
    p = scene(name)
    c = plan_conditions(p)
    vc = np.full(p.n_cams, -1)
    vc[c["cam_of_vc"]] = np.arange(c["nvc"])
    A = np.zeros((p.n_pts, c["nvc"]), np.int64)
    sel = vc[p.obs_cam] >= 0
    A[p.obs_pt[sel], vc[p.obs_cam[sel]]] = 1
    pairs = (A.T @ A)[np.tril_indices(c["nvc"], -1)]
    pairs = pairs[pairs > 0]
    assert pairs.min() == 1 and pairs.max() >= 50


@pytest.mark.parametrize("name", list(SCENES))
def test_shuffled_and_unshuffled_builds_are_one_problem(name):
    a, b = scene(name, shuffle=True), scene(name, shuffle=False)
    for f in ("cams", "K", "pts", "cam_fixed", "cam_fixed_extr"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert (a.pt_fixed is None) == (b.pt_fixed is None)
    if a.pt_fixed is not None:
        assert np.array_equal(a.pt_fixed, b.pt_fixed)

    def rows(p):
        r = np.column_stack([p.obs_pt.astype(np.float64), p.obs_cam, p.obs_uv[:, 0], p.obs_uv[:, 1]])
        return r[np.lexsort(r.T[::-1])]
    assert a.n_obs == b.n_obs and np.array_equal(rows(a), rows(b))
    assert not np.array_equal(a.obs_pt, b.obs_pt), "the shuffle changed the caller's order"


def min_rtol(a, b, atol=1e-10):
    """The smallest rtol at which assert_close(a, b, rtol, atol) would pass."""
    m = 0.0
    for x, y in zip(a, b):
        m = max(m, float(np.max((np.abs(x - y) - atol) / np.maximum(np.maximum(np.abs(x), np.abs(y)), 1e-300))))
    return max(m, 0.0)


@pytest.mark.parametrize("name", list(SCENES))
def test_oracle_sensitivity_to_observation_order(oracle_lib, name):
    """The oracle on the shuffled against the unshuffled build: the same
    accept / reject sequence, costs within 1e-11, the reduced system within
    1e-12 of its largest entry (measured: <= 6e-12, band201's PCG run, the
    rest <= 2e-13; and <= 7e-14), and the parameters after 6 iterations
    within 1e-9 at atol 1e-10 (measured <= 9e-11; a figure moves by up to 5 x
    between runs and thread counts, the oracle's OpenMP sums not being
    reproducible; the table in structured_problems.py).  The GPU parity tests
    compare parameters at rtol 1e-8: >= 100 x above every measured figure."""
    a, b = scene(name, shuffle=True), scene(name, shuffle=False)
    la, ra = oracle_lib.reduced_system(a, radius=1e4)
    lb, rb = oracle_lib.reduced_system(b, radius=1e4)
    s_sens = np.abs(la - lb).max() / np.abs(lb).max()
    r_sens = np.abs(ra - rb).max() / np.abs(rb).max()
    line = [f"{name:10s}"]
    figs = {}
    for kind, kw in ORACLE_KINDS.items():
        ca, pa, _, loga = oracle_lib.solve(a, oracle_lib.default_options(max_num_iterations=6, **kw))
        cb, pb, _, logb = oracle_lib.solve(b, oracle_lib.default_options(max_num_iterations=6, **kw))
        assert len(loga) == len(logb) == 7
        assert [r["step_is_successful"] for r in loga] == [r["step_is_successful"] for r in logb], kind
        assert [r["step_is_valid"] for r in loga] == [r["step_is_valid"] for r in logb], kind
        figs[kind] = (max(abs(x["cost"] - y["cost"]) / y["cost"] for x, y in zip(loga, logb)),
                      min_rtol((ca, pa), (cb, pb)))
        if name in ("band201", "band230") and kind == "dense":
            assert not all(r["step_is_successful"] for r in loga), "the scene is meant to reject a step"
    print(f"{name:10s} {figs['dense'][0]:8.1e} {figs['iter'][0]:8.1e} {s_sens:8.1e} "
          f"{figs['dense'][1]:9.1e} {figs['iter'][1]:9.1e}")
    for kind, (dcost, dpar) in figs.items():
        assert dcost <= 1e-11, (kind, dcost)
        assert dpar <= 1e-9, (kind, dpar)
    assert s_sens <= 1e-12 and r_sens <= 1e-12, (s_sens, r_sens)


def test_debug_plan_is_declared_and_refuses_null():
    """ba_debug_plan(ctx, out, n): bound with three parameters, one name per
    value of the header's BA_DEBUG_PLAN_FIELDS, and a NULL context or a NULL
    out is refused without a device."""
    sig = {name: (res, args) for name, res, args in N.SIGNATURES}["ba_debug_plan"]
    assert sig[0] is C.c_int and len(sig[1]) == 3
    import re
    from conftest import ROOT
    m = re.search(r"#define\s+BA_DEBUG_PLAN_FIELDS\s+(\d+)", (ROOT / "include" / "ba_hip.h").read_text())
    assert m and int(m.group(1)) == len(N.DEBUG_PLAN_FIELDS) == len(set(N.DEBUG_PLAN_FIELDS))
    lib = N.load_library()
    out = (C.c_int32 * len(N.DEBUG_PLAN_FIELDS))()
    assert lib.ba_debug_plan(None, out, len(out)) == 1   # BA_ERR_INVALID_ARGUMENT
    assert lib.ba_debug_plan(None, None, 0) == 1
