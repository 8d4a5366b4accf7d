"""CPU tests for the five-point essential solver of ba_two_view_ransac
(BA_TV_E_FIVE_POINT): the numpy reference (tests/two_view_e5_ref.py) is itself
checked, the ctypes mirrors of the touched structs match the C layout, and the
device's solver text (tv_solve_e5, csrc/ba_two_view.h) runs as a stand-alone
host program under ASan + UBSan and meets the yardstick of the GPU tests.
No GPU.

Host program, worst over the eight yardstick cases (1000 hypotheses each):
sample residual 4.7e-16, constraint residual 1.2e-15 (reference 1.4e-5),
constraint / bound 1.1e-3, nearest / bound 3.7e-4, no count mismatch, no
borderline hypothesis; 4.5 .. 5.1 solutions per sample."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import two_view_e5_ref as F
import two_view_ref as R
from bundleadjustment_amd import _native as N
from conftest import ROOT
from test_two_view_cpu import HEADER, MARGIN, REF_DIR_RAD, REF_ROT_RAD, THR2

REF_E_RESIDUAL = 1e-14      # a null-space member leaves |b2^T E b1| at a few eps (see test_two_view_cpu.py)


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("n", F.SOLVER_NS)
def test_reference_solutions_fit_their_samples(n, planar):
    ref = F.solver_reference(n, planar)
    worst = float(ref["res"].max())
    print(f"reference n={n} planar={planar}: worst sample residual {worst:.3g}, solutions per sample "
          f"{ref['n_sol'].mean():.2f} ({ref['n_sol'].min()} .. {ref['n_sol'].max()}), borderline {int(ref['border'].sum())}, "
          f"worst constraint residual {float(ref['con_worst'].max()):.3g}")
    assert 0.0 < worst <= REF_E_RESIDUAL
    assert ref["border"].sum() <= F.MAX_BORDER * F.SOLVER_H
    assert ref["n_sol"].min() >= 0 and ref["n_sol"].max() <= 10
    if not planar:
        assert np.median(ref["near_dist"]) < 1e-4                     # the typical sample holds the truth among its solutions


@pytest.mark.parametrize("n,frac", R.E2E_CASES)
def test_reference_recovers_the_truth_on_noise_free_scenes(n, frac):
    sc = R.e2e_scene(n, frac, False)
    E, votes, kept = F.ransac(sc, R.E2E_H)
    Rm, t, _, mask, good, second = R.pose_from(R.ESSENTIAL, E, sc.uv1, sc.uv2, THR2)
    errs = R.truth_errors(sc, Rm, t, None)
    print(f"five-point reference n={n} outliers={frac}: votes {votes}, kept {kept}, errors (rad) {errs}, good {good}/{second}")
    assert votes == int(sc.inlier.sum()) and np.array_equal(mask, sc.inlier)
    assert errs[0] <= REF_ROT_RAD and errs[1] <= REF_DIR_RAD


def test_reference_projection_keeps_the_votes_on_the_noisy_scene():
    sc = R.e2e_scene(200, 0.3, False, 0.3)
    _, votes, kept = F.ransac(sc, R.E2E_H)
    print(f"five-point reference, noisy 200: votes {votes}, kept by the projection {kept} (generator inliers {int(sc.inlier.sum())})")
    assert kept >= 0.9 * votes and votes >= 0.9 * int(sc.inlier.sum())


# ---------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------
STRUCTS = {"ba_two_view_options": N.ba_two_view_options, "ba_two_view_result": N.ba_two_view_result}


def test_ctypes_layout_of_the_touched_structs_matches_c(tmp_path):
    body = "".join(f'  printf("{t} %zu\\n", sizeof({t}));\n' +
                   "".join(f'  printf("{t}.{f} %zu\\n", offsetof({t}, {f}));\n' for f, _ in cls._fields_)
                   for t, cls in STRUCTS.items())
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ba_hip.h"\nint main(void) {\n' + body +
                   '  printf("enum %d %d\\n", BA_TV_E_EIGHT_POINT, BA_TV_E_FIVE_POINT);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == 2 + sum(len(c._fields_) for c in STRUCTS.values()) + 1
    for line in lines:
        k, *v = line.split()
        if k == "enum":
            assert [int(x) for x in v] == [N.TV_E_EIGHT_POINT, N.TV_E_FIVE_POINT] == [0, F.FIVE_POINT]
        elif "." in k:
            t, f = k.split(".")
            assert getattr(STRUCTS[t], f).offset == int(v[0]), k
        else:
            assert C.sizeof(STRUCTS[k]) == int(v[0]), k
    assert "reserved" in dict(N.ba_two_view_options._fields_) and "reserved" in dict(N.ba_two_view_result._fields_)


def test_header_names_the_new_symbols():
    txt = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    fns = set(re.findall(r"\b(ba_[a-z0-9_]+)\s*\(", txt))
    assert "ba_two_view_hypotheses_e5" in fns
    assert re.search(r"enum\s+ba_tv_e_solver\s*\{\s*BA_TV_E_EIGHT_POINT\s*=\s*0\s*,\s*BA_TV_E_FIVE_POINT\s*=\s*1\s*\}", txt)
    assert re.search(r"#define\s+BA_ABI_VERSION\s+2\b", txt)
    assert "ba_two_view_hypotheses_e5" in {name for name, _, _ in N.SIGNATURES_DIGIT}
    assert len(dict((n, a) for n, _, a in N.SIGNATURES_DIGIT)["ba_two_view_hypotheses_e5"]) == 10


def test_entry_point_and_defaults_without_a_device():
    lib = N.load_library()
    p = N.ba_two_view_options()
    p.reserved = 7
    lib.ba_two_view_defaults(C.byref(p))
    assert p.reserved == 0 == N.TV_E_EIGHT_POINT
    assert lib.ba_two_view_hypotheses_e5(None, None, None, 0, 0, 0, None, None, None, None) == 1   # BA_ERR_INVALID_ARGUMENT
    assert lib.ba_abi_version() == 2


# ---------------------------------------------------------------------------
# the device's text as a host program under ASan + UBSan
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e5_host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("two_view_e5_host") / "two_view_e5_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "cpp" / "two_view_e5_host.cpp"), "-o", str(exe)], check=True)

    def run(sc, smp):
        """(n_sol (H,), E (H, 10, 3, 3)) of the samples smp (H, 8) of scene sc"""
        fl = lambda xs: " ".join(repr(float(x)) for x in xs)   # noqa: E731
        cases = exe.parent / "cases.txt"
        cases.write_text("".join("solve5 " + fl(sc.K) + "\n" + "".join(fl((*sc.uv1[i], *sc.uv2[i])) + "\n" for i in s[:5])
                                 for s in smp))
        out = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == 11 * len(smp)
        n_sol = np.array([int(out[11 * h]) for h in range(len(smp))])
        E = np.array([[out[11 * h + 1 + s].split() for s in range(10)] for h in range(len(smp))], np.float64)
        return n_sol, E.reshape(len(smp), 10, 3, 3)
    return run


def test_the_eight_point_host_program_still_compiles_with_the_new_text(tmp_path):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsyntax-only",
                    str(ROOT / "tests" / "cpp" / "two_view_host.cpp")], check=True)


@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("n", F.SOLVER_NS)
def test_host_program_solver_within_the_yardstick(e5_host, n, planar):
    ref = F.solver_reference(n, planar)
    n_sol, E = e5_host(R.solver_scene(n, planar), ref["smp"])
    F.check_yardstick(n, planar, n_sol, E, MARGIN)
    # ordered by the root of the hidden variable: no two solutions of a hypothesis coincide
    for h in np.flatnonzero(n_sol > 1)[:200]:
        S = E[h, :n_sol[h]].reshape(-1, 9)
        d = np.minimum(np.linalg.norm(S[:, None] - S[None], axis=2), np.linalg.norm(S[:, None] + S[None], axis=2))
        assert np.all(d[~np.eye(len(S), dtype=bool)] > 0.0)


def test_host_program_on_degenerate_samples(e5_host):
    """Rank-deficient and repeated samples end without a fault and with valid output: unit matrices in the null
    space, zeros past n_sol."""
    sc = R.solver_scene(9, False)
    smp = np.array([[0, 0, 0, 0, 0, 1, 2, 3], [0, 1, 0, 1, 0, 2, 3, 4], [3, 3, 3, 3, 4, 0, 1, 2]], np.int32)
    n_sol, E = e5_host(sc, smp)
    b1, b2 = F.sample_bearings(sc, smp)
    for h in range(len(smp)):
        assert 0 <= n_sol[h] <= 10 and np.all(E[h, n_sol[h]:] == 0.0)
        if n_sol[h]:
            assert np.all(np.abs(np.linalg.norm(E[h, :n_sol[h]], axis=(1, 2)) - 1.0) <= 1e-14)
            assert F.sample_residual(E[h:h + 1, :n_sol[h]], b1[h:h + 1], b2[h:h + 1]).max() <= MARGIN * 1e-14
