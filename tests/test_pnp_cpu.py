"""CPU tests for ba_pnp_ransac: the numpy reference (tests/pnp_ref.py) is itself
checked (the pinned sampler's properties, the independent P3P on noise-free
scenes), the ctypes mirrors of the new structs match the C layout, the header
names the entry points, and the device's sampler and solver (csrc/ba_p3p.h)
run as a stand-alone host program under ASan + UBSan.  No GPU."""
import ctypes as C
import itertools
import re
import subprocess

import numpy as np
import pytest

import pnp_ref as R
from bundleadjustment_amd import _native as N
from bundleadjustment_amd.problem import rotation_to_angle_axis
from conftest import ROOT

HEADER = ROOT / "include" / "ba_hip.h"
# The reference must find the truth to fp64 rounding times the conditioning of
# the minimal problem: image triangles down to ~2 px^2 at 525 px focal length
# amplify the 1.1e-16 of the bearings by up to ~1e6, so 1e-9 on R and t, and
# 1e-8 px once multiplied by the focal length.
REF_DIST_BOUND, REF_REPROJ_BOUND = 1e-9, 1e-8
MARGIN = 16.0          # a different root-finder at the same conditioning


# ---------------------------------------------------------------------------
# sampler
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 4, 7, 64, 65])
def test_sampler_draws_three_distinct_indices_in_range(n):
    for seed in (0, 99, (1 << 64) - 1):
        t = R.samples(seed, n, 2000, False)
        assert t.min() >= 0 and t.max() < n
        assert np.all(t[:, 0] != t[:, 1]) and np.all(t[:, 0] != t[:, 2]) and np.all(t[:, 1] != t[:, 2])
    assert np.array_equal(R.samples(5, n, 40, False)[7:], R.samples(5, n, 40, False, h0=7))
    assert np.array_equal(R.samples(5, n, 3, True)[0], [-1, -1, -1])
    assert np.array_equal(R.samples(5, n, 3, True)[1:], R.samples(5, n, 3, False)[1:])


def test_sampler_is_uniform_over_triples():
    """20000 draws over the 35 triples of n = 7: 571 expected each, sigma 23.6;
    every count within 5 sigma.  Every ordered triple of n = 4 occurs."""
    t = R.samples(0, 7, 20000, False)
    cnt = {c: 0 for c in itertools.combinations(range(7), 3)}
    for row in np.sort(t, axis=1):
        cnt[tuple(int(x) for x in row)] += 1
    assert min(cnt.values()) >= 453 and max(cnt.values()) <= 690, (min(cnt.values()), max(cnt.values()))
    seen = {tuple(int(x) for x in row) for row in R.samples(0, 4, 2000, False)}
    assert seen == set(itertools.permutations(range(4), 3))
    assert {tuple(int(x) for x in row) for row in R.samples(0, 3, 200, False)} == set(itertools.permutations(range(3)))


def test_sampler_pinned_values():
    """The rule by hand for one draw: any implementation gives these triples."""
    z = (0 + 1 * 0x9E3779B97F4A7C15) & R.M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & R.M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & R.M64
    z ^= z >> 31
    assert R.draw(0, 0, 0, 1000) == ((z >> 32) * 1000) >> 32
    assert R.mix(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF      # splitmix64's first output for seed 0


# ---------------------------------------------------------------------------
# the reference solver
# ---------------------------------------------------------------------------
def test_reference_solver_finds_the_truth_in_every_sample():
    """Noise-free scenes n in {7, 64, 65, 257}, 1000 samples each, seed 99: the
    true pose is among the solutions of EVERY sample.  The two worst values are
    the yardstick of the device tests (pnp_ref.yardstick)."""
    wd, wr = R.yardstick()
    print(f"reference: worst distance to the truth {wd:.3g}, worst sample reprojection {wr:.3g} px")
    assert wd <= REF_DIST_BOUND and wr <= REF_REPROJ_BOUND
    assert wd > 0.0 and wr > 0.0


def test_scene_generator():
    sc = R.scene(65, 0.6, 0.5, 3)
    assert sc.pts.shape == (65, 3) and sc.uv.dtype == np.float32 and int((~sc.inlier).sum()) == 39
    e, z = R.reproj_err(sc.R, sc.t, sc.K, sc.pts, sc.uv)
    assert np.all(z >= 1.0 - 1e-9) and np.all(e[sc.inlier] < 4.0) and np.all(e[~sc.inlier] > 45.0)
    sc0 = R.solver_scene(64)
    e0, _ = R.reproj_err(sc0.R, sc0.t, sc0.K, sc0.pts, sc0.uv)
    assert np.max(e0) < 1e-9                                   # exact in fp64: built from the float pixels
    assert np.array_equal(R.inliers_cam(sc.cam, sc.K, sc.pts, sc.uv, 8.0), sc.inlier)


# ---------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------
LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "ba_hip.h"
#define F(T, f) printf("%s.%s %zu\n", #T, #f, offsetof(T, f));
int main(void) {
  printf("ba_pnp_options %zu\nba_pnp_result %zu\n", sizeof(ba_pnp_options), sizeof(ba_pnp_result));
  F(ba_pnp_options, max_hypotheses) F(ba_pnp_options, min_points) F(ba_pnp_options, min_inliers)
  F(ba_pnp_options, use_prior) F(ba_pnp_options, refine) F(ba_pnp_options, reserved) F(ba_pnp_options, seed)
  F(ba_pnp_options, threshold_px)
  F(ba_pnp_result, status) F(ba_pnp_result, n_inliers) F(ba_pnp_result, n_inliers_ransac)
  F(ba_pnp_result, best_hypothesis) F(ba_pnp_result, cam_ransac) F(ba_pnp_result, refine)
  printf("enum %d %d %d %d\n", BA_PNP_OK, BA_PNP_FEW_POINTS, BA_PNP_NO_MODEL, BA_PNP_REFINE_FAILED);
  return 0;
}
"""


def test_ctypes_layout_of_the_new_structs_matches_c(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    types = {"ba_pnp_options": N.ba_pnp_options, "ba_pnp_result": N.ba_pnp_result}
    assert len(lines) == 17
    for line in lines:
        k, *v = line.split()
        if k == "enum":
            assert [int(x) for x in v] == [N.PNP_OK, N.PNP_FEW_POINTS, N.PNP_NO_MODEL, N.PNP_REFINE_FAILED]
            assert [int(x) for x in v] == [R.OK, R.FEW_POINTS, R.NO_MODEL, R.REFINE_FAILED]
        elif "." in k:
            t, f = k.split(".")
            assert getattr(types[t], f).offset == int(v[0]), k
        else:
            assert C.sizeof(types[k]) == int(v[0]), k


def test_header_names_the_new_symbols():
    txt = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    fns = set(re.findall(r"\b(ba_[a-z0-9_]+)\s*\(", txt))
    assert {"ba_pnp_defaults", "ba_pnp_ransac", "ba_pnp_times", "ba_pnp_hypotheses"} <= fns
    for name in ("ba_pnp_options", "ba_pnp_result", "BA_PNP_OK", "BA_PNP_FEW_POINTS", "BA_PNP_NO_MODEL",
                 "BA_PNP_REFINE_FAILED"):
        assert re.search(r"\b%s\b" % name, txt), name
    assert re.search(r"#define\s+BA_ABI_VERSION\s+2\b", txt)


def test_entry_points_and_defaults_without_a_device():
    lib = N.load_library()
    p = N.ba_pnp_options()
    lib.ba_pnp_defaults(C.byref(p))
    assert (p.max_hypotheses, p.min_points, p.min_inliers, p.use_prior, p.refine, p.reserved, p.seed,
            p.threshold_px) == (1000, 7, 6, 1, 1, 0, 0, 8.0)
    lib.ba_pnp_defaults(None)
    assert lib.ba_pnp_ransac(None, None, None, None, None, None, None) == 1   # BA_ERR_INVALID_ARGUMENT
    assert lib.ba_pnp_hypotheses(None, None, None, 0, 0, 0, None, None, None, None) == 1
    assert lib.ba_pnp_times(None, None, 0) == -1
    assert lib.ba_abi_version() == 2


# ---------------------------------------------------------------------------
# the device's sampler and solver as a host program under ASan + UBSan
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pnp_host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pnp_host") / "pnp_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "cpp" / "pnp_host.cpp"), "-o", str(exe)], check=True)

    def run(text: str) -> list[str]:
        cases = exe.parent / "cases.txt"
        cases.write_text(text)
        return subprocess.run([str(exe), str(cases)], capture_output=True, text=True, check=True).stdout.splitlines()
    return run


def test_host_program_sampler_equals_the_reference(pnp_host):
    cases = [(seed, n, h0, 130) for seed in (0, 99, (1 << 64) - 1) for n in (3, 4, 7, 64, 65) for h0 in (0, 63, 64)]
    out = pnp_host("".join(f"sample {s} {n} {h0} {c}\n" for s, n, h0, c in cases))
    got = np.array([[int(x) for x in line.split()] for line in out], np.int32)
    want = np.concatenate([R.samples(s, n, h0 + c, False, h0=h0) for s, n, h0, c in cases])
    assert np.array_equal(got, want)


def test_host_program_solver_finds_the_truth_within_the_yardstick(pnp_host):
    """The GPU test's solver cases through the same header text on the host:
    the truth is among the solutions of every sample within 16 x the
    reference's own worst error, every solution reprojects its sample within
    16 x the reference's worst, R is a rotation."""
    wd_ref, wr_ref = R.yardstick()
    lines, cases = [], []
    for n in R.SOLVER_NS:
        sc = R.solver_scene(n)
        for h in range(R.SOLVER_H):
            tri = R.sample(0, h, n)
            cases.append((sc, tri))
            lines.append("p3p " + " ".join(repr(float(k)) for k in sc.K))
            lines += [" ".join(repr(float(x)) for x in (*sc.pts[i], *sc.uv[i])) for i in tri]
    out = pnp_host("\n".join(lines) + "\n")
    pos, wd, wr = 0, 0.0, 0.0
    for sc, tri in cases:
        ns = int(out[pos])
        rows = np.array([out[pos + 1 + k].split() for k in range(ns)], np.float64).reshape(ns, 12)
        pos += 1 + ns
        assert 1 <= ns <= 4, tri
        sols = [(r[:9].reshape(3, 3), r[9:]) for r in rows]
        for Rm, _ in sols:
            assert np.max(np.abs(Rm @ Rm.T - np.eye(3))) <= 1e-12 and abs(np.linalg.det(Rm) - 1.0) <= 1e-12
        d, rp = R.truth_and_reproj(sols, sc, tri)
        wd, wr = max(wd, d), max(wr, rp)
    assert pos == len(out)
    print(f"host program: worst distance {wd:.3g} (reference {wd_ref:.3g}), worst reprojection {wr:.3g} px "
          f"(reference {wr_ref:.3g})")
    assert wd <= MARGIN * wd_ref and wr <= MARGIN * wr_ref


def test_host_program_angle_axis_is_the_ceres_conversion(pnp_host):
    rng = np.random.default_rng(5)
    ws = np.concatenate([rng.normal(size=(20, 3)), 3.1 * rng.normal(size=(20, 3)) / np.sqrt(3.0),
                         [[0.0, 0.0, 0.0], [np.pi, 0.0, 0.0], [0.0, -3.0, 0.5], [1e-9, 0.0, 0.0]]])
    from bundleadjustment_amd.problem import angle_axis_to_rotation
    Rs = angle_axis_to_rotation(ws)
    assert sum(np.trace(M) < 0.0 for M in Rs) >= 5            # the Shepperd branches are exercised
    out = pnp_host("".join("aa " + " ".join(repr(float(x)) for x in M.reshape(-1)) + "\n" for M in Rs))
    got = np.array([line.split() for line in out], np.float64)
    want = rotation_to_angle_axis(Rs)
    # the same operations in the same order; libm's atan2 / sqrt may differ from Python's by an ulp
    assert np.max(np.abs(got - want)) <= 1e-14
