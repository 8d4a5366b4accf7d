"""CPU checks around ba_covariance: the reference helper against a dense
inverse of the whole H, the conditioning of the shared test problems (so the
GPU tests' tolerance formula applies), and the ctypes layout of the request."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import covariance_ref as R
from bundleadjustment_amd import _native as N
from conftest import ROOT


@pytest.mark.parametrize("name", ["n24", "n132"])
def test_reference_schur_route_matches_dense_inverse(oracle_lib, name):
    p = R.make_case(name)
    ref = R.reference(oracle_lib, p)
    worst = R.dense_inverse_check(ref)
    print(f"{name}: Schur route vs inv(H): {worst:.3e} (tolerance {ref.tolerance():.3e})")
    assert worst <= ref.tolerance()
    # constant cameras 0 and 1: zero blocks; variable ones: symmetric, positive definite
    assert not ref.cam_var[0] and not ref.cam_var[1] and ref.cam_var[2:].all()
    assert np.all(ref.cam_cov[:2] == 0.0) and np.all(ref.cam_cov[:, :2] == 0.0)
    for c in range(2, p.n_cams):
        assert np.linalg.eigvalsh(ref.cam_cov[c, c]).min() > 0.0
    assert np.allclose(ref.cam_cov, ref.cam_cov.transpose(1, 0, 3, 2), rtol=0, atol=1e-9 * np.abs(ref.cam_cov).max())


@pytest.mark.parametrize("name", list(R.CASES))
def test_shared_problems_are_well_conditioned(oracle_lib, name):
    _, ref = R.case_reference(oracle_lib, name)
    print(f"{name}: n = {ref.n}, cond2(S) = {ref.cond_S:.3e}, tolerance {ref.tolerance():.3e}")
    assert ref.n == R.ORDER[name]
    assert ref.cond_S < 1e6


LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "ba_hip.h"
#define F(T, f) printf("%s.%s %zu\n", #T, #f, offsetof(T, f));
int main(void) {
  printf("ba_covariance_request %zu\n", sizeof(ba_covariance_request));
  F(ba_covariance_request, n_cam_pairs) F(ba_covariance_request, n_points) F(ba_covariance_request, cam_pairs)
  F(ba_covariance_request, cam_cov) F(ba_covariance_request, points) F(ba_covariance_request, pt_cov)
  printf("BA_ERR_SINGULAR %d\nBA_ABI_VERSION %d\n", (int)BA_ERR_SINGULAR, BA_ABI_VERSION);
  return 0;
}
"""


def test_request_layout_matches_c_compiler(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    vals = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                          check=True).stdout.splitlines())
    assert C.sizeof(N.ba_covariance_request) == int(vals.pop("ba_covariance_request"))
    assert int(vals.pop("BA_ERR_SINGULAR")) == 6 and N.STATUS_NAMES[6] == "BA_ERR_SINGULAR"
    assert int(vals.pop("BA_ABI_VERSION")) == N.BA_ABI_VERSION == 2
    for k, v in vals.items():
        assert getattr(N.ba_covariance_request, k.split(".")[1]).offset == int(v), k


def test_covariance_without_problem_or_context_is_a_status():
    lib = N.load_library()
    assert lib.ba_covariance(None, None) == 1
    assert lib.ba_covariance_times(None, None, 0) < 0
