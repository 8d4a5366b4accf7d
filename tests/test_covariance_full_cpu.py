"""CPU checks around ba_covariance_ex: the cross-block / leverage reference
(covariance_full_ref.py) against a dense inverse of the whole H, the trace
identity of the reference leverages, and the ctypes layout of the request."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import covariance_full_ref as F
import covariance_ref as R
from bundleadjustment_amd import _native as N
from conftest import ROOT


@pytest.mark.parametrize("name", ["n24", "n132"])
def test_reference_cross_blocks_match_dense_inverse(oracle_lib, name):
    p, full, _ = F.case_full(oracle_lib, name)
    cams, pts = np.arange(p.n_cams), np.arange(p.n_pts)
    cam_pt = [(c, q) for c in cams for q in pts]
    rng = np.random.default_rng(11)
    pt_pairs = ([(a, b) for a in pts for b in pts] if name == "n24"
                else [tuple(x) for x in rng.integers(0, p.n_pts, size=(2000, 2))] + [(q, q) for q in pts])
    worst = F.dense_check(full, cam_pt, pt_pairs)
    print(f"{name}: Schur-route cross blocks vs inv(H): {worst:.3e} (tolerance {full.tolerance():.3e})")
    assert worst <= full.tolerance()
    # constant cameras 0 and 1: zero blocks
    assert np.all(full.cam_pt(0, 3) == 0.0) and np.all(full.cam_pt(1, 5) == 0.0)
    # Cov(p, q)^T = Cov(q, p); p == q is the marginal of covariance_ref
    a, b = full.pt_pt(2, 9), full.pt_pt(9, 2)
    assert np.allclose(a, b.T, rtol=0, atol=1e-12 * np.abs(a).max())
    ref = R.reference(oracle_lib, p, [4])
    assert np.allclose(full.pt_pt(4, 4), ref.pt_cov[4], rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", ["n24", "n132", "n192"])
def test_reference_leverages_satisfy_the_trace_identity(oracle_lib, name):
    p, full, (h, g) = F.case_full(oracle_lib, name)
    trace = float(np.einsum("oii->", h))
    n_par = full.n_params()
    # per diagonal entry the first-order bound tol * g_r^2 of the GPU test
    bound = full.tolerance() * float((g * g).sum())
    print(f"{name}: sum tr(h) = {trace!r}, parameters {n_par}, |diff| {abs(trace - n_par):.3e} (bound {bound:.3e}), "
          f"max h {h.max():.4f}, max g_r g_s {np.einsum('or,os->ors', g, g).max():.3f}")
    assert abs(trace - n_par) <= bound
    assert np.allclose(h, h.transpose(0, 2, 1), rtol=0, atol=1e-14)
    gg = np.einsum("or,os->ors", g, g).max()
    assert gg <= 32.0
    # diagonal blocks of a projector: eigenvalues in [0, 1], up to the entry bound
    ev = np.linalg.eigvalsh(h)
    assert ev.min() >= -2.0 * full.tolerance() * gg and ev.max() <= 1.0 + 2.0 * full.tolerance() * gg


LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "ba_hip.h"
#define F(T, f) printf("%s.%s %zu\n", #T, #f, offsetof(T, f));
int main(void) {
  printf("ba_covariance_request_ex %zu\n", sizeof(ba_covariance_request_ex));
  F(ba_covariance_request_ex, base) F(ba_covariance_request_ex, n_cam_pt) F(ba_covariance_request_ex, n_pt_pairs)
  F(ba_covariance_request_ex, cam_pt) F(ba_covariance_request_ex, cam_pt_cov) F(ba_covariance_request_ex, pt_pairs)
  F(ba_covariance_request_ex, pt_pt_cov) F(ba_covariance_request_ex, n_lev) F(ba_covariance_request_ex, reserved)
  F(ba_covariance_request_ex, lev_obs) F(ba_covariance_request_ex, leverage)
  printf("BA_ABI_VERSION %d\n", BA_ABI_VERSION);
  return 0;
}
"""


def test_request_ex_layout_matches_c_compiler(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    vals = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                          check=True).stdout.splitlines())
    assert C.sizeof(N.ba_covariance_request_ex) == int(vals.pop("ba_covariance_request_ex"))
    assert int(vals.pop("BA_ABI_VERSION")) == N.BA_ABI_VERSION == 2
    assert len(vals) == len(N.ba_covariance_request_ex._fields_)
    for k, v in vals.items():
        assert getattr(N.ba_covariance_request_ex, k.split(".")[1]).offset == int(v), k


def test_covariance_ex_without_context_is_a_status():
    lib = N.load_library()
    assert lib.ba_covariance_ex(None, None) == 1
