"""CPU tests for ba_triangulate: the numpy reference (tests/triangulate_ref.py)
is itself checked (ground truth on noise-free scenes, the two-view status
rules of SfMHelper::triangulatePoints, the Jacobi restatement against the SVD),
the ctypes mirrors of the new structs match the C layout, and the Problem ->
batch helper is correct.  No GPU."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import triangulate_ref as R
from bundleadjustment_amd import _native as N
from bundleadjustment_amd import make_synthetic, triangulation_batch
from bundleadjustment_amd.problem import K_colmajor, extr_colmajor
from conftest import ROOT


# ---------------------------------------------------------------------------
# DLT
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nc,k,seed", R.SCENES)
def test_reference_dlt_recovers_ground_truth_without_noise(nc, k, seed):
    p = R.all_fixed(make_synthetic(nc, 64, k, seed=seed, perturb=None, anchor=False, noise_px=0.0, outlier_frac=0.0))
    b = triangulation_batch(p)
    P = R.proj_matrices(b.extr, b.K)
    for q in range(64):
        cams, uv = R.views(b, q)
        if len(cams) < 2:
            continue
        A = R.dlt_rows(P, cams, uv)
        # float pixels and float extrinsics: ~1e-7 relative input error times the triangulation's conditioning
        assert np.allclose(R.dlt_svd(A), p.gt_pts[q], atol=1e-3)
        assert np.allclose(R.dlt_jacobi(A), p.gt_pts[q], atol=1e-3)


@pytest.mark.parametrize("nc,k,seed", R.SCENES)
def test_jacobi_restatement_is_within_the_perturbation_bound(nc, k, seed):
    """The kernel's Jacobi (pair order, stopping rule) restated in numpy stays
    within 256 beta of the SVD on every point of the GPU test's scenes."""
    b = R.scene(nc, k, seed)
    P = R.proj_matrices(b.extr, b.K)
    for q in range(len(b.pts)):
        cams, uv = R.views(b, q)
        assert len(cams) >= 2
        A = R.dlt_rows(P, cams, uv)
        beta = R.dlt_beta(A)
        assert beta <= 1e-9, (q, beta)
        assert R.dlt_error(R.dlt_jacobi(A), R.dlt_svd(A)) <= 256 * beta, q


def test_jacobi_eigenpairs_and_rank_rule():
    rng = np.random.default_rng(3)
    A = rng.normal(size=(9, 4))
    lam, V = R.jacobi4(A.T @ A)
    assert np.allclose(np.sort(lam), np.linalg.eigvalsh(A.T @ A), rtol=1e-13)
    assert np.allclose(V.T @ V, np.eye(4), atol=1e-14)
    # the same ray twice: rank 2, no point
    assert np.all(np.isnan(R.dlt_jacobi(np.vstack([A[:2], A[:2]]))))


# ---------------------------------------------------------------------------
# the status rules on hand-made two-view cases
# ---------------------------------------------------------------------------
def two_cams(c1=(1.0, 0.0, 0.0), flip1=False):
    """Camera 0 at the origin, camera 1 at centre c1, both looking along +z
    (flip1: camera 1 looks along -z)."""
    K = np.tile(K_colmajor(525.0, 525.0, 319.5, 239.5), (2, 1))
    R1 = np.diag([-1.0, 1.0, -1.0]) if flip1 else np.eye(3)
    c1 = np.asarray(c1, np.float64)
    extr = np.stack([extr_colmajor(np.eye(3), np.zeros(3)), extr_colmajor(R1, -R1 @ c1)])
    ctr = np.stack([np.zeros(3), c1]).astype(np.float32)
    return extr, ctr, K


def exact_uv(extr, K, X):
    P = R.proj_matrices(extr, K)
    q = np.einsum("cij,j->ci", P, np.append(np.asarray(X, np.float64), 1.0))
    return (q[:, :2] / q[:, 2:3]).astype(np.float32)


def status(X, extr, ctr, K, uv, scale=None, order=(0, 1), **kw):
    o = list(order)
    return R.point_status(np.asarray(X, np.float64), extr, ctr, K, np.array(o), uv[o],
                          None if scale is None else np.asarray(scale, np.float32)[o], **kw)


def test_status_ok_and_few_views():
    extr, ctr, K = two_cams()
    X = [0.5, 0.1, 4.0]
    uv = exact_uv(extr, K, X)
    assert status(X, extr, ctr, K, uv) == R.OK
    assert R.point_status(np.array(X), extr, ctr, K, np.array([0]), uv[:1], None) == R.FEW_VIEWS
    assert status(X, extr, ctr, K, uv, min_views=3) == R.FEW_VIEWS
    assert status([np.nan, 0, 0], extr, ctr, K, uv) == R.DEGENERATE
    assert status([1e39, 0, 0], extr, ctr, K, uv) == R.DEGENERATE      # not finite as a float
    assert status(X, extr, ctr, K, uv, failed=True) == R.DEGENERATE


def test_status_behind_both_or_behind_one():
    extr, ctr, K = two_cams()
    X = [0.5, 0.1, -4.0]
    uv = exact_uv(extr, K, X)   # (the reprojection is exact: only the cheirality test can reject)
    assert status(X, extr, ctr, K, uv) == R.BEHIND
    assert status(X, extr, ctr, K, uv, checks=R.CHECK_CHI2 | R.CHECK_SCALE) == R.OK
    # behind camera 1 only: the reference's `&&` accepts it, behind_rule 1 rejects it
    extr, ctr, K = two_cams(flip1=True)
    X = [0.5, 0.1, 4.0]
    uv = exact_uv(extr, K, X)
    assert status(X, extr, ctr, K, uv, behind_rule=0) == R.OK
    assert status(X, extr, ctr, K, uv, behind_rule=1) == R.BEHIND


def test_status_chi_is_a_norm_not_a_squared_norm():
    extr, ctr, K = two_cams()
    X = [0.5, 0.1, 4.0]
    uv = exact_uv(extr, K, X)
    off3, off7 = uv.copy(), uv.copy()
    off3[1, 0] += 3.0      # 3 px: 3 < 5.991 < 9
    off7[1, 0] += 7.0
    assert status(X, extr, ctr, K, off3) == R.OK
    assert status(X, extr, ctr, K, off7) == R.CHI2
    # invSigma = 1 / 1.2^octave: 7 px at octave 2 is 4.86
    assert status(X, extr, ctr, K, off7, scale=[1.0, 1.44], checks=R.CHECK_CHEIRALITY | R.CHECK_CHI2) == R.OK
    assert status(X, extr, ctr, K, off7, scale=[1.44, 1.0], checks=R.CHECK_CHEIRALITY | R.CHECK_CHI2) == R.CHI2


def test_status_scale_distance_zero_and_both_sides_of_the_ratio():
    extr, ctr, K = two_cams(c1=(0.0, 0.0, 2.0))
    uv = np.zeros((2, 2), np.float32)
    only = dict(checks=R.CHECK_SCALE)
    assert status([0, 0, 8.0], extr, ctr, K, uv, **only) == R.OK           # d0 / d1 = 8 / 6
    assert status([0, 0, 5.0], extr, ctr, K, uv, **only) == R.SCALE        # 5 / 3 > 1.5
    assert status([0, 0, 5.0], extr, ctr, K, uv, order=(1, 0), **only) == R.SCALE   # (3 / 5) 1.5 < 1
    assert status([0, 0, 2.0], extr, ctr, K, uv, **only) == R.SCALE        # at camera 1's centre: d1 == 0
    assert status([0, 0, 0.0], extr, ctr, K, uv, **only) == R.SCALE        # d0 == 0
    # octave scales: s1 / s0 = 2.0736 > (8 / 6) 1.5; and 5 / 3 <= 1.2 * 1.5
    assert status([0, 0, 8.0], extr, ctr, K, uv, scale=[1.0, 2.0736], **only) == R.SCALE
    assert status([0, 0, 5.0], extr, ctr, K, uv, scale=[1.0, 1.2], **only) == R.OK
    # the exact boundary is accepted on both sides (strict comparisons): 6 / 4 = 1.5
    assert status([0, 0, 6.0], extr, ctr, K, uv, **only) == R.OK


def test_status_order_is_behind_then_chi_then_scale():
    extr, ctr, K = two_cams(c1=(0.0, 0.0, 2.0))
    X = [0.3, 0.0, 5.0]
    uv = exact_uv(extr, K, X)
    assert status(X, extr, ctr, K, uv) == R.SCALE
    uv[0, 1] += 9.0
    assert status(X, extr, ctr, K, uv) == R.CHI2
    assert status([0.3, 0.0, -5.0], extr, ctr, K, uv) == R.BEHIND


def test_scenes_produce_every_status_class_on_the_cpu():
    b = R.scene(2, 2, 11)
    P = R.proj_matrices(b.extr, b.K)
    X = np.array([R.dlt_svd(R.dlt_rows(P, *R.views(b, q))) for q in range(len(b.pts))])
    cnt = np.bincount(R.batch_statuses(X, b), minlength=6)
    assert cnt[R.BEHIND] == 7 and cnt[R.CHI2] == 18, cnt
    r = R.ragged_scene()
    assert [int(r.obs_offset[q + 1] - r.obs_offset[q]) for q in range(len(r.pts))] == R.RAGGED_COUNTS + [6]
    st = R.batch_statuses(r.pts, r)
    assert list(st[:2]) == [R.FEW_VIEWS, R.FEW_VIEWS] and np.all(st[2:] != R.FEW_VIEWS)


# ---------------------------------------------------------------------------
# ABI and helper
# ---------------------------------------------------------------------------
LAYOUT_C = r"""
#include <stdio.h>
#include <stddef.h>
#include "ba_hip.h"
#define F(T, f) printf("%s.%s %zu\n", #T, #f, offsetof(T, f));
int main(void) {
  printf("ba_tri_batch %zu\nba_tri_options %zu\n", sizeof(ba_tri_batch), sizeof(ba_tri_options));
  F(ba_tri_batch, n_pts) F(ba_tri_batch, extr) F(ba_tri_batch, cam_center) F(ba_tri_batch, K)
  F(ba_tri_batch, obs_offset) F(ba_tri_batch, obs_cam) F(ba_tri_batch, obs_uv) F(ba_tri_batch, obs_scale)
  F(ba_tri_batch, pts_init) F(ba_tri_batch, huber_a)
  F(ba_tri_options, init) F(ba_tri_options, refine) F(ba_tri_options, min_views) F(ba_tri_options, checks)
  F(ba_tri_options, behind_rule) F(ba_tri_options, reserved)
  printf("enum %d %d %d %d %d %d %d %d\n", BA_TRI_OK, BA_TRI_FEW_VIEWS, BA_TRI_DEGENERATE, BA_TRI_BEHIND, BA_TRI_CHI2,
         BA_TRI_SCALE, BA_TRI_INIT_GIVEN, BA_TRI_CHECK_CHEIRALITY | BA_TRI_CHECK_CHI2 | BA_TRI_CHECK_SCALE);
  return 0;
}
"""


def test_ctypes_layout_of_the_new_structs_matches_c(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    types = {"ba_tri_batch": N.ba_tri_batch, "ba_tri_options": N.ba_tri_options}
    for line in lines:
        k, *v = line.split()
        if k == "enum":
            assert [int(x) for x in v] == [N.TRI_OK, N.TRI_FEW_VIEWS, N.TRI_DEGENERATE, N.TRI_BEHIND, N.TRI_CHI2,
                                           N.TRI_SCALE, N.TRI_INIT_GIVEN, N.TRI_CHECK_ALL]
            assert [R.OK, R.FEW_VIEWS, R.DEGENERATE, R.BEHIND, R.CHI2, R.SCALE] == [int(x) for x in v[:6]]
        elif "." in k:
            t, f = k.split(".")
            assert getattr(types[t], f).offset == int(v[0]), k
        else:
            assert C.sizeof(types[k]) == int(v[0]), k


def test_entry_points_and_defaults_without_a_device():
    lib = N.load_library()
    t = N.ba_tri_options()
    lib.ba_triangulate_defaults(C.byref(t))
    assert (t.init, t.refine, t.min_views, t.checks, t.behind_rule) == (N.TRI_INIT_DLT, 0, 2, N.TRI_CHECK_ALL, 0)
    assert lib.ba_triangulate(None, None, None, None, None, None, None) == 1   # BA_ERR_INVALID_ARGUMENT
    assert lib.ba_abi_version() == 2


def test_triangulation_batch_helper():
    p = make_synthetic(5, 40, 3, seed=21, perturb=None, anchor=False)
    with pytest.raises(ValueError, match="constant"):
        triangulation_batch(p)
    p = R.all_fixed(p)
    rng = np.random.default_rng(0)
    sh = rng.permutation(p.n_obs)            # caller order: not sorted by point
    p.obs_cam, p.obs_pt, p.obs_uv = p.obs_cam[sh], p.obs_pt[sh], p.obs_uv[sh]
    b = triangulation_batch(p)
    assert b.obs_offset[0] == 0 and b.obs_offset[-1] == p.n_obs and np.all(np.diff(b.obs_offset) >= 0)
    assert np.array_equal(np.sort(b.order), np.arange(p.n_obs))
    for q in range(p.n_pts):
        a0, a1 = b.obs_offset[q], b.obs_offset[q + 1]
        src = b.order[a0:a1]
        assert np.all(p.obs_pt[src] == q) and np.all(np.diff(src) > 0)     # the point's views, caller order kept
        assert np.array_equal(b.obs_cam[a0:a1], p.obs_cam[src]) and np.array_equal(b.obs_uv[a0:a1], p.obs_uv[src])
    assert np.array_equal(b.extr, p.cam_fixed_extr) and np.array_equal(b.pts, p.pts)
    # the centre maps to the camera's origin: E [c; 1] = 0
    E = b.extr.reshape(-1, 4, 4).transpose(0, 2, 1).astype(np.float64)
    z = np.einsum("cij,cj->ci", E[:, :3, :3], b.cam_center.astype(np.float64)) + E[:, :3, 3]
    assert np.max(np.abs(z)) < 1e-5
    # and the one-point problem the oracle solves carries exactly the point's views
    o = R.one_point_problem(b, 7, b.pts[7])
    assert o.n_pts == 1 and o.n_obs == b.obs_offset[8] - b.obs_offset[7] and np.all(o.cam_fixed == 1)
