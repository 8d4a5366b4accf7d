"""CPU tests for ba_icp: the host checker, the grid plan and the grid search of
the kernels (host/ba_batch_pack.hpp, csrc/ba_icp.h) run as a stand-alone host
program under ASan + UBSan and equal the brute-force numpy restatement
(tests/icp_ref.py) in index and in d2 bits; the restatement itself on the clean
scene and on the reference's two gtest cases; the sensitivity that sets the
noisy-scene tolerance of tests/test_icp.py; defaults, argument errors, the
ctypes mirrors, the PLY reader and writer and the normalisation are checked
without a device.  No GPU."""
import ctypes as C
import json
import struct
import subprocess

import numpy as np
import pytest

import icp_ref as R
from bundleadjustment_amd import _native as N
from bundleadjustment_amd import reconstruction
from bundleadjustment_amd.io import read_ply_vertices, write_ply_vertices
from bundleadjustment_amd.problem import ICP_RESULT_DTYPE, pack_icp_batch
from conftest import GOLDEN, ROOT

GRID, BRUTE = N.ICP_ROUTE_GRID, N.ICP_ROUTE_BRUTE
HUGE_CELL, TINY_CELL = 1.0e6, 0.125          # one cell; at most one distinct lattice point per cell


def bits(a) -> str:
    return " ".join(f"{v:08x}" for v in np.asarray(a, np.float32).reshape(-1).view(np.uint32).tolist())


def case(sets, pairs, guess=None, max_ring=6, max_iterations=10, route=GRID, min_correspondences=3, with_scale=0,
         reserved=0, max_corr_dist=np.inf, cell=0.0, set_offset=None, n_points=None):
    sets = [np.asarray(s, np.float32).reshape(-1, 3) for s in sets]
    off = np.cumsum([0] + [s.shape[0] for s in sets]) if set_offset is None else np.asarray(set_offset)
    xyz = np.concatenate(sets) if sets else np.zeros((0, 3), np.float32)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    lines = [f"{len(off) - 1} {pairs.shape[0]} {xyz.shape[0] if n_points is None else n_points} {int(guess is not None)} {max_ring}",
             f"{max_iterations} {route} {min_correspondences} {with_scale} {reserved} {bits([max_corr_dist])} {bits([cell])}",
             " ".join(str(int(v)) for v in off), " ".join(f"{a} {b}" for a, b in pairs.tolist()), bits(xyz)]
    if guess is not None:
        lines.append(bits(guess))
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("icp_host") / "icp_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-omit-frame-pointer", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "cpp" / "icp_host.cpp"), "-o", str(exe)], check=True)

    def run(text: str) -> list[str]:
        path = exe.parent / "case.txt"
        path.write_text(text)
        return subprocess.run([str(exe), str(path)], capture_output=True, text=True, check=True).stdout.splitlines()
    return run


def parse(out):
    """grids [(n0, n1, n2, h, cells, most)], pairs [dict(ns, nt, route, swept, idx, d2, perm, step)]"""
    u32 = lambda words: np.array([int(w, 16) for w in words], np.uint32).view(np.float32)
    grids, pairs, pos = [], [], 0
    while pos < len(out) and out[pos].startswith("grid "):
        w = out[pos].split()
        grids.append((int(w[1]), int(w[2]), int(w[3]), float(u32([w[4]])[0]), int(w[5]), int(w[6])))
        pos += 1
    while pos < len(out):
        w = out[pos].split()
        assert w[0] == "pair"
        step = out[pos + 4].split()
        assert out[pos + 3].split()[0] == "perm" and step[0] == "step"
        pairs.append(dict(ns=int(w[2]), nt=int(w[3]), route=int(w[4]), swept=int(w[5]),
                          idx=np.array(out[pos + 1].split(), np.int32), d2=u32(out[pos + 2].split()),
                          perm=np.array(out[pos + 3].split()[1:], np.int32),
                          state=int(step[1]), iterations=int(step[2]), n_corr=int(step[3]),
                          M=u32(step[4:13]).reshape(3, 3), t=u32(step[13:16])))
        pos += 5
    return grids, pairs


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


# ---------------------------------------------------------------------------
# the scenes and the restatement itself
# ---------------------------------------------------------------------------
def test_coarse_scene_holds_every_case():
    sc = R.coarse_scene(257, 1000)
    D = R.d2_matrix(sc.src, sc.tgt)
    assert len({tuple(p) for p in sc.tgt.tolist()}) < 1000                       # duplicated targets
    assert D[0, 0].view(np.uint32) == D[0, 1].view(np.uint32) and not np.array_equal(sc.tgt[0], sc.tgt[1])
    ties = (D == D.min(axis=1, keepdims=True)).sum(axis=1)
    assert (ties > 1).sum() > 50                                                 # bitwise-equal best d2
    lo, hi = sc.tgt.min(axis=0), sc.tgt.max(axis=0)
    assert (np.any((sc.src < lo - 50) | (sc.src > hi + 50), axis=1)).sum() >= 40  # far outside the box
    assert np.ptp(R.coarse_scene(9, 65, "coplanar").tgt[:, 2]) == 0
    col = R.coarse_scene(9, 65, "collinear").tgt
    assert np.ptp(col[:, 1]) == 0 and np.ptp(col[:, 2]) == 0 and np.ptp(col[:, 0]) > 0
    assert R.coarse_scene(9, 1).tgt.shape == (1, 3)
    idx, d2 = R.nn_brute(sc.src, sc.tgt)
    assert idx[0] == 0 or D[0, idx[0]] < D[0, 0]                                 # the tie goes to the lower index


def test_clean_scene_under_the_restatement():
    sc = R.clean_scene()
    assert sc.src.shape == (300, 3)
    r = R.icp(sc.src, sc.tgt)
    gap = R.second_gap(r.cur, sc.tgt)
    print(f"clean scene: state {r.state}, iterations {r.iterations}, fitness {r.fitness:.3g}, "
          f"transform error {np.abs(r.final.astype(np.float64) - sc.truth).max():.3g}, smallest best-to-second gap {gap:.3g}")
    assert r.state == R.ABS_MSE and r.converged == 1
    assert r.fitness < 1e-12
    assert np.abs(r.final.astype(np.float64) - sc.truth).max() < 1e-6
    assert gap > 1e-6          # far above the float error of a d2 of this size: the correspondences cannot flip


def test_reference_gtest_cases():
    """ReconstructionError_test.cc: CompareIdenticalClouds and CompareSimilarClouds (three-point clouds)."""
    g = json.loads((GOLDEN / "icp_three_points.json").read_text())
    c1, c2 = np.array(g["cloud1"], np.float32), np.array(g["cloud2"], np.float32)
    same = R.icp(c1, c1)
    assert same.converged and same.fitness <= 1e-5
    near = R.icp(c1, c2)
    assert near.converged and 0.0 <= near.fitness < 0.1


def test_noisy_scene_sensitivity():
    """What one ulp of every step's float R, t does to the result: the spread
    that sets the tolerance of test_icp.py's noisy-scene test."""
    sc = R.noisy_scene()
    assert sc.src.shape == (700, 3) and sc.tgt.shape == (1900, 3)
    a, b = R.icp(sc.src, sc.tgt), R.icp(sc.src, sc.tgt, perturb=True)
    print(f"noisy scene: fitness {a.fitness:.9g} / {b.fitness:.9g}, spread {abs(a.fitness - b.fitness):.3g}; "
          f"final spread {np.abs(a.final - b.final).max():.3g}")
    assert a.state == b.state == R.ITERATIONS and a.iterations == 10
    assert abs(a.fitness - b.fitness) < 1e-3 * a.fitness and np.abs(a.final - b.final).max() < 1e-3


# ---------------------------------------------------------------------------
# the host program
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.COARSE_KINDS)
@pytest.mark.parametrize("n_tgt", [1, 2, 64, 65, 1000])
def test_host_grid_search_equals_brute_force(host, kind, n_tgt):
    sc = R.coarse_scene(257, n_tgt, kind)
    idx, d2 = R.nn_brute(sc.src, sc.tgt)
    for cell, ring in ((HUGE_CELL, 6), (0.0, 6), (TINY_CELL, 6), (0.0, 1 << 20), (TINY_CELL, 1 << 20), (0.0, 0)):
        grids, pairs = parse(host(case([sc.src, sc.tgt], [[0, 1]], cell=cell, max_ring=ring)))
        (n0, n1, n2, h, cells, most), p = grids[0], pairs[0]
        assert cells == n0 * n1 * n2 and (p["ns"], p["nt"], p["route"]) == (257, n_tgt, GRID)
        if cell == HUGE_CELL:
            assert cells == 1 and most == n_tgt
        if cell == TINY_CELL:
            assert h == TINY_CELL and most <= 1 + n_tgt // 4 + 1     # a cell holds one lattice point and its repeats
        if ring == 1 << 20:
            assert p["swept"] == 0                                   # the walk alone decides every query
        assert np.array_equal(p["idx"], idx), (kind, n_tgt, cell, ring)
        assert same_bits(p["d2"], d2), (kind, n_tgt, cell, ring)
        assert sorted(p["perm"].tolist()) == list(range(257))


def test_host_planned_cell_size_aims_at_eight_points(host):
    sc = R.noisy_scene()
    rng = np.random.default_rng(0)
    cube = rng.random((4000, 3)).astype(np.float32)
    grids, pairs = parse(host(case([sc.src, sc.tgt, cube], [[0, 1], [0, 2]])))
    assert 4000 / 16 <= grids[1][4] <= 4000 / 4                      # a filled box: about 8 points per cell
    assert grids[0][4] >= 1900 / 16                                  # a surface leaves most cells of its box empty
    for p, tgt in zip(pairs, (sc.tgt, cube)):
        idx, d2 = R.nn_brute(sc.src, tgt)
        assert np.array_equal(p["idx"], idx) and same_bits(p["d2"], d2)


def test_host_gate_brute_route_guess_and_step(host):
    sc = R.noisy_scene(257, 1000)
    guess = R.rigid(1.0, (0, 0, 1), (0.01, 0, 0)).astype(np.float32)
    cur = R.apply(guess[:3, :3], guess[:3, 3], sc.src)
    for route in (GRID, BRUTE):
        for dist in (np.inf, 0.05, 0.004):
            _, pairs = parse(host(case([sc.src, sc.tgt], [[0, 1]], guess=[guess], route=route, max_corr_dist=dist)))
            p = pairs[0]
            idx, d2 = R.nn_brute(cur, sc.tgt, np.float32(dist) * np.float32(dist))
            assert np.array_equal(p["idx"], idx) and same_bits(p["d2"], d2)
            n = int((idx >= 0).sum())
            assert p["n_corr"] == n and (0 < n < 257 or dist != 0.05)
            if n >= 3:
                M, t = R.estimate(cur, sc.tgt, idx)
                assert p["state"] == R.NOT_CONVERGED and p["iterations"] == 1
                assert np.abs(p["M"] - M).max() < 1e-6 and np.abs(p["t"] - t).max() < 1e-6
            else:
                assert p["state"] == R.NO_CORRESPONDENCES and p["iterations"] == 0


def test_host_step_with_scale_and_reflection_guard(host):
    sc = R.clean_scene(scale=1.25)
    _, pairs = parse(host(case([sc.src, sc.tgt], [[0, 1]], with_scale=1)))
    idx, _ = R.nn_brute(sc.src, sc.tgt)
    M, t = R.estimate(sc.src, sc.tgt, idx, with_scale=1)
    assert np.abs(pairs[0]["M"] - M).max() < 1e-6 and np.abs(pairs[0]["t"] - t).max() < 1e-6
    assert np.linalg.det(pairs[0]["M"].astype(np.float64)) > 0
    # a mirrored target: the estimate stays a proper rotation
    mir = sc.tgt * np.array([1, 1, -1], np.float32)
    _, pairs = parse(host(case([sc.tgt, mir], [[0, 1]])))
    assert abs(np.linalg.det(pairs[0]["M"].astype(np.float64)) - 1.0) < 1e-5


def test_checker_refusals(host):
    a = R.clean_scene(20).src
    b = R.clean_scene(30, seed=6).tgt
    ok = dict(sets=[a, b], pairs=[[0, 1]])
    bad = lambda **kw: host(case(**{**ok, **kw}))[0]
    assert not host(case(**ok))[0].startswith("invalid")
    nan = a.copy()
    nan[7, 1] = np.nan
    assert bad(sets=[nan, b]) == "invalid icp_host: set 0 point 7 is not finite"
    inf = b.copy()
    inf[29, 2] = -np.inf
    assert bad(sets=[a, inf]) == "invalid icp_host: set 1 point 29 is not finite"
    assert bad(sets=[a[:2], b]) == "invalid icp_host: pair 0: source set 0 has fewer than 3 points"
    assert bad(sets=[a, b[:0]]) == "invalid icp_host: pair 0: target set 1 is empty"
    assert bad(pairs=[[0, 1], [0, 2]]) == "invalid icp_host: pair 1 names a set out of range"
    assert bad(pairs=[[-1, 1]]) == "invalid icp_host: pair 0 names a set out of range"
    assert bad(set_offset=[0, 30, 20], n_points=50) == "invalid icp_host: set_offset decreases at set 1"
    assert bad(set_offset=[1, 20, 50]) == "invalid icp_host: set_offset[0] != 0"
    g = np.eye(4, dtype=np.float32)
    g[1, 3] = np.nan
    assert bad(guess=[g]) == "invalid icp_host: pair 0: guess is not finite"
    assert bad(max_iterations=0).startswith("invalid icp_host: max_iterations")
    assert bad(min_correspondences=2).startswith("invalid icp_host: min_correspondences")
    assert bad(max_corr_dist=-1.0).startswith("invalid icp_host: max_corr_dist")
    assert bad(max_corr_dist=np.nan).startswith("invalid icp_host: max_corr_dist")
    assert bad(cell=-1.0).startswith("invalid icp_host: cell") and bad(cell=np.inf).startswith("invalid icp_host: cell")
    assert bad(with_scale=2) == "invalid icp_host: unknown with_scale 2"
    assert bad(route=3) == "invalid icp_host: unknown route 3"
    assert bad(reserved=1) == "invalid icp_host: reserved must be 0"
    assert host(case(sets=[], pairs=[])) == []                                   # the empty batch is valid


# ---------------------------------------------------------------------------
# defaults, mirrors and argument errors without a device
# ---------------------------------------------------------------------------
def test_defaults_and_ctypes_mirrors(tmp_path):
    lib = N.load_library()
    p = N.ba_icp_options(max_iterations=1, max_corr_dist=1.0, mse_abs_eps=1.0, mse_rel_eps=1.0, transformation_eps=1.0,
                         min_correspondences=9, with_scale=1, fitness_max_range=1.0, route=2, cell=1.0, reserved=7)
    lib.ba_icp_defaults(C.byref(p))
    assert {k: getattr(p, k) for k in R.DEFAULTS} == R.DEFAULTS
    assert (p.route, p.cell, p.reserved) == (N.ICP_ROUTE_AUTO, 0.0, 0)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ba_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d %d %d %d\\n", sizeof(ba_icp_batch),\n'
                   '         sizeof(ba_icp_options), sizeof(ba_icp_result), offsetof(ba_icp_batch, guess),\n'
                   '         offsetof(ba_icp_options, mse_abs_eps), offsetof(ba_icp_options, fitness_max_range),\n'
                   '         offsetof(ba_icp_options, reserved), offsetof(ba_icp_result, fitness), BA_ICP_ROUTE_AUTO,\n'
                   '         BA_ICP_ROUTE_GRID, BA_ICP_ROUTE_BRUTE, BA_ICP_NOT_CONVERGED, BA_ICP_ITERATIONS, BA_ICP_TRANSFORM,\n'
                   '         BA_ICP_ABS_MSE, BA_ICP_REL_MSE, BA_ICP_NO_CORRESPONDENCES);\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(N.ba_icp_batch), C.sizeof(N.ba_icp_options), C.sizeof(N.ba_icp_result),
                   N.ba_icp_batch.guess.offset, N.ba_icp_options.mse_abs_eps.offset,
                   N.ba_icp_options.fitness_max_range.offset, N.ba_icp_options.reserved.offset,
                   N.ba_icp_result.fitness.offset, N.ICP_ROUTE_AUTO, N.ICP_ROUTE_GRID, N.ICP_ROUTE_BRUTE,
                   N.ICP_NOT_CONVERGED, N.ICP_ITERATIONS, N.ICP_TRANSFORM, N.ICP_ABS_MSE, N.ICP_REL_MSE,
                   N.ICP_NO_CORRESPONDENCES]
    assert C.sizeof(N.ba_icp_result) == 88 == ICP_RESULT_DTYPE.itemsize and C.sizeof(N.ba_icp_options) == 56
    assert ICP_RESULT_DTYPE.fields["fitness"][1] == N.ba_icp_result.fitness.offset
    assert [N.ICP_NOT_CONVERGED, N.ICP_ITERATIONS, N.ICP_TRANSFORM, N.ICP_ABS_MSE, N.ICP_REL_MSE,
            N.ICP_NO_CORRESPONDENCES] == [R.NOT_CONVERGED, R.ITERATIONS, R.TRANSFORM, R.ABS_MSE, R.REL_MSE,
                                          R.NO_CORRESPONDENCES]
    assert lib.ba_icp(None, None, None, None, None) == 1                          # BA_ERR_INVALID_ARGUMENT
    assert lib.ba_icp_nn(None, None, 0, None, None, None) == 1
    assert lib.ba_icp_times(None, None, 0) == -1


def test_pack_icp_batch():
    a, b = np.arange(12).reshape(4, 3), np.arange(9.0).reshape(3, 3)
    ib = pack_icp_batch([a, b, np.zeros((0, 3))], [[0, 1], [1, 0]])
    assert ib.set_offset.tolist() == [0, 4, 7, 7] and ib.xyz.dtype == np.float32 and ib.xyz.shape == (7, 3)
    assert ib.pairs.dtype == np.int32 and ib.pairs.tolist() == [[0, 1], [1, 0]] and ib.guess is None
    g = pack_icp_batch([a, b], [[0, 1]], guess=[np.eye(4)]).guess
    assert g.shape == (1, 4, 4) and g.dtype == np.float32
    with pytest.raises(ValueError):
        pack_icp_batch([a, b], [[0, 1]], guess=np.zeros((2, 4, 4)))


# ---------------------------------------------------------------------------
# PLY and the normalisation
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("binary", [True, False])
def test_ply_round_trip(tmp_path, binary):
    rng = np.random.default_rng(4)
    pts = (rng.normal(size=(57, 3)) * 10.0 ** rng.integers(-6, 6, size=(57, 1))).astype(np.float32)
    path = tmp_path / "cloud.ply"
    write_ply_vertices(path, pts, binary=binary)
    head = path.read_bytes().split(b"end_header\n")[0].decode()
    assert ("binary_little_endian" if binary else "ascii") in head and "element vertex 57" in head
    assert same_bits(read_ply_vertices(path), pts)
    write_ply_vertices(path, np.zeros((0, 3)), binary=binary)
    assert read_ply_vertices(path).shape == (0, 3)


def test_ply_reader_skips_other_properties_and_elements(tmp_path):
    v = np.array([[1.5, -2.0, 3.25], [0.0, 1e-3, 7.0]], np.float32)
    head = ("ply\nformat {} 1.0\ncomment made by hand\nelement thing 2\nproperty uchar a\nproperty list uchar int b\n"
            "element vertex 2\nproperty uchar red\nproperty float x\nproperty double z\nproperty float y\n"
            "element face 1\nproperty list uchar int vertex_indices\nend_header\n")
    asc = tmp_path / "a.ply"
    asc.write_text(head.format("ascii") + "7 2 1 2\n9 0\n" +
                   "".join(f"255 {p[0]!r} {p[2]!r} {p[1]!r}\n" for p in v.tolist()) + "3 0 1 0\n")
    assert same_bits(read_ply_vertices(asc), v)
    body = struct.pack("<BBii", 7, 2, 1, 2) + struct.pack("<BB", 9, 0)
    body += b"".join(struct.pack("<Bfdf", 255, p[0], p[2], p[1]) for p in v.tolist()) + struct.pack("<Biii", 3, 0, 1, 0)
    binf = tmp_path / "b.ply"
    binf.write_bytes(head.format("binary_little_endian").encode() + body)
    assert same_bits(read_ply_vertices(binf), v)
    bad = tmp_path / "c.ply"
    bad.write_text("ply\nformat binary_big_endian 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(ValueError):
        read_ply_vertices(bad)
    bad.write_text("not a ply\n")
    with pytest.raises(ValueError):
        read_ply_vertices(bad)


def test_normalisation_on_a_hand_made_cloud():
    # a 2 x 4 x 1 box of corners, posed; the target a 4 x 8 x 2 box elsewhere
    box = np.array([[x, y, z] for x in (0, 2) for y in (0, 4) for z in (0, 1)], np.float32)
    pose = R.rigid(90.0, (0, 0, 1), (5.0, -3.0, 2.0))
    world = (box.astype(np.float64) @ pose[:3, :3].T + pose[:3, 3]).astype(np.float32)
    target = 2.0 * box + np.array([10, 10, 10], np.float32)
    src, tgt, scale = reconstruction.normalise_clouds(world, target, pose)
    assert scale == pytest.approx(2.0, abs=1e-6)
    assert np.abs(src.astype(np.float64).mean(axis=0)).max() < 1e-6 and np.abs(tgt.mean(axis=0)).max() == 0
    assert np.abs(src - (box - box.mean(axis=0)) * 2.0).max() < 1e-5
    assert np.array_equal(tgt, 2.0 * box - np.array([2, 4, 1], np.float32))
    s2, t2, sc2 = R.normalise(world, target, pose)
    assert same_bits(src, s2) and same_bits(tgt, t2) and scale == sc2
    # no pose: the clouds are only centred and scaled
    src, tgt, scale = reconstruction.normalise_clouds(box, target)
    assert same_bits(src, (box - box.mean(axis=0)) * np.float32(2.0)) and scale == 2.0
    with pytest.raises(ValueError):
        reconstruction.normalise_clouds(np.zeros((0, 3)), target)
