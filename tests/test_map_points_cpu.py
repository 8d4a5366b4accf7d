"""CPU tests for ba_map_points_update / ba_associate: the pinned arithmetic
(csrc/ba_map_points.h) and the host checkers run as a stand-alone host program
under ASan + UBSan and equal the numpy float32 restatement
(tests/map_points_ref.py) bit for bit; the float32 results agree with float64
within bounds that follow from the number format; the rank index, defaults,
argument errors and the ctypes mirrors are checked without a device.  No GPU."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import map_points_ref as M
import match_ref as R
from bundleadjustment_amd import _native as N
from bundleadjustment_amd.problem import ASSOC_DTYPE, FUSE_DTYPE, MAP_POINT_DTYPE
from conftest import ROOT

F32 = np.float32


def hexbits(a) -> str:
    return " ".join(f"{v:08x}" for v in np.ascontiguousarray(a, F32).reshape(-1).view(np.uint32).tolist())


def ints(a) -> str:
    return " ".join(str(int(v)) for v in np.asarray(a).reshape(-1).tolist())


def mp_case(mb, rule=0, max_scale=M.MAX_SCALE, reserved=0, reserved_f=0.0, **override) -> str:
    f = dict(dim=mb.dim, n_cams=mb.cam_center.shape[0], n_pts=mb.pts.shape[0], n_rows=mb.desc.shape[0],
             obs_offset=mb.obs_offset, obs_cam=mb.obs_cam, obs_row=mb.obs_row, ref_obs=mb.ref_obs)
    f.update(override)
    lines = [f"mp {f['dim']} {f['n_cams']} {f['n_pts']} {f['n_rows']} {mb.obs_cam.size} {int(mb.obs_scale is not None)} "
             f"{int(f['ref_obs'] is not None)} {rule} {reserved} {hexbits([max_scale])} {hexbits([reserved_f])}",
             hexbits(mb.cam_center), hexbits(mb.pts), ints(f["obs_offset"]), ints(f["obs_cam"]), ints(f["obs_row"])]
    if mb.obs_scale is not None:
        lines.append(hexbits(mb.obs_scale))
    if f["ref_obs"] is not None:
        lines.append(ints(f["ref_obs"]))
    lines.append(hexbits(mb.desc if f["dim"] == mb.dim else np.zeros((mb.desc.shape[0], f["dim"]), F32)))
    return "\n".join(lines) + "\n"


def assoc_case(ab, reserved=0, options=None, **override) -> str:
    o = {**M.DEFAULTS, **(options or {})}
    f = dict(dim=ab.dim, item_cam=ab.item_cam, item_pt=ab.item_pt, item_row=ab.item_row, item_cur_row=ab.item_cur_row,
             fuse_pairs=ab.fuse_pairs)
    f.update(override)
    lines = [f"assoc {f['dim']} {ab.extr.shape[0]} {ab.pts.shape[0]} {ab.desc.shape[0]} {ab.item_cam.size} {ab.fuse_pairs.shape[0]} "
             f"{int(ab.item_scale is not None)} {int(f['item_cur_row'] is not None)} "
             + " ".join(hexbits([o[k]]) for k in ("chi2", "min_cos", "max_desc_dist", "fuse_min_cos", "fuse_max_desc_dist"))
             + f" {reserved}",
             hexbits(ab.extr), hexbits(ab.cam_center), hexbits(ab.K), ints(ab.image_size), hexbits(ab.pts),
             hexbits(ab.pt_view_dir), hexbits(ab.pt_dist), hexbits(ab.pt_desc[:, :f["dim"]]), hexbits(ab.desc[:, :f["dim"]]),
             ints(f["item_cam"]),
             ints(f["item_pt"]), hexbits(ab.item_uv)]
    if ab.item_scale is not None:
        lines.append(hexbits(ab.item_scale))
    lines.append(ints(f["item_row"]))
    if f["item_cur_row"] is not None:
        lines.append(ints(f["item_cur_row"]))
    lines.append(ints(f["fuse_pairs"]))
    return "\n".join(lines) + "\n"


def f32_of(words):
    return np.array([int(w, 16) for w in words], np.uint32).view(F32)


def parse_mp(out):
    plan = [int(x) for x in out[0].split()[1:]]
    pos, recs, Ds, ms = 1, [], [], []
    while pos < len(out):
        w = out[pos].split()
        n = int(w[2])
        rec = np.zeros((), MAP_POINT_DTYPE)
        v = f32_of(w[5:11])
        rec["status"], rec["best"], rec["median"], rec["view_dir"] = int(w[3]), int(w[4]), v[0], v[1:4]
        rec["min_dist"], rec["max_dist"] = v[4], v[5]
        recs.append(rec)
        Ds.append(f32_of(" ".join(out[pos + 1:pos + 1 + n]).split()).reshape(n, n))
        ms.append(f32_of(out[pos + 1 + n].split()))
        pos += n + 2
    return plan, np.array(recs, MAP_POINT_DTYPE), Ds, ms


def parse_assoc(out, ni):
    items, fuse = np.zeros(ni, ASSOC_DTYPE), np.zeros(len(out) - ni, FUSE_DTYPE)
    for i, line in enumerate(out):
        w = line.split()
        if i < ni:
            items[i] = (int(w[0]), *f32_of(w[1:]))
        else:
            fuse[i - ni] = (int(w[0]), *f32_of(w[1:]))
    return items, fuse


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("map_points_host") / "map_points_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-omit-frame-pointer", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "cpp" / "map_points_host.cpp"), "-o", str(exe)], check=True)

    def run(text: str) -> list[str]:
        case = exe.parent / "case.txt"
        case.write_text(text)
        return subprocess.run([str(exe), str(case)], capture_output=True, text=True, check=True).stdout.splitlines()
    return run


def same_bits(a, b) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------
# the rank index
# ---------------------------------------------------------------------------
def test_rank_index_is_the_references_truncation():
    """curDistances[(n / 2.0) - 1]: the double index converted to size_t truncates toward zero."""
    for n in range(1, 1025):
        assert M.rank(n) == int(n / 2.0 - 1), n
    assert [M.rank(n) for n in (1, 2, 3, 4, 5, 64, 65)] == [0, 0, 0, 1, 1, 31, 31]


# ---------------------------------------------------------------------------
# the device's text as a host program under ASan + UBSan
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [64, 128])
def test_host_program_equals_the_float32_restatement(host, dim):
    """Every track length of the GPU tests (0 .. 1024 at dim 64): D, m, best
    under both rules, view_dir and the depth bounds, bit for bit."""
    sc, parts = M.scene(dim), M.scene_parts(dim)
    n = sc.lengths()
    for rule in (M.REFERENCE, M.FLOAT):
        plan, recs, Ds, ms = parse_mp(host(mp_case(sc.batch, rule)))
        want, _ = M.update32(sc.batch, rule, parts)
        assert plan[1] == int((n <= 16).sum()) and plan[3] == int(((n > 16) & (n <= 64)).sum()) and plan[5] == int((n > 64).sum())
        for p in range(n.size):
            assert same_bits(Ds[p], parts[p][0]), ("D", p, n[p])
            assert same_bits(ms[p], parts[p][1]), ("m", p, n[p])
        bad = [p for p in range(n.size) if recs[p].tobytes() != want[p].tobytes()]
        assert not bad, (rule, bad, recs[bad[:3]], want[bad[:3]])
    # the reference rule is exercised beyond "index 0" and differs from the float rule
    ref, _ = M.update32(sc.batch, M.REFERENCE, parts)
    flt, _ = M.update32(sc.batch, M.FLOAT, parts)
    coarse = np.array([k == "coarse" for k in sc.kind])
    assert np.count_nonzero(ref["best"][coarse] > 0) >= 3 and np.any(ref["best"] != flt["best"])
    assert np.all(ref["best"][~coarse & (n > 0)] == 0)       # unit-norm rows: every truncated median is 0


def test_reference_rule_by_hand_on_three_coarse_points():
    """MapPoint.cpp:217-246 run by hand (sort, the double index, the int median,
    the strict <) on three coarse points whose truncated medians differ."""
    sc, parts = M.scene(64), M.scene_parts(64)
    n = sc.lengths()
    done = 0
    for p in range(n.size):
        D = parts[p][0]
        if sc.kind[p] != "coarse" or n[p] < 4 or n[p] > 130:
            continue
        index, smallest, meds = 0, 2 ** 31 - 1, []
        for i in range(n[p]):
            cur = sorted(D[i].tolist())
            median = int(cur[int(n[p] / 2.0 - 1)])
            meds.append(median)
            if median < smallest:
                smallest, index = median, i
        if len(set(meds)) < 2:
            continue
        assert M.choose(parts[p][1], M.REFERENCE) == index, p
        done += 1
    assert done >= 3


def test_distance_matrix_properties():
    sc, parts = M.scene(64), M.scene_parts(64)
    for p, (D, m, *_rest) in enumerate(parts):
        assert same_bits(D, np.ascontiguousarray(D.T)) and np.all(np.diag(D).view(np.uint32) == 0)
        if D.shape[0] == 8:                                   # this track names one row twice
            assert D[5, 2].view(np.uint32) == 0
        if D.shape[0] in (4, 5) and sc.kind[p] == "unit":     # k = 1: the mutually nearest rows tie; the lower index wins
            off = D + np.where(np.eye(D.shape[0], dtype=bool), np.inf, 0).astype(F32)
            i, j = np.unravel_index(np.argmin(off), off.shape)
            assert m[i].view(np.uint32) == m[j].view(np.uint32) and M.choose(m, M.FLOAT) == min(i, j)


def test_host_association_equals_the_restatement(host):
    ab, want, fwant = M.edge_scene()
    items, fuse = parse_assoc(host(assoc_case(ab)), ab.item_cam.size)
    ri, rf = M.associate32(ab)
    assert ri["status"].tolist() == want.tolist() and rf["status"].tolist() == fwant.tolist()
    assert same_bits(items, ri) and same_bits(fuse, rf)
    sc, parts = M.scene(64), M.scene_parts(64)
    rec, desc_out = M.update32(sc.batch, M.FLOAT, parts)
    ab = M.assoc_scene(sc.batch, rec, desc_out)
    items, fuse = parse_assoc(host(assoc_case(ab)), ab.item_cam.size)
    ri, rf = M.associate32(ab)
    assert set(ri["status"].tolist()) == set(range(9))        # every status occurs
    assert same_bits(items, ri) and same_bits(fuse, rf)
    options = dict(chi2=F32(3.0), min_cos=F32(0.8), max_desc_dist=F32(1.5), fuse_min_cos=F32(0.9), fuse_max_desc_dist=F32(1.41))
    items, fuse = parse_assoc(host(assoc_case(ab, options=options)), ab.item_cam.size)
    ri, rf = M.associate32(ab, **options)
    assert same_bits(items, ri) and same_bits(fuse, rf) and set(rf["status"].tolist()) == {0, 1, 2}


# ---------------------------------------------------------------------------
# the host checkers
# ---------------------------------------------------------------------------
def small_batch():
    sc = M.scene(64)
    return M.sub_batch(sc, [p for p in range(sc.lengths().size) if 0 < sc.lengths()[p] <= 8][:4])


def test_checker_refuses_bad_map_point_batches(host):
    mb = small_batch()
    no = mb.obs_cam.size

    def refused(text):
        out = host(text)
        assert len(out) == 1 and out[0].startswith("invalid map_points_host: "), out[:2]
        return out[0]
    assert "dim 96 is neither 64 nor 128" in refused(mp_case(mb, dim=96))
    assert "unknown median_rule 2" in refused(mp_case(mb, rule=2))
    for bad in (0.0, -1.0, np.inf, np.nan):
        assert "max_scale must be positive and finite" in refused(mp_case(mb, max_scale=bad))
    assert "reserved must be 0" in refused(mp_case(mb, reserved=1))
    assert "reserved must be 0" in refused(mp_case(mb, reserved_f=1.0))
    off = mb.obs_offset.copy(); off[0] = 1
    assert "obs_offset[0] != 0" in refused(mp_case(mb, obs_offset=off))
    off = mb.obs_offset.copy(); off[2] = off[1] - 1
    assert "obs_offset decreases at point 1" in refused(mp_case(mb, obs_offset=off))
    cam = mb.obs_cam.copy(); cam[no - 1] = mb.cam_center.shape[0]
    assert f"obs_cam[{no - 1}] out of range" in refused(mp_case(mb, obs_cam=cam))
    row = mb.obs_row.copy(); row[3] = -1
    assert "obs_row[3] out of range" in refused(mp_case(mb, obs_row=row))
    row[3] = mb.desc.shape[0]
    assert "obs_row[3] out of range" in refused(mp_case(mb, obs_row=row))
    ref = mb.ref_obs.copy(); ref[2] = int(np.diff(mb.obs_offset)[2])
    assert "ref_obs[2] out of range" in refused(mp_case(mb, ref_obs=ref))


def test_checker_refuses_a_track_longer_than_the_maximum(host):
    sc = M.scene(64)
    p = int(np.argmax(sc.lengths()))
    assert sc.lengths()[p] == N.BA_MP_MAX_TRACK
    mb = M.sub_batch(sc, [p], pad={0: [sc.tracks[p][0]]})
    out = host(mp_case(mb))
    assert out == ["invalid map_points_host: point 0 has a track of 1025 observations, more than 1024"]


def test_checker_refuses_bad_association_batches(host):
    ab, _, _ = M.edge_scene()

    def refused(text):
        out = host(text)
        assert len(out) == 1 and out[0].startswith("invalid map_points_host: "), out[:2]
        return out[0]
    assert "dim 32 is neither 64 nor 128" in refused(assoc_case(ab, dim=32))
    assert "reserved must be 0" in refused(assoc_case(ab, reserved=3))
    for name, bad in (("item_cam", 1), ("item_cam", -1), ("item_pt", ab.pts.shape[0]), ("item_row", ab.desc.shape[0]),
                      ("item_cur_row", -2), ("item_cur_row", ab.desc.shape[0])):
        a = getattr(ab, name).copy(); a[4] = bad
        assert f"{name}[4] out of range" in refused(assoc_case(ab, **{name: a}))
    fp = ab.fuse_pairs.copy(); fp[1, 1] = ab.pts.shape[0]
    assert "fuse_pairs[3] out of range (pair 1)" in refused(assoc_case(ab, fuse_pairs=fp))


# ---------------------------------------------------------------------------
# float64 cross-checks on unit-norm rows
# ---------------------------------------------------------------------------
def test_float32_results_agree_with_float64_within_the_format_bounds():
    """|d2_f32 - d2_f64| <= 4 (dim + 3) 2^-24; best under
    MEDIAN_FLOAT equals the float64 choice wherever the two smallest float64
    medians differ by more than twice the distance bound; view_dir within
    (n + 8) 2^-23 per component."""
    for dim in (64, 128):
        sc, parts = M.scene(dim), M.scene_parts(dim)
        bound = R.d2_bound(dim)
        worst_d2, worst_view, least_margin, compared = 0.0, 0.0, np.inf, 0
        for p in range(sc.lengths().size):
            n = int(sc.lengths()[p])
            if n == 0:
                continue
            d2_64, D64, m64, best64, view64 = M.point64(sc.batch, p)
            D, m, view = parts[p][:3]
            err = float(np.max(np.abs(view.astype(np.float64) - view64)))
            worst_view = max(worst_view, err / ((n + 8) * 2.0 ** -23))
            assert err <= (n + 8) * 2.0 ** -23, (p, n, err)
            if sc.kind[p] != "unit":
                continue
            o0 = sc.batch.obs_offset[p]
            rows = sc.batch.desc[sc.batch.obs_row[o0:o0 + n]]
            d2 = R.d2_32(rows, rows) if n <= 130 else None
            if d2 is not None:
                worst_d2 = max(worst_d2, float(np.max(np.abs(d2.astype(np.float64) - d2_64))))
            # a distance error from a d2 error: |sqrt(a) - sqrt(b)| <= |a - b| / (sqrt(a) + sqrt(b)), + one rounding of the root
            srt = np.sort(m64)
            if n >= 2 and srt[0] > 0:
                dist_bound = bound / (2 * srt[0]) + 2.0 ** -23
                margin = (srt[1] - srt[0]) / (2 * dist_bound)
                if margin > 1:
                    least_margin = min(least_margin, margin)
                    compared += 1
                    assert M.choose(m, M.FLOAT) == best64, (p, n)
        print(f"dim {dim}: max |d2_f32 - d2_f64| = {worst_d2:.3g} (bound {bound:.3g}); view_dir error / bound = {worst_view:.3g}; "
              f"{compared} points compared, least median margin / (2 bound) = {least_margin:.3g}")
        assert worst_d2 <= bound and compared >= 8


# ---------------------------------------------------------------------------
# defaults, mirrors and argument errors without a device
# ---------------------------------------------------------------------------
def test_defaults_and_ctypes_mirrors(tmp_path):
    lib = N.load_library()
    p = N.ba_map_point_options(median_rule=7, reserved=7, max_scale=1.0, reserved_f=1.0)
    lib.ba_map_points_defaults(C.byref(p))
    assert (p.median_rule, p.reserved, p.reserved_f) == (0, 0, 0.0) and F32(p.max_scale) == F32(1.2 ** 7) == M.MAX_SCALE
    a = N.ba_assoc_options()
    lib.ba_associate_defaults(C.byref(a))
    assert [F32(a.chi2), F32(a.min_cos), F32(a.max_desc_dist), F32(a.fuse_min_cos), F32(a.fuse_max_desc_dist), a.reserved] == \
        [F32(5.991), F32(0.5), F32(0.2), F32(0.0), F32(0.3), 0]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "ba_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(ba_map_point_batch), sizeof(ba_map_point_options),\n'
                   '         sizeof(ba_map_point), sizeof(ba_assoc_batch), sizeof(ba_assoc_options), sizeof(ba_assoc_result),\n'
                   '         sizeof(ba_fuse_result), BA_MP_MAX_TRACK);\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(N.ba_map_point_batch), C.sizeof(N.ba_map_point_options), C.sizeof(N.ba_map_point),
                   C.sizeof(N.ba_assoc_batch), C.sizeof(N.ba_assoc_options), C.sizeof(N.ba_assoc_result),
                   C.sizeof(N.ba_fuse_result), N.BA_MP_MAX_TRACK]
    assert C.sizeof(N.ba_map_point) == 32 == MAP_POINT_DTYPE.itemsize
    assert ASSOC_DTYPE.itemsize == C.sizeof(N.ba_assoc_result) and FUSE_DTYPE.itemsize == C.sizeof(N.ba_fuse_result)
    assert lib.ba_map_points_update(None, None, None, None, None) == 1          # BA_ERR_INVALID_ARGUMENT
    assert lib.ba_map_points_distances(None, None, 0, None, None) == 1
    assert lib.ba_associate(None, None, None, None, None) == 1
    assert lib.ba_map_points_times(None, None, 0) == -1
