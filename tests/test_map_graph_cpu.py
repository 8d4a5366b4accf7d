"""CPU tests for ba_map_graph: the host checker, the frame-sorted plan and the
plain C++ restatement (host/ba_batch_pack.hpp, csrc/ba_map_graph.h) run as a
stand-alone host program under ASan + UBSan and equal the numpy restatement
(tests/map_graph_ref.py) field for field; a dense brute-force second
restatement checks the first; the scene holds every case it was built for;
defaults, argument errors and the ctypes mirrors are checked without a
device.  No GPU."""
import ctypes as C
import struct
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import map_graph_ref as G
from bundleadjustment_amd import _native as N
from bundleadjustment_amd.problem import GRAPH_FRAME_DTYPE, MapTable
from conftest import ROOT

ARRAYS = ("frame_id", "frame_is_key", "pt_invalid", "pt_ref_frame", "obs_offset", "obs_frame", "obs_octave", "obs_outlier")


def ints(a) -> str:
    return " ".join(str(int(v)) for v in np.asarray(a).reshape(-1).tolist())


def case(t: MapTable, queries, want_status=0, table_reserved=0, tile=0, chunk=0, reserved=0, null=(), counts=None, **options):
    """The text of one run.  null: names of arrays passed as NULL; counts: overrides of n_frames / n_pts / n_obs /
    n_query; the other keywords override an array of the table or an option."""
    o = {**G.DEFAULTS, **{k: v for k, v in options.items() if k in G.DEFAULTS}}
    arr = {k: getattr(t, k) for k in ARRAYS}
    arr.update({k: v for k, v in options.items() if k in ARRAYS})
    arr["query"] = np.asarray(queries, np.int64)
    n = dict(n_frames=t.n_frames, n_pts=t.n_pts, n_obs=t.n_obs, n_query=arr["query"].size)
    n.update(counts or {})
    have = sum(1 << b for b, k in enumerate((*ARRAYS, "query")) if arr[k] is not None and k not in null)
    frac = struct.unpack("<Q", struct.pack("<d", float(o["redundant_fraction"])))[0]
    lines = [f"graph {n['n_frames']} {n['n_pts']} {n['n_obs']} {n['n_query']} {have} {want_status} {table_reserved}",
             f"{o['th']} {o['n_best']} {o['order']} {o['build_windows']} {o['current_frame_id']} {tile} {chunk} {reserved} {frac:x}"]
    lines += [ints(arr[k]) for b, k in enumerate((*ARRAYS, "query")) if (have >> b) & 1]
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("map_graph_host") / "map_graph_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fno-omit-frame-pointer", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    str(ROOT / "tests" / "cpp" / "map_graph_host.cpp"), "-o", str(exe)], check=True)

    def run(text: str) -> list[str]:
        path = exe.parent / "case.txt"
        path.write_text(text)
        return subprocess.run([str(exe), str(path)], capture_output=True, text=True, check=True).stdout.splitlines()
    return run


def parse(out, nq, want_status):
    vals = lambda s, dt=np.int32: np.array(s.split()[1:], np.int64).astype(dt)
    plan = [int(x) for x in out[0].split()[1:]]
    frame_off, perm = vals(out[1]), vals(out[2])
    res = SimpleNamespace(records=np.zeros(nq, GRAPH_FRAME_DTYPE), pt_status=None, **{k: [] for k in G.LISTS})
    Ws, pos = [], 3
    for i in range(nq):
        assert out[pos].startswith("rec ")
        res.records[i] = tuple(vals(out[pos]).tolist())
        Ws.append(vals(out[pos + 1], np.int64))
        for j, k in enumerate(G.LISTS):
            assert out[pos + 2 + j].split()[0] == k
            getattr(res, k).append(vals(out[pos + 2 + j], np.uint8 if k == "win_cam_fixed" else np.int32))
        pos += 10
    if want_status:
        res.pt_status = vals(out[pos], np.uint8)
        pos += 1
    assert pos == len(out)
    return plan, frame_off, perm, Ws, res


# ---------------------------------------------------------------------------
# the scene and the restatement itself
# ---------------------------------------------------------------------------
def test_scene_holds_every_case():
    sc = G.scene()
    t = sc.table
    assert t.n_frames == 40 and 2900 <= t.n_pts <= 3300
    lens = np.diff(t.obs_offset)
    assert set(lens[:2800].tolist()) == set(range(13)) and lens[sc.every] == 40
    assert 0.07 < t.obs_outlier.mean() < 0.13 and 0.03 < t.pt_invalid.mean() < 0.07
    assert set(t.obs_octave.tolist()) == set(range(8)) and 0 < (t.frame_is_key == 0).sum() <= 4
    G.assert_scene_cases()


def brute(t: MapTable, q: int, o: dict):
    """A second restatement of one query: a dense points x frames count matrix
    and Python loops per frame and per observation."""
    v = G.View(t)
    A = np.zeros((v.np, v.nf), np.int64)          # observations of frame f on point p
    A_in = np.zeros((v.np, v.nf), np.int64)       # ... that are not outliers
    for k in range(v.no):
        A[v.pt[k], v.frame[k]] += 1
        A_in[v.pt[k], v.frame[k]] += 0 if v.outlier[k] else 1
    W = (A_in.T @ A)[q].copy()                    # (A_in^T A)[q][g] = sum_p in(q, p) all(g, p)
    W[q] = 0
    cand = sorted((int(W[g]), g) for g in range(v.nf) if W[g] > o["th"] and v.key[g])
    status = G.OK
    if not cand:
        status = G.ISOLATED
        if W.max() > 0:
            g = min(g for g in range(v.nf) if W[g] == W.max())
            cand, status = [(int(W[g]), g)], G.FALLBACK
    lst = [g for _, g in cand]
    best = lst if o["order"] == G.WEAKEST_FIRST else [g for _, g in sorted(((-w, g) for w, g in cand))]
    local = best[:o["n_best"]] + [q]
    n_map = n_red = 0
    for k in range(v.no):
        if v.frame[k] != q or v.invalid[v.pt[k]]:
            continue
        n_map += 1
        track = range(v.off[v.pt[k]], v.off[v.pt[k] + 1])
        views = sum(1 for j in track if v.frame[j] != q and v.octave[j] <= v.octave[k] + 1)
        n_red += int(len(track) > 3 and views >= 3)
    cull = int(v.frame_id[q] not in (0, 1) and n_map * o["redundant_fraction"] < n_red)
    pts = [p for p in range(v.np) if not v.invalid[p] and A_in[p, local].sum() > 0]
    fixed = [g for g in range(v.nf) if v.key[g] and g not in local and A_in[pts, g].sum() > 0]
    cams = local + fixed
    obs = [k for k in range(v.no) if v.pt[k] in set(pts) and not v.outlier[k] and v.frame[k] in cams]
    rec = (status, len(lst), int(W.max()), n_map, n_red, cull, len(local), len(fixed), len(pts), len(obs))
    return rec, W, lst, cams, [int(c >= len(local) or v.frame_id[g] == 0) for c, g in enumerate(cams)], pts, obs, \
        [cams.index(int(v.frame[k])) for k in obs], [pts.index(int(v.pt[k])) for k in obs]


def small_table(seed=5):
    """12 frames, 90 points, thresholds scaled down so that every status occurs."""
    rng = np.random.default_rng(seed)
    tracks = [np.sort(rng.choice(10, size=int(rng.integers(0, 7)), replace=False)).tolist() for _ in range(84)]
    tracks += [[10, 3]] * 2 + [[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10]] + [[2, 2, 5]] + [[11]] * 2     # 11 is isolated; one duplicate pair
    off = np.zeros(len(tracks) + 1, np.int64)
    np.cumsum([len(x) for x in tracks], out=off[1:])
    no = int(off[-1])
    key = np.ones(12, np.uint8); key[[4, 9]] = 0
    fid = np.arange(12) + 3; fid[6], fid[7] = 0, 1
    return MapTable(frame_id=fid, obs_offset=off, obs_frame=np.array([f for x in tracks for f in x]), frame_is_key=key,
                    pt_invalid=(rng.random(len(tracks)) < 0.1), pt_ref_frame=rng.integers(0, 12, len(tracks)),
                    obs_octave=rng.integers(0, 4, no), obs_outlier=(rng.random(no) < 0.15)).normalized()


@pytest.mark.parametrize("order,n_best,th", [(0, 3, 8), (1, 3, 8), (0, 0, 30), (1, 15, 2)])
def test_restatement_equals_a_dense_brute_force(order, n_best, th):
    t = small_table()
    o = {**G.DEFAULTS, "order": order, "n_best": n_best, "th": th, "redundant_fraction": 0.5}
    res = G.graph(t, np.arange(12), **o)
    v = G.View(t)
    seen = set()
    for q in range(12):
        rec, W, lst, cams, fixed, pts, obs, ocam, opt = brute(t, q, o)
        seen.add(rec[0])
        assert tuple(res.records[q].tolist()) == rec, q
        assert G.weights(v, q).tolist() == W.tolist()
        got = [getattr(res, k)[q].tolist() for k in G.LISTS]
        assert got == [lst, [int(W[g]) for g in lst], cams, fixed, pts, obs, ocam, opt], q
    if th == 8:
        assert seen == {G.OK, G.FALLBACK, G.ISOLATED}


# ---------------------------------------------------------------------------
# the host program under ASan + UBSan
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("order,n_best", [(0, 10), (1, 10), (0, 0), (1, 3), (0, 15)])
def test_host_program_equals_the_restatement_on_the_scene(host, order, n_best):
    t = G.scene().table
    q = np.arange(G.N_FRAMES)
    out = host(case(t, q, want_status=1, order=order, n_best=n_best, current_frame_id=G.CURRENT_FRAME_ID))
    plan, frame_off, perm, Ws, res = parse(out, q.size, True)
    want = G.scene_result(order, n_best)
    assert G.same(res, want) == []
    v = G.View(t)
    assert all(Ws[i].tolist() == G.weights(v, i).tolist() for i in range(q.size))
    # the plan: a stable counting sort by frame; one tile and one chunk at this size
    assert plan == [40, 40]
    assert frame_off.tolist() == np.concatenate([[0], np.cumsum(np.bincount(t.obs_frame, minlength=40))]).tolist()
    assert perm.tolist() == np.argsort(t.obs_frame, kind="stable").tolist()


def test_host_program_on_small_tables_and_debug_fields(host):
    t = small_table()
    q = [5, 11, 5, 0, 2]
    for kw in (dict(th=8, n_best=3), dict(th=8, n_best=3, build_windows=0), dict(th=2, order=1, redundant_fraction=0.5)):
        plan, _, _, _, res = parse(host(case(t, q, tile=5, chunk=2, **kw)), len(q), False)
        assert plan == [5, 2] and G.same(res, G.graph(t, q, **kw)) == []
    # optional arrays as NULL equal explicit zeros / ones
    bare = MapTable(frame_id=t.frame_id, obs_offset=t.obs_offset, obs_frame=t.obs_frame)
    _, _, _, _, res = parse(host(case(bare, q, th=3)), len(q), False)
    assert G.same(res, G.graph(bare, q, th=3)) == []
    # empty batch, empty table
    assert parse(host(case(t, [], null=("query",))), 0, False)[4].records.size == 0
    empty = MapTable(frame_id=np.arange(3), obs_offset=np.zeros(5), obs_frame=np.zeros(0)).normalized()
    _, _, _, _, res = parse(host(case(empty, [0, 2])), 2, False)
    assert G.same(res, G.graph(empty, [0, 2])) == [] and res.records["status"].tolist() == [G.ISOLATED] * 2


def test_checker_refuses_bad_tables(host):
    t = small_table()
    q = [1, 2, 3]

    def refused(text):
        out = host(text)
        assert len(out) == 1 and out[0].startswith("invalid map_graph_host: "), out[:2]
        return out[0]
    for name in ("frame_id", "obs_offset", "obs_frame", "query"):
        assert f"null array {name}" in refused(case(t, q, null=(name,)))
    for name in ("n_frames", "n_pts", "n_obs", "n_query"):
        assert "bad table" in refused(case(t, q, counts={name: -1}))
    off = t.obs_offset.copy(); off[0] = 1
    assert "obs_offset[0] != 0" in refused(case(t, q, obs_offset=off))
    off = t.obs_offset.copy(); off[4] = off[3] - 1
    assert "obs_offset decreases at point 3" in refused(case(t, q, obs_offset=off))
    off = t.obs_offset.copy(); off[-1] += 1
    assert f"obs_offset[n_pts] is {off[-1]}, not n_obs {t.n_obs}" in refused(case(t, q, obs_offset=off))
    for bad in (-1, 12):
        fr = t.obs_frame.copy(); fr[7] = bad
        assert "obs_frame[7] out of range" in refused(case(t, q, obs_frame=fr))
        ref = t.pt_ref_frame.copy(); ref[5] = bad
        assert "pt_ref_frame[5] out of range" in refused(case(t, q, pt_ref_frame=ref))
        assert "query[2] out of range" in refused(case(t, [1, 2, bad]))
    assert "n_best -1 outside 0 .. 15" in refused(case(t, q, n_best=-1))
    assert "n_best 16 outside 0 .. 15" in refused(case(t, q, n_best=16))
    assert "unknown order 2" in refused(case(t, q, order=2))
    assert "th -1 is negative" in refused(case(t, q, th=-1))
    for bad in (np.inf, -np.inf, np.nan):
        assert "redundant_fraction must be finite" in refused(case(t, q, redundant_fraction=bad))
    assert "reserved must be 0" in refused(case(t, q, reserved=1))
    assert "reserved must be 0" in refused(case(t, q, table_reserved=1))
    assert "a debug field is negative" in refused(case(t, q, tile=-1))
    assert "a debug field is negative" in refused(case(t, q, chunk=-1))
    assert "pt_status needs pt_ref_frame" in refused(case(t, q, want_status=1, null=("pt_ref_frame",)))


# ---------------------------------------------------------------------------
# defaults, mirrors and argument errors without a device
# ---------------------------------------------------------------------------
def test_defaults_and_ctypes_mirrors(tmp_path):
    lib = N.load_library()
    p = N.ba_graph_options(th=1, n_best=1, order=1, build_windows=0, current_frame_id=5, debug_tile_frames=3,
                           debug_chunk_queries=3, reserved=3, redundant_fraction=0.5)
    lib.ba_map_graph_defaults(C.byref(p))
    assert (p.th, p.n_best, p.order, p.build_windows, p.current_frame_id, p.debug_tile_frames, p.debug_chunk_queries,
            p.reserved, p.redundant_fraction) == (10, 10, 0, 1, 0, 0, 0, 0, 0.95)
    assert {k: getattr(p, k) for k in G.DEFAULTS} == G.DEFAULTS
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "ba_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %d %d %d %d %d %d\\n", sizeof(ba_map_table), sizeof(ba_graph_options),\n'
                   '         sizeof(ba_graph_frame), sizeof(ba_graph_lists), BA_GRAPH_ISOLATED, BA_GRAPH_STRONGEST_FIRST,\n'
                   '         BA_GRAPH_PT_RECENT, BA_GRAPH_PT_MATURE, BA_GRAPH_PT_ERASE, BA_GRAPH_PT_INVALID);\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(N.ba_map_table), C.sizeof(N.ba_graph_options), C.sizeof(N.ba_graph_frame),
                   C.sizeof(N.ba_graph_lists), N.GRAPH_ISOLATED, N.GRAPH_STRONGEST_FIRST, N.GRAPH_PT_RECENT,
                   N.GRAPH_PT_MATURE, N.GRAPH_PT_ERASE, N.GRAPH_PT_INVALID]
    assert C.sizeof(N.ba_graph_frame) == 40 == GRAPH_FRAME_DTYPE.itemsize and C.sizeof(N.ba_graph_options) == 40
    assert [N.GRAPH_OK, N.GRAPH_FALLBACK, N.GRAPH_ISOLATED] == [G.OK, G.FALLBACK, G.ISOLATED]
    assert [N.GRAPH_PT_RECENT, N.GRAPH_PT_MATURE, N.GRAPH_PT_ERASE, N.GRAPH_PT_INVALID] == \
        [G.PT_RECENT, G.PT_MATURE, G.PT_ERASE, G.PT_INVALID]
    assert lib.ba_map_graph(None, None, None, 0, None, None, None) == 1          # BA_ERR_INVALID_ARGUMENT
    assert lib.ba_map_graph_lists(None, None) == 1
    assert lib.ba_map_graph_weights(None, None, 0, None, None) == 1
    assert lib.ba_map_graph_times(None, None, 0) == -1
