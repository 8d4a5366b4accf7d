"""GPU tests of ba_map_graph (ba_map_graph.hip): covisibility lists, culling
votes, point status and local-BA windows of a batch of query frames equal the
numpy restatement (tests/map_graph_ref.py) exactly: every record and every
list, under both orders, any column tile, any batching and any chunking.
Everything is integers, so there is no tolerance anywhere but in the last
test, which solves the windows and borrows the comparisons of
tests/test_window_batch.py."""
import numpy as np
import pytest

import map_graph_ref as G
from bundleadjustment_amd import (Options, Solver, make_synthetic, map_table_from_problem, pack_window_batch,
                                  windows_from_graph)
from bundleadjustment_amd._native import BAError
from bundleadjustment_amd.problem import MapTable, fix_camera
from conftest import assert_close, compare_logs

pytestmark = pytest.mark.gpu

INVALID = 1   # BA_ERR_INVALID_ARGUMENT
ALL = np.arange(G.N_FRAMES)
CUR = G.CURRENT_FRAME_ID


@pytest.fixture(scope="module")
def solver():
    s = Solver(0)
    yield s
    s.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------
# 1. every record and every list on the scene
# ---------------------------------------------------------------------------
def test_scene_holds_every_case():
    G.assert_scene_cases()


@pytest.mark.parametrize("order", [G.WEAKEST_FIRST, G.STRONGEST_FIRST])
@pytest.mark.parametrize("n_best", [0, 3, 10, 15])
def test_scene_equals_the_restatement(solver, order, n_best):
    got = solver.map_graph(G.scene().table, ALL, pt_status=True, order=order, n_best=n_best, current_frame_id=CUR)
    want = G.scene_result(order, n_best)
    assert G.same(got, want) == []
    assert got.records["n_local"].max() == min(n_best, 39) + 1
    again = solver.map_graph(G.scene().table, ALL, pt_status=True, order=order, n_best=n_best, current_frame_id=CUR)
    assert G.same(again, got) == []
    t = solver.map_graph_times()
    assert t.shape == (3,) and t[2] >= t[0] > 0.0 and t[1] > 0.0


def test_windows_off_and_other_thresholds(solver):
    t = G.scene().table
    for kw in (dict(build_windows=0), dict(th=0), dict(th=100, n_best=2), dict(redundant_fraction=0.5), dict(redundant_fraction=-1.0)):
        assert G.same(solver.map_graph(t, ALL, **kw), G.graph(t, ALL, **kw)) == [], kw
    off = solver.map_graph(t, ALL, build_windows=0)
    assert off.records["n_local"].max() == 0 and all(a.size == 0 for a in off.win_cam + off.win_obs)


# ---------------------------------------------------------------------------
# 2. raw weight rows and column tiles
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [0, 16, 17])
def test_weight_rows_and_lists_under_tilings(solver, tile):
    t = G.scene().table
    v = G.View(t)
    for q in range(G.N_FRAMES):
        W = solver.map_graph_weights(t, q, debug_tile_frames=tile)
        assert W.dtype == np.int32 and W.tolist() == G.weights(v, q).tolist(), q
    got = solver.map_graph(t, ALL, pt_status=True, current_frame_id=CUR, debug_tile_frames=tile)
    assert G.same(got, G.scene_result()) == []


# ---------------------------------------------------------------------------
# 3. batching and chunking
# ---------------------------------------------------------------------------
def test_a_querys_bits_do_not_depend_on_the_batch(solver):
    t = G.scene().table
    want = G.scene_result()
    rng = np.random.default_rng(3)
    sub = rng.permutation(G.N_FRAMES)[:17]
    for q in (sub, [5, G.NAMES["D"], 5, 5, G.NAMES["I"], G.NAMES["D"]], [G.NAMES["V5"]], [0]):
        got = solver.map_graph(t, q, pt_status=True, current_frame_id=CUR)
        assert G.same(got, G.take(want, q)) == []
    for chunk in (13, 7, 1):         # 40 queries in 4, 6 and 40 chunks
        got = solver.map_graph(t, ALL, pt_status=True, current_frame_id=CUR, debug_chunk_queries=chunk)
        assert G.same(got, want) == [], chunk
    got = solver.map_graph(t, np.concatenate([ALL, sub]), pt_status=True, current_frame_id=CUR, debug_chunk_queries=13,
                           debug_tile_frames=17)
    assert G.same(got, G.take(want, np.concatenate([ALL, sub]))) == []


# ---------------------------------------------------------------------------
# 4. optional arrays, empty batches and tables
# ---------------------------------------------------------------------------
def test_null_optional_arrays_equal_explicit_ones(solver):
    t = G.scene().table
    full = dict(frame_id=t.frame_id, obs_offset=t.obs_offset, obs_frame=t.obs_frame, frame_is_key=t.frame_is_key,
                pt_invalid=t.pt_invalid, pt_ref_frame=t.pt_ref_frame, obs_octave=t.obs_octave, obs_outlier=t.obs_outlier)
    neutral = dict(frame_is_key=np.ones(t.n_frames, np.uint8), pt_invalid=np.zeros(t.n_pts, np.uint8),
                   obs_octave=np.zeros(t.n_obs, np.int32), obs_outlier=np.zeros(t.n_obs, np.uint8))
    for name, explicit in neutral.items():
        a = solver.map_graph(MapTable(**{**full, name: None}), ALL, pt_status=True, current_frame_id=CUR)
        b = solver.map_graph(MapTable(**{**full, name: explicit}), ALL, pt_status=True, current_frame_id=CUR)
        assert G.same(a, b) == [] and G.same(a, G.graph(MapTable(**{**full, name: explicit}), ALL, pt_status=True,
                                                        current_frame_id=CUR)) == [], name
        assert G.same(a, G.scene_result()) != [], name         # the array matters on this scene
    bare = MapTable(frame_id=t.frame_id, obs_offset=t.obs_offset, obs_frame=t.obs_frame)
    assert G.same(solver.map_graph(bare, ALL), G.graph(bare, ALL)) == []
    with pytest.raises(BAError) as e:
        solver.map_graph(bare, ALL, pt_status=True)
    assert e.value.status == INVALID and "pt_status needs pt_ref_frame" in str(e.value)


def test_empty_batch_empty_table_and_all_points_invalid(solver):
    t = G.scene().table
    got = solver.map_graph(t, [], pt_status=True, current_frame_id=CUR)
    assert got.records.size == 0 and got.nbr_frame == [] and np.array_equal(got.pt_status, G.scene_result().pt_status)
    empty = MapTable(frame_id=np.arange(5), obs_offset=np.zeros(8), obs_frame=np.zeros(0),
                     pt_ref_frame=np.zeros(7)).normalized()
    got = solver.map_graph(empty, [0, 4, 4], pt_status=True, current_frame_id=9)
    assert G.same(got, G.graph(empty, [0, 4, 4], pt_status=True, current_frame_id=9)) == []
    assert got.records["status"].tolist() == [G.ISOLATED] * 3 and got.records["n_local"].tolist() == [1] * 3
    assert solver.map_graph_weights(empty, 2).tolist() == [0] * 5
    bad = MapTable(frame_id=t.frame_id, obs_offset=t.obs_offset, obs_frame=t.obs_frame, frame_is_key=t.frame_is_key,
                   pt_invalid=np.ones(t.n_pts, np.uint8), pt_ref_frame=t.pt_ref_frame, obs_octave=t.obs_octave,
                   obs_outlier=t.obs_outlier).normalized()
    got = solver.map_graph(bad, ALL, pt_status=True, current_frame_id=CUR)
    assert G.same(got, G.graph(bad, ALL, pt_status=True, current_frame_id=CUR)) == []
    assert got.records["n_map"].max() == 0 and got.records["n_win_pts"].max() == 0 and got.records["degree"].max() > 15
    assert set(got.pt_status.tolist()) == {G.PT_INVALID}


def test_argument_errors_name_the_culprit(solver):
    t = G.scene().table
    for q, kw, text in (([0, 40], {}, "query[1] out of range"), ([0], dict(n_best=16), "n_best 16 outside 0 .. 15"),
                        ([0], dict(order=2), "unknown order 2"), ([0], dict(reserved=1), "reserved must be 0"),
                        ([0], dict(redundant_fraction=np.nan), "redundant_fraction must be finite")):
        with pytest.raises(BAError) as e:
            solver.map_graph(t, q, **kw)
        assert e.value.status == INVALID and text in str(e.value)
    fr = t.obs_frame.copy(); fr[11] = 40
    with pytest.raises(BAError) as e:
        solver.map_graph(MapTable(frame_id=t.frame_id, obs_offset=t.obs_offset, obs_frame=fr), [0])
    assert "obs_frame[11] out of range" in str(e.value)
    with pytest.raises(BAError) as e:
        solver.map_graph_weights(t, -1)
    assert "query[0] out of range" in str(e.value)


# ---------------------------------------------------------------------------
# 5. a larger table
# ---------------------------------------------------------------------------
def test_larger_table_equals_the_restatement(solver):
    """300 frames x 20 000 points x 8 views: several hundred workgroups, lists of
    more than 30 neighbours, point bitmaps of 625 words, windows of thousands of
    observations."""
    rng = np.random.default_rng(11)
    nf, npts, views = 300, 20000, 8
    start = rng.integers(0, nf, npts)
    frame = ((start[:, None] + np.sort(rng.choice(60, size=(npts, views)), axis=1)) % nf)
    lens = rng.integers(0, views + 1, npts)
    lens[:50] = views
    keep = np.arange(views)[None, :] < lens[:, None]
    off = np.concatenate([[0], np.cumsum(lens)])
    no = int(off[-1])
    t = MapTable(frame_id=rng.permutation(nf), obs_offset=off, obs_frame=frame[keep], frame_is_key=rng.random(nf) > 0.1,
                 pt_invalid=rng.random(npts) < 0.05, pt_ref_frame=start, obs_octave=rng.integers(0, 8, no),
                 obs_outlier=rng.random(no) < 0.1).normalized()
    q = np.arange(nf)
    kw = dict(pt_status=True, current_frame_id=150, th=15, redundant_fraction=0.56)
    want = G.graph(t, q, **kw)
    got = solver.map_graph(t, q, **kw)
    assert G.same(got, want) == []
    assert want.records["degree"].max() > 30 and want.records["n_win_obs"].max() > 5000
    assert set(want.records["cull"].tolist()) == {0, 1} and set(want.pt_status.tolist()) == {0, 1, 2, 3}
    got = solver.map_graph(t, q[::7], order=G.STRONGEST_FIRST, th=15, debug_tile_frames=64, debug_chunk_queries=10)
    assert G.same(got, G.graph(t, q[::7], order=G.STRONGEST_FIRST, th=15)) == []


# ---------------------------------------------------------------------------
# 6. end to end: table from a Problem, windows, ba_solve_window_batch
# ---------------------------------------------------------------------------
def test_windows_solve_in_one_batch_as_they_do_alone(solver):
    p = make_synthetic(24, 1500, 6, seed=0xBA5E0261, intr="freiburg")
    table = map_table_from_problem(p)
    assert table.n_frames == 24 and table.n_pts == 1500 and table.n_obs == p.n_obs
    queries = [3, 11, 0, 20]
    res = solver.map_graph(table, queries)
    assert G.same(res, G.graph(table, queries)) == []
    wins = windows_from_graph(p, res)
    assert len(wins) == 4
    for i, w in enumerate(wins):
        r = res.records[i]
        assert w.n_cams == r["n_local"] + r["n_fixed"] and w.n_pts == r["n_win_pts"] and w.n_obs == r["n_win_obs"]
        assert int((1 - w.cam_fixed).sum()) <= 11 and w.n_obs > 0
        assert w.cam_fixed.tolist() == res.win_cam_fixed[i].tolist()
        assert same_bits(w.obs_uv, p.obs_uv[table.order[res.win_obs[i]]]) and same_bits(w.K, p.K[res.win_cam[i]])
        assert same_bits(w.pts, p.pts[res.win_pt[i]])
        assert np.array_equal(res.win_cam[i][w.obs_cam], p.obs_cam[table.order[res.win_obs[i]]])
        assert np.array_equal(res.win_pt[i][w.obs_pt], p.obs_pt[table.order[res.win_obs[i]]])
        c = int(np.flatnonzero(w.cam_fixed)[0])          # a fixed camera is formed the way fix_camera forms it
        alone = w.copy()
        alone.cams[c], alone.cam_fixed[c], alone.cam_fixed_extr[c] = p.cams[res.win_cam[i][c]], 0, 0.0
        alone = fix_camera(alone, c)
        assert same_bits(alone.cams[c], w.cams[c]) and same_bits(alone.cam_fixed_extr[c], w.cam_fixed_extr[c])
        assert alone.cam_fixed[c] == 1 and np.any(w.cam_fixed_extr[c] != 0)
    # frame id 0 (camera 0) is a local frame of its own window and is flagged fixed there
    assert res.win_cam[2][res.records["n_local"][2] - 1] == 0 and res.win_cam_fixed[2][res.records["n_local"][2] - 1] == 1
    opts = Options(max_num_iterations=15)
    out, summs = solver.solve_window_batch(wins, opts)
    assert pack_window_batch(wins).n_problems == 4
    for i, w in enumerate(wins):
        # the comparisons of tests/test_window_batch.py::test_one_window_matches_oracle_and_ba_solve
        log = solver.window_iteration_log(i)
        solver.set_problem(w)
        gs = solver.solve(opts)
        gc, gp = solver.params()
        (cams, pts), summ = out[i], summs[i]
        assert summ.termination_type == gs.termination_type and summ.num_iterations == gs.num_iterations
        assert summ.final_cost == pytest.approx(gs.final_cost, rel=1e-10)
        assert_close(cams, gc, 1e-8, 1e-10, "cameras vs ba_solve")
        assert_close(pts, gp, 1e-8, 1e-10, "points vs ba_solve")
        compare_logs(log, solver.iteration_log())


# ---------------------------------------------------------------------------
# 7. the lists need a graph call; the context's problem is untouched
# ---------------------------------------------------------------------------
def test_lists_before_any_graph_call_and_an_untouched_solve():
    from bundleadjustment_amd import _native as N
    import ctypes as C
    p = fix_camera(make_synthetic(8, 300, 4, seed=0xBA5E0262, intr="freiburg"), 1)
    with Solver(0) as s:
        out = N.ba_graph_lists()
        assert s.lib.ba_map_graph_lists(s.h, C.byref(out)) == INVALID
        assert "no ba_map_graph result" in s.lib.ba_last_error(s.h).decode()
        s.set_problem(p.copy())
        s1 = s.solve(Options(max_num_iterations=8))
        c1, p1 = s.params()
        log1 = s.iteration_log()
        s.set_problem(p.copy())
        got = s.map_graph(G.scene().table, ALL, pt_status=True, current_frame_id=CUR)
        assert G.same(got, G.scene_result()) == []
        with pytest.raises(BAError):
            s.map_graph(G.scene().table, [99])
        # a refused call launches nothing: the lists are still those of the last successful call; any array may be NULL
        nbr = np.zeros(int(got.records["degree"].sum()), np.int32)
        out.nbr_weight = nbr.ctypes.data_as(C.c_void_p)
        assert s.lib.ba_map_graph_lists(s.h, C.byref(out)) == 0
        assert nbr.tolist() == np.concatenate(got.nbr_weight).tolist()
        s.map_graph_weights(G.scene().table, 3)
        s2 = s.solve(Options(max_num_iterations=8))
        c2, p2 = s.params()
        assert same_bits(c1, c2) and same_bits(p1, p2) and s1.final_cost == s2.final_cost
        strip = lambda log: [{k: v for k, v in r.items() if not k.endswith("time_s")} for r in log]
        assert strip(log1) == strip(s.iteration_log())
