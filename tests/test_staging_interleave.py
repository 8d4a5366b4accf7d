"""The staging arenas of the map-point, ICP and map-graph entry points under
growth, reuse at a smaller size and interleaving: one context runs map-points
update small -> large -> small, the distance inspection, the association gates,
ICP small -> large -> small with the correspondence pass in between, and the
map graph on a small table -> a larger one -> the small one with the weight row
and the lists read after each; every result equals, byte for byte, the same
call on a fresh context.  (test_match.py, test_pnp.py, test_two_view.py and
test_triangulate.py pin the other arenas the same way.)

Shapes: the smallest that grow the buffer, reuse it at a smaller size and fill
every section.  Map points: 3 tracks and 204, one and many in each tier of
map_points_plan, at dim 64 (the smaller of the two descriptor sizes the entry
accepts).  ICP: 1 pair of 40 points; 4 pairs over sources of 257 and 300 points,
two on the brute route and two on the grid route.  The route is an option of
the call, and only AUTO mixes both in one batch: it takes the grid for a target
of more than 2048 points (kIcpBruteMax), so one target has 2100 points and the
other 300.  Map graph: tables of 8 and 40 frames with windows on."""
import numpy as np
import pytest

import icp_ref as I
import map_graph_ref as G
import map_points_ref as M
from bundleadjustment_amd import Solver, make_synthetic, map_table_from_problem, pack_icp_batch

pytestmark = pytest.mark.gpu


def map_point_batches():
    sc = M.scene(64)
    n = sc.lengths()
    tier = np.array([0 if k <= 16 else 1 if k <= 64 else 2 for k in n])
    small = [int(np.flatnonzero((tier == t) & (n > 0))[0]) for t in (0, 1, 2)]
    body = [p for p in range(n.size) if n[p] <= 130]           # (the two 1024-tracks once, not six times)
    large = body * 6 + [p for p in range(n.size) if n[p] > 130]
    assert len(small) == 3 and 190 <= len(large) <= 215 and {0, 1, 2} == set(tier[large].tolist())
    return sc, M.sub_batch(sc, small), M.sub_batch(sc, large), large.index(int(np.flatnonzero(n == 17)[0]))


def icp_batches():
    a, b = I.clean_scene(300), I.noisy_scene(257, 2100)
    small = pack_icp_batch([I.clean_scene(40).src, I.clean_scene(40).tgt], [[0, 1]])
    large = pack_icp_batch([a.src, a.tgt, b.src, b.tgt], [[0, 1], [2, 3], [0, 3], [2, 1]])   # AUTO: brute, grid, grid, brute
    return small, large


def graph_bytes(r):
    return [r.records.tobytes(), None if r.pt_status is None else r.pt_status.tobytes()] + \
           [[a.tobytes() for a in getattr(r, k)] for k in G.LISTS]


def test_staging_arenas_of_map_points_icp_and_map_graph_interleave_bitwise():
    sc, mp_small, mp_large, p17 = map_point_batches()
    icp_small, icp_large = icp_batches()
    prob = make_synthetic(8, 200, 4, seed=0xBA5E0901)
    g_small = map_table_from_problem(prob, pt_ref_frame=np.zeros(prob.n_pts, np.int32))
    g_large = G.scene().table
    with Solver(0) as s:                                       # the association scene needs the scene's own records
        rec, desc = s.map_points_update(sc.batch)
    ab = M.assoc_scene(sc.batch, rec, desc)

    def update(mb, **kw):
        def call(s):
            r, d = s.map_points_update(mb, **kw)
            return [r.tobytes(), None if d is None else d.tobytes()]
        return call

    def icp(ib):
        return lambda s: [a.tobytes() for a in s.icp(ib)]

    def graph(t, q, **kw):
        def call(s):
            r = s.map_graph(t, q, pt_status=True, **kw)
            assert r.records["n_local"].max() > 1 and sum(a.size for a in r.win_obs) > 0   # windows were built
            return graph_bytes(r)
        return call

    calls = {
        "mp_small": update(mp_small), "mp_large": update(mp_large, median_rule=M.FLOAT),
        "mp_large_no_desc": update(mp_large, want_desc=False),
        "mp_dist": lambda s: [a.tobytes() for a in s.map_points_distances(mp_large, p17)],
        "assoc": lambda s: [a.tobytes() for a in s.associate(ab)],
        "icp_small": icp(icp_small), "icp_large": icp(icp_large),
        "icp_nn": lambda s: [a.tobytes() for a in s.icp_nn(icp_large, pair=1)],
        "g_small": graph(g_small, np.arange(8)),
        "g_large": graph(g_large, np.arange(G.N_FRAMES), current_frame_id=G.CURRENT_FRAME_ID),
        "g_weights": lambda s: [s.map_graph_weights(g_large, G.NAMES["H"]).tobytes()],
        "g_weights_small": lambda s: [s.map_graph_weights(g_small, 3).tobytes()],
    }
    fresh = {}
    for name, call in calls.items():
        with Solver(0) as s:
            fresh[name] = call(s)
    order = ("mp_small", "mp_large", "mp_small", "mp_dist", "assoc", "mp_large_no_desc", "mp_small",
             "icp_small", "icp_large", "icp_nn", "icp_small", "g_small", "g_weights_small", "g_large", "g_weights",
             "g_small", "mp_large", "icp_large", "assoc", "g_large", "icp_nn", "mp_dist")
    assert set(order) == set(calls)
    with Solver(0) as reused:
        for name in order:
            assert calls[name](reused) == fresh[name], name
