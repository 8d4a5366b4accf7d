"""GPU tests for ba_map_points_update / ba_map_points_distances / ba_associate:
the device equals the float32 restatement of the pinned formulas
(tests/map_points_ref.py, itself checked against the host program and float64
in test_map_points_cpu.py) bit for bit at every track length (both sides of
every tier boundary), under both median rules and whatever the batching; ties
resolve as pinned; the association gates flip one float either side of their
thresholds; the other entries are untouched."""
import dataclasses

import numpy as np
import pytest

import map_points_ref as M
import match_ref as R
from bundleadjustment_amd import Options, Solver, make_synthetic, pack_match_batch
from bundleadjustment_amd import _native as N
from bundleadjustment_amd._native import BAError

pytestmark = pytest.mark.gpu

F32 = np.float32
RULES = (M.REFERENCE, M.FLOAT)


@pytest.fixture(scope="module")
def solver():
    s = Solver(0)
    yield s
    s.close()


def same_bits(a, b) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def differing(got, want):
    return [p for p in range(want.size) if got[p].tobytes() != want[p].tobytes()]


# ---------------------------------------------------------------------------
# 1. records, chosen descriptors, D and m at every track length
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [64, 128])
def test_update_equals_the_float32_restatement(solver, dim):
    sc, parts = M.scene(dim), M.scene_parts(dim)
    n = sc.lengths()
    assert set(n.tolist()) >= set(M.LENGTHS if dim == 64 else M.LENGTHS_128) and np.count_nonzero(sc.ref_obs) >= n.size // 3
    for rule in RULES:
        got, desc = solver.map_points_update(sc.batch, median_rule=rule)
        want, want_desc = M.update32(sc.batch, rule, parts)
        bad = differing(got, want)
        print(f"dim {dim} rule {rule}: {len(bad)} of {n.size} records differ (lengths {sorted(set(n[bad].tolist()))})")
        assert not bad, (got[bad[:3]], want[bad[:3]])
        assert same_bits(got, want) and same_bits(desc, want_desc)
        only, none = solver.map_points_update(sc.batch, want_desc=False, median_rule=rule)
        assert same_bits(only, want) and none is None
    empty = n == 0
    assert empty.any() and np.all(got["status"][empty] == N.MP_EMPTY) and np.all(got["best"][empty] == -1)
    for f in ("median", "view_dir", "min_dist", "max_dist"):
        assert not got[f][empty].view(np.uint32).any(), f
    assert not desc[empty].view(np.uint32).any()
    # the reference rule is exercised beyond "index 0": coarse rows have truncated medians that differ
    ref, _ = solver.map_points_update(sc.batch)                       # the default rule
    coarse = np.array([k == "coarse" for k in sc.kind])
    assert same_bits(ref, M.update32(sc.batch, M.REFERENCE, parts)[0])
    assert np.count_nonzero(ref["best"][coarse] > 0) >= 3 and np.all(ref["best"][~coarse & ~empty] == 0)
    assert np.any(ref["best"] != got["best"])


@pytest.mark.parametrize("dim", [64, 128])
def test_distances_and_medians_equal_the_restatement(solver, dim):
    sc, parts = M.scene(dim), M.scene_parts(dim)
    for p, n in enumerate(sc.lengths()):
        D, m = solver.map_points_distances(sc.batch, p)
        assert D.shape == (n, n) and m.shape == (n,)
        assert same_bits(D, parts[p][0]), ("D", p, n, int(np.count_nonzero(D.view(np.uint32) != parts[p][0].view(np.uint32))))
        assert same_bits(m, parts[p][1]), ("m", p, n)
        assert same_bits(D, np.ascontiguousarray(D.T)) and np.all(np.diag(D).view(np.uint32) == 0)
        if n == 8:                                        # this track names one row twice
            assert D[5, 2].view(np.uint32) == 0


def test_ties_at_four_and_five_go_to_the_lower_index(solver):
    sc = M.scene(64)
    got, _ = solver.map_points_update(sc.batch, median_rule=M.FLOAT)
    seen = 0
    for p, n in enumerate(sc.lengths()):
        if n not in (4, 5):
            continue
        D, m = solver.map_points_distances(sc.batch, p)
        off = D + np.where(np.eye(n, dtype=bool), np.inf, 0).astype(F32)
        i, j = np.unravel_index(np.argmin(off), off.shape)
        assert i != j and m[i].view(np.uint32) == m[j].view(np.uint32) == off[i, j].view(np.uint32)
        assert got["best"][p] == min(i, j) and got["median"][p].view(np.uint32) == m[i].view(np.uint32)
        seen += 1
    assert seen >= 4


# ---------------------------------------------------------------------------
# 2. batching does not matter
# ---------------------------------------------------------------------------
def test_batch_independence(solver):
    sc = M.scene(64)
    n = sc.lengths()
    idx = list(range(n.size))
    for rule in RULES:
        whole, whole_desc = solver.map_points_update(sc.batch, median_rule=rule)
        again, again_desc = solver.map_points_update(sc.batch, median_rule=rule)
        assert same_bits(whole, again) and same_bits(whole_desc, again_desc)
        rev, rev_desc = solver.map_points_update(M.sub_batch(sc, idx[::-1]), median_rule=rule)
        assert same_bits(rev[::-1].copy(), whole) and same_bits(rev_desc[::-1].copy(), whole_desc)
        twice, twice_desc = solver.map_points_update(M.sub_batch(sc, idx + idx), median_rule=rule)
        assert same_bits(twice[:n.size].copy(), whole) and same_bits(twice[n.size:].copy(), whole)
        assert same_bits(twice_desc[n.size:].copy(), whole_desc)
    for p in idx:                                          # each point alone (the float rule is still set)
        one, one_desc = solver.map_points_update(M.sub_batch(sc, [p]), median_rule=M.FLOAT)
        assert one[0].tobytes() == whole[p].tobytes() and same_bits(one_desc[0], whole_desc[p]), (p, n[p])


def test_padding_another_track_across_a_tier_changes_nothing_else(solver):
    """A 16-track padded to 17 and a 64-track padded to 65 move to the next
    tier, which shifts every other point's place in the plan."""
    sc = M.scene(64)
    n = sc.lengths()
    idx = list(range(n.size))
    whole, whole_desc = solver.map_points_update(sc.batch, median_rule=M.FLOAT)
    a, b = int(np.nonzero(n == 16)[0][0]), int(np.nonzero(n == 64)[0][0])
    padded = M.sub_batch(sc, idx, pad={a: [sc.tracks[a][3]], b: [sc.tracks[b][7]]})
    got, desc = solver.map_points_update(padded, median_rule=M.FLOAT)
    keep = np.array([p not in (a, b) for p in idx])
    assert same_bits(got[keep], whole[keep]) and same_bits(desc[keep], whole_desc[keep])
    want, _ = M.update32(padded, M.FLOAT)
    assert got[a].tobytes() == want[a].tobytes() and got[b].tobytes() == want[b].tobytes()


# ---------------------------------------------------------------------------
# 3. ba_associate
# ---------------------------------------------------------------------------
def test_association_gates_one_float_either_side_of_each_threshold(solver):
    ab, want, fuse_want = M.edge_scene()
    items, fuse = solver.associate(ab)
    ri, rf = M.associate32(ab)
    assert set(want.tolist()) == set(range(9)) and fuse_want.tolist() == [N.FUSE_OK, N.FUSE_ANGLE, N.FUSE_DESC]
    assert ri["status"].tolist() == want.tolist() and rf["status"].tolist() == fuse_want.tolist()
    assert items["status"].tolist() == want.tolist() and fuse["status"].tolist() == fuse_want.tolist()
    assert same_bits(items, ri) and same_bits(fuse, rf)
    no_cur = dataclasses.replace(ab, item_cur_row=None, item_scale=np.ones(ab.item_cam.size, F32))
    items, _ = solver.associate(no_cur)
    assert same_bits(items, M.associate32(no_cur)[0]) and not np.isin(items["status"], (N.AS_REPLACE, N.AS_WORSE)).any()


def test_random_associations_fed_by_the_update(solver):
    sc = M.scene(64)
    rec, desc_out = solver.map_points_update(sc.batch, median_rule=M.FLOAT)
    ab = M.assoc_scene(sc.batch, rec, desc_out)             # view directions, depth bounds, descriptors: the device's own
    assert ab.item_cam.size == 300 and set(ab.item_cam.tolist()) == {0, 1, 2}
    items, fuse = solver.associate(ab)
    ri, rf = M.associate32(ab)
    print("statuses:", np.bincount(ri["status"], minlength=9).tolist(), "fuse:", np.bincount(rf["status"], minlength=3).tolist())
    assert set(ri["status"].tolist()) == set(range(9))
    bad = differing(items, ri)
    assert not bad, (items[bad[:3]], ri[bad[:3]])
    assert same_bits(items, ri) and same_bits(fuse, rf)
    options = dict(chi2=3.0, min_cos=0.8, max_desc_dist=1.5, fuse_min_cos=0.9, fuse_max_desc_dist=1.41)
    items, fuse = solver.associate(ab, **options)
    ri, rf = M.associate32(ab, **options)
    assert same_bits(items, ri) and same_bits(fuse, rf) and set(rf["status"].tolist()) == {0, 1, 2}
    again, fuse_again = solver.associate(ab, **options)
    assert same_bits(again, items) and same_bits(fuse_again, fuse)
    half = dataclasses.replace(ab, item_cam=ab.item_cam[150:], item_pt=ab.item_pt[150:], item_uv=ab.item_uv[150:],
                               item_scale=ab.item_scale[150:], item_row=ab.item_row[150:],
                               item_cur_row=ab.item_cur_row[150:], fuse_pairs=ab.fuse_pairs[::-1].copy())
    part, fuse_rev = solver.associate(half, **options)
    assert same_bits(part, items[150:].copy()) and same_bits(fuse_rev[::-1].copy(), fuse)


# ---------------------------------------------------------------------------
# 4. context and staging
# ---------------------------------------------------------------------------
def test_solve_and_match_are_untouched_by_the_calls_in_between(solver):
    p = make_synthetic(6, 300, 4, seed=31)
    sc = M.scene(64)
    small = M.sub_batch(sc, [q for q in range(sc.lengths().size) if sc.lengths()[q] <= 130])
    ab, _, _ = M.edge_scene()
    msc = R.scene(65, 63, 64)
    mb = pack_match_batch([msc.Q, msc.T], [(0, 1)], row_ref=[msc.row_ref, None], ref_desc=msc.ref_desc, dim=64)
    fields = ["iteration", "step_is_valid", "step_is_successful", "cost", "cost_change", "gradient_max_norm",
              "gradient_norm", "step_norm", "relative_decrease", "trust_region_radius", "model_cost_change"]

    def solve(between):
        solver.set_problem(p)
        if between:
            solver.map_points_update(small)
            solver.associate(ab)
        solver.solve(Options(max_num_iterations=6))
        if between:
            solver.map_points_distances(small, 0)
        cams, pts = solver.params()
        return [[r[f] for f in fields] for r in solver.iteration_log()], cams, pts

    log0, c0, x0 = solve(False)
    log1, c1, x1 = solve(True)
    assert log0 == log1 and c0.tobytes() == c1.tobytes() and x0.tobytes() == x1.tobytes()
    solver.solve(Options(max_num_iterations=6))
    ref = solver.params()
    solver.set_problem(p)
    solver.solve(Options(max_num_iterations=6))
    solver.map_points_update(small, median_rule=M.FLOAT)
    solver.associate(ab)
    solver.solve(Options(max_num_iterations=6))
    again = solver.params()
    assert ref[0].tobytes() == again[0].tobytes() and ref[1].tobytes() == again[1].tobytes()
    off0, m0 = solver.match_descriptors(mb)
    solver.map_points_update(small)
    solver.associate(ab)
    off1, m1 = solver.match_descriptors(mb)
    assert same_bits(off0, off1) and same_bits(m0, m1)


def test_times_of_the_last_call(solver):
    solver.map_points_update(M.scene(128).batch)
    ms = solver.map_points_times()
    assert ms.shape == (3,) and np.all(ms >= 0) and ms[2] >= ms[0] and ms[2] >= ms[1]


# ---------------------------------------------------------------------------
# 5. errors
# ---------------------------------------------------------------------------
def test_errors_leave_the_context_usable(solver):
    sc = M.scene(64)
    n = sc.lengths()
    good = M.sub_batch(sc, [p for p in range(n.size) if 0 < n[p] <= 17][:6])
    want, want_desc = solver.map_points_update(good)
    no = good.obs_cam.size

    def refused(what, mb=good, distances=True, **kw):
        with pytest.raises(BAError) as e:
            solver.map_points_update(mb, **kw)
        assert e.value.status == 1 and what in str(e.value), str(e.value)
        if distances and not kw:
            with pytest.raises(BAError) as e:
                solver.map_points_distances(mb, 0)
            assert e.value.status == 1 and what in str(e.value)

    def changed(**f):
        return dataclasses.replace(good, **{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in f.items()})

    def poke(name, at, value):
        a = getattr(good, name).copy()
        a[at] = value
        return changed(**{name: a})
    refused("dim 32 is neither 64 nor 128", changed(dim=32))
    refused("unknown median_rule 2", median_rule=2)
    for bad in (0.0, -2.0, np.inf, np.nan):
        refused("max_scale must be positive and finite", max_scale=bad)
    refused("reserved must be 0", reserved=1)
    refused("reserved must be 0", reserved_f=0.5)
    refused("obs_offset[0] != 0", poke("obs_offset", 0, 1))
    refused("obs_offset decreases at point 2", poke("obs_offset", 3, int(good.obs_offset[2]) - 1))
    refused(f"obs_cam[{no - 1}] out of range", poke("obs_cam", no - 1, M.N_CAMS))
    refused("obs_cam[0] out of range", poke("obs_cam", 0, -1))
    refused("obs_row[2] out of range", poke("obs_row", 2, good.desc.shape[0]))
    refused("ref_obs[1] out of range", poke("ref_obs", 1, int(np.diff(good.obs_offset)[1])))
    refused("null array", changed(obs_row=None))
    long = int(np.argmax(n))
    refused("point 0 has a track of 1025 observations, more than 1024", M.sub_batch(sc, [long], pad={0: [sc.tracks[long][0]]}))
    with pytest.raises(BAError) as e:
        solver.map_points_distances(good, 6)
    assert e.value.status == 1 and "point 6 out of range" in str(e.value)
    with pytest.raises(TypeError):
        solver.map_points_update(good, median="float")

    ab, _, _ = M.edge_scene()
    items_want, fuse_want = solver.associate(ab)

    def refused_assoc(what, batch=ab, **kw):
        with pytest.raises(BAError) as e:
            solver.associate(batch, **kw)
        assert e.value.status == 1 and what in str(e.value), str(e.value)

    def poke_assoc(name, at, value):
        a = getattr(ab, name).copy()
        a[at] = value
        return dataclasses.replace(ab, **{name: a})
    refused_assoc("dim 32", dataclasses.replace(ab, dim=32))
    refused_assoc("reserved must be 0", reserved=1)
    for name, bad in (("item_cam", 1), ("item_pt", -1), ("item_pt", ab.pts.shape[0]), ("item_row", ab.desc.shape[0]),
                      ("item_cur_row", -2), ("item_cur_row", ab.desc.shape[0])):
        refused_assoc(f"{name}[5] out of range", poke_assoc(name, 5, bad))
    refused_assoc("fuse_pairs[4] out of range (pair 2)", poke_assoc("fuse_pairs", (2, 0), ab.pts.shape[0]))
    refused_assoc("null array", dataclasses.replace(ab, item_uv=None))
    with pytest.raises(TypeError):
        solver.associate(ab, ratio=0.5)

    got, got_desc = solver.map_points_update(good)                        # valid calls afterwards
    assert same_bits(got, want) and same_bits(got_desc, want_desc)
    items, fuse = solver.associate(ab)
    assert same_bits(items, items_want) and same_bits(fuse, fuse_want)
    none = M.sub_batch(sc, [])                                            # empty batches are valid
    rec, desc = solver.map_points_update(none)
    assert rec.size == 0 and desc.shape == (0, 64)
    empty = dataclasses.replace(ab, item_cam=ab.item_cam[:0], item_pt=ab.item_pt[:0], item_uv=ab.item_uv[:0],
                                item_row=ab.item_row[:0], item_cur_row=ab.item_cur_row[:0], fuse_pairs=ab.fuse_pairs[:0])
    items, fuse = solver.associate(empty)
    assert items.size == 0 and fuse.size == 0
