"""GPU tests for ba_match_descriptors / ba_match_knn: the device equals the
float32 restatement of the pinned formulas (tests/match_ref.py, itself checked
against the host program and a float64 matcher in test_match_cpu.py) bit for
bit, at the tile edges, across train chunks and whatever the batching; ties
and train collisions resolve as pinned; the other entries are untouched."""
from functools import lru_cache

import numpy as np
import pytest

import match_ref as R
from bundleadjustment_amd import Options, Solver, make_synthetic, pack_match_batch
from bundleadjustment_amd import _native as N
from bundleadjustment_amd._native import BAError

pytestmark = pytest.mark.gpu

F32 = np.float32
OPTIONS = ((0.7, 1, np.inf), (0.7, 0, np.inf), (0.9, 1, np.inf), (0.9, 0, 0.25))


@pytest.fixture(scope="module")
def solver():
    s = Solver(0)
    yield s
    s.close()


def same_bits(a, b) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def pair_of(sc):
    return pack_match_batch([sc.Q, sc.T], [(0, 1)], row_ref=[sc.row_ref, None], ref_desc=sc.ref_desc, dim=sc.dim)


@lru_cache(maxsize=None)
def device_single(shape, ratio=0.7, unique=1, max_distance=np.inf):
    """One pair alone on a fresh context (read-only afterwards)."""
    with Solver(0) as s:
        off, m = s.match_descriptors(pair_of(R.scene(*shape)), ratio=ratio, unique=unique, max_distance=max_distance)
    m.setflags(write=False)
    return off, m


# ---------------------------------------------------------------------------
# 1. the dense 2-NN: the chain order of the contraction
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.GPU_SHAPES)
def test_knn_equals_the_float32_restatement(solver, shape):
    sc = R.scene(*shape)
    got = solver.match_knn(pair_of(sc), pair=0)
    want, _ = R.knn_of(R.scene_d2_32(*shape))
    assert got.shape == (shape[0],)
    bad = np.nonzero((got["idx0"] != want["idx0"]) | (got["idx1"] != want["idx1"]) |
                     (got["d2_0"].view(np.uint32) != want["d2_0"].view(np.uint32)) |
                     (got["d2_1"].view(np.uint32) != want["d2_1"].view(np.uint32)))[0]
    print(f"{shape}: {bad.size} of {shape[0]} dense records differ")
    assert bad.size == 0, (got[bad[:4]], want[bad[:4]])
    assert same_bits(got, want)


# ---------------------------------------------------------------------------
# 2. matches: ratio, cap, unique filter, collisions, reference distances
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.GPU_SHAPES)
def test_matches_equal_the_float32_restatement(solver, shape):
    sc = R.scene(*shape)
    d2 = R.scene_d2_32(*shape)
    for ratio, unique, maxd in OPTIONS:
        off, m = solver.match_descriptors(pair_of(sc), ratio=ratio, unique=unique, max_distance=maxd)
        _, want = R.match32(sc.Q, sc.T, ratio, unique, maxd, sc.row_ref, sc.ref_desc, d2=d2)
        assert off.tolist() == [0, want.size], (ratio, unique, maxd)
        assert same_bits(m, want), (ratio, unique, maxd)
        key = m["train"].astype(np.int64) * (1 << 32) + m["query"]
        assert np.all(np.diff(key) > 0)                                   # increasing (train, query)
        if unique:
            assert np.unique(m["train"]).size == m.size
        if shape[0] == 0 or shape[1] < 2:                                 # fewer than two train rows: no matches
            assert m.size == 0
    if shape[0] >= 63:      # the scene's collisions and references were exercised
        _, all_m = solver.match_descriptors(pair_of(sc), unique=0)
        assert all_m.size - np.unique(all_m["train"]).size == 3 and np.any(all_m["ref_distance"] >= 0)


def test_a_set_against_itself(solver):
    sc = R.scene(257, 130, 64)
    got = solver.match_knn([sc.Q], [(0, 0)])
    assert np.array_equal(got["idx0"], np.arange(257)) and np.all(got["d2_0"].view(np.uint32) == 0)
    assert np.all(got["idx1"] != got["idx0"]) and np.all(got["d2_1"] > 0)


def test_an_exact_tie_goes_to_the_lower_train_index(solver):
    Q, T, t, copy = R.tie_scene()
    knn = solver.match_knn([Q, T], [(0, 1)])
    hit = knn["idx0"] == t
    assert hit.any() and not np.any(knn["idx0"] == copy)
    assert np.all(knn["idx1"][hit] == copy)
    assert np.array_equal(knn["d2_1"][hit].view(np.uint32), knn["d2_0"][hit].view(np.uint32))
    _, m = solver.match_descriptors([Q, T], [(0, 1)], unique=0, ratio=0.999)
    assert not np.isin(np.nonzero(hit)[0], m["query"]).any()             # d0 < ratio * d1 fails at d0 == d1
    assert same_bits(knn, R.knn_of(R.d2_32(Q, T))[0])


# ---------------------------------------------------------------------------
# 3. batching and the grid split do not matter
# ---------------------------------------------------------------------------
def test_mixed_batch_equals_the_single_pairs(solver):
    shapes = [s for s in R.GPU_SHAPES if s[2] == 64]
    sets, pairs, row_ref, refs, n_ref = [], [], [], [], 0
    for shp in shapes:
        sc = R.scene(*shp)
        pairs.append((len(sets), len(sets) + 1))
        sets += [sc.Q, sc.T]
        row_ref += [np.where(sc.row_ref >= 0, sc.row_ref + n_ref, -1), None]
        refs.append(sc.ref_desc)
        n_ref += sc.ref_desc.shape[0]
    empty = len(sets)
    sets.append(np.zeros((0, 64), F32))
    row_ref.append(None)
    big_q = 2 * shapes.index((600, 700, 64))
    extra = [(big_q, 2 * shapes.index((257, 130, 64)) + 1), (big_q, 2 * shapes.index((64, 64, 64)) + 1),
             (big_q + 1, big_q), (empty, big_q), (big_q, empty), (empty, empty)]
    mb = pack_match_batch(sets, pairs + extra, row_ref=row_ref, ref_desc=np.concatenate(refs), dim=64)
    for ratio, unique, maxd in OPTIONS[:2]:
        off, m = solver.match_descriptors(mb, ratio=ratio, unique=unique, max_distance=maxd)
        assert off.size == len(pairs) + len(extra) + 1 and off[-1] == m.size
        for i, shp in enumerate(shapes):
            _, want = device_single(shp, ratio, unique, maxd)
            assert same_bits(m[off[i]:off[i + 1]], want), (shp, unique)
        for k, (q, t) in enumerate(extra):
            i = len(pairs) + k
            _, want = R.match32(sets[q], sets[t], ratio, unique, maxd, row_ref[q], mb.ref_desc)
            assert same_bits(m[off[i]:off[i + 1]], want), (q, t, unique)
    for i in (len(pairs), len(pairs) + 3, len(pairs) + 4):      # the dense records of a pair inside a batch
        q, t = (pairs + extra)[i]
        assert same_bits(solver.match_knn(mb, pair=i), R.knn_of(R.d2_32(sets[q], sets[t]))[0])


def test_dim_128_batch_both_directions(solver):
    sc = R.scene(130, 257, 128)
    mb = pack_match_batch([sc.Q, sc.T, np.zeros((0, 128), F32)], [(0, 1), (1, 0), (2, 1), (0, 1)],
                          row_ref=[sc.row_ref, None, None], ref_desc=sc.ref_desc)
    off, m = solver.match_descriptors(mb)
    _, want = device_single((130, 257, 128))
    assert same_bits(m[off[0]:off[1]], want) and same_bits(m[off[3]:off[4]], want) and off[2] == off[3]
    _, back = R.match32(sc.T, sc.Q)
    assert same_bits(m[off[1]:off[2]], back)


# ---------------------------------------------------------------------------
# 4. context and staging
# ---------------------------------------------------------------------------
def test_solve_is_untouched_by_a_match_call_in_between(solver):
    p = make_synthetic(6, 300, 4, seed=31)
    mb = pair_of(R.scene(65, 63, 64))
    fields = ["iteration", "step_is_valid", "step_is_successful", "cost", "cost_change", "gradient_max_norm",
              "gradient_norm", "step_norm", "relative_decrease", "trust_region_radius", "model_cost_change"]

    def solve(between):
        solver.set_problem(p)
        if between:
            solver.match_descriptors(mb)
        solver.solve(Options(max_num_iterations=6))
        if between:
            solver.match_knn(mb)
        cams, pts = solver.params()
        return [[r[f] for f in fields] for r in solver.iteration_log()], cams, pts

    log0, c0, x0 = solve(False)
    log1, c1, x1 = solve(True)
    assert log0 == log1 and c0.tobytes() == c1.tobytes() and x0.tobytes() == x1.tobytes()
    solver.solve(Options(max_num_iterations=6))
    ref = solver.params()
    solver.set_problem(p)
    solver.solve(Options(max_num_iterations=6))
    solver.match_descriptors(mb)
    solver.solve(Options(max_num_iterations=6))
    again = solver.params()
    assert ref[0].tobytes() == again[0].tobytes() and ref[1].tobytes() == again[1].tobytes()


def test_staging_arenas_interleave_bitwise():
    """One context through match small -> large -> small interleaved with a
    two-view call, a PnP call and the inspection entry: every result equals,
    bit for bit, the same call on a fresh context."""
    import pnp_ref as P
    import two_view_ref as TV

    small, large = pair_of(R.scene(63, 65, 64)), pair_of(R.scene(600, 700, 64))
    tsc = TV.e2e_scene(65, 0.3, False)
    tvb = (np.array([0, len(tsc.uv1)], np.int32), tsc.K.astype(F32).reshape(1, 9), None,
           tsc.uv1.astype(F32).reshape(-1, 2), tsc.uv2.astype(F32).reshape(-1, 2))
    ps = P.scene(64, 0.3, 0.5, 75)
    pb = (np.array([0, 64], np.int32), ps.cam[None], ps.K[None], ps.pts, ps.uv)

    def match(mb, **kw):
        def call(s):
            off, m = s.match_descriptors(mb, **kw)
            return [off.tobytes(), m.tobytes()]
        return call

    def tv(s):
        inl, res = s.two_view_ransac(*tvb, min_good=8, max_hypotheses=65)
        return [inl.tobytes(), res[0].status, res[0].cam.tobytes(), res[0].E.tobytes(), res[0].votes_e]

    def pnp(s):
        cams, inl, res = s.pnp_ransac(*pb, options=Options(max_num_iterations=10))
        return [cams.tobytes(), inl.tobytes(), res[0].status, res[0].best_hypothesis]

    def knn(s):
        return [s.match_knn(large).tobytes()]

    calls = {"small": match(small), "large": match(large, unique=0), "tv": tv, "pnp": pnp, "knn": knn}
    fresh = {}
    for name, call in calls.items():
        with Solver(0) as s:
            fresh[name] = call(s)
    with Solver(0) as reused:
        for name in ("small", "large", "small", "tv", "knn", "large", "pnp", "small", "tv"):
            assert calls[name](reused) == fresh[name], name


def test_times_of_the_last_call(solver):
    solver.match_descriptors(pair_of(R.scene(257, 130, 64)))
    ms = solver.match_times()
    assert ms.shape == (6,) and np.all(ms >= 0) and ms[2] >= ms[0]
    assert abs(ms[3] + ms[4] + ms[5] - ms[1]) <= 1e-3 * max(ms[1], 1.0)


# ---------------------------------------------------------------------------
# 5. errors
# ---------------------------------------------------------------------------
def test_errors_leave_the_context_usable(solver):
    sc = R.scene(63, 65, 64)
    good = pair_of(sc)
    _, want = device_single((63, 65, 64))

    def refused(mb, what, **kw):
        with pytest.raises(BAError) as e:
            solver.match_descriptors(mb, **kw)
        assert e.value.status == 1 and what in str(e.value), str(e.value)
        with pytest.raises(BAError) as e:
            solver.match_knn(mb)
        assert e.value.status == 1

    rng = np.random.default_rng(5)
    refused(pack_match_batch([R.unit_rows(rng, 4, 32), R.unit_rows(rng, 4, 32)], [(0, 1)]), "dim 32")
    for pairs in ([(0, 2)], [(2, 0)], [(-1, 0)]):
        refused(pack_match_batch([sc.Q, sc.T], pairs), "out of range")
    dec = pack_match_batch([sc.Q, sc.T], [(0, 1)])
    dec.set_offset = np.array([0, 70, 63], np.int32)
    refused(dec, "decreases at set 1")
    bad_ref = pair_of(sc)
    bad_ref.row_ref = bad_ref.row_ref.copy()
    bad_ref.row_ref[3] = sc.ref_desc.shape[0]
    refused(bad_ref, "row_ref[3]")
    for kw, what in ((dict(ratio=-1.0), "ratio"), (dict(ratio=np.inf), "ratio"), (dict(max_distance=np.nan), "max_distance"),
                     (dict(unique=2), "unique")):
        with pytest.raises(BAError) as e:
            solver.match_descriptors(good, **kw)
        assert e.value.status == 1 and what in str(e.value)
    with pytest.raises(BAError) as e:
        solver.match_knn(good, pair=1)
    assert e.value.status == 1 and "pair 1" in str(e.value)
    with pytest.raises(TypeError):
        solver.match_descriptors(good, cross_check=1)
    off, m = solver.match_descriptors(good)                              # a valid call afterwards
    assert same_bits(m, want)
    off, m = solver.match_descriptors(pack_match_batch([], np.zeros((0, 2), np.int32), dim=64))
    assert off.tolist() == [0] and m.size == 0                           # an empty batch is valid


# ---------------------------------------------------------------------------
# 6. composition: descriptors -> matches -> relative pose
# ---------------------------------------------------------------------------
def test_composition_with_two_view_ransac(solver):
    import two_view_ref as TV

    sc = TV.e2e_scene(200, 0.0, False)
    n = len(sc.uv1)
    rng = np.random.default_rng(77)
    base = R.unit_rows(rng, n, 64).astype(np.float64)
    d1 = R.renorm(base + 0.02 * rng.standard_normal((n, 64)))            # view 1: keypoint i sees point i
    perm = rng.permutation(n)                                            # view 2: keypoint j sees point perm[j]
    d2 = R.renorm(base[perm] + 0.02 * rng.standard_normal((n, 64)))
    uv1, uv2 = np.asarray(sc.uv1, F32).reshape(-1, 2), np.asarray(sc.uv2, F32).reshape(-1, 2)[perm]
    off, m = solver.match_descriptors([d1, d2], [(0, 1)])
    assert m.size == n and np.array_equal(perm[m["train"]], m["query"])  # every point found, none wrong
    inl, res = solver.two_view_ransac(np.array([0, m.size], np.int32), np.asarray(sc.K, F32).reshape(1, 9), None,
                                      uv1[m["query"]], uv2[m["train"]], e_solver=N.TV_E_FIVE_POINT)
    assert res[0].status == N.TV_OK and res[0].model == N.TV_ESSENTIAL and inl.sum() >= 0.9 * n
