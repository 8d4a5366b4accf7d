"""References for ba_match_descriptors (include/ba_hip.h), in numpy.

1. A bit-exact float32 restatement of the pinned formulas (csrc/ba_match.h).
   fmaf is emulated exactly: the product of two float32 values is exact in
   float64 (48 significant bits); the float64 sum with the addend is rounded
   once, and its rounding error, obtained by TwoSum, decides the only case in
   which rounding that sum to float32 differs from rounding the exact value:
   a float64 sum that is exactly the midpoint of two adjacent float32 values.
2. A float64 brute-force matcher (true squared distances), the semantic
   cross-check of the first.

The scene generator makes unit-norm float32 descriptors at full precision (on
a coarse grid every partial sum would be exact and a wrong chain order would
go unnoticed)."""
from __future__ import annotations

import functools

import numpy as np

F32, F64 = np.float32, np.float64
MATCH_DTYPE = np.dtype([("query", np.int32), ("train", np.int32), ("distance", np.float32),
                        ("second_distance", np.float32), ("ref_distance", np.float32)])
KNN_DTYPE = np.dtype([("idx0", np.int32), ("idx1", np.int32), ("d2_0", np.float32), ("d2_1", np.float32)])
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---------------------------------------------------------------------------
# float32 restatement
# ---------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, exactly (finite values, no overflow)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    p = a.astype(F64) * b.astype(F64)                 # exact
    c64 = c.astype(F64)
    s = p + c64                                       # rounded once
    bb = s - p
    e = (p - (s - bb)) + (c64 - bb)                   # TwoSum: p + c == s + e exactly
    r = s.astype(F32)                                 # round to nearest even of s
    d = s - r.astype(F64)                             # exact
    other = np.nextafter(r, np.where(d > 0, F32(np.inf), F32(-np.inf)).astype(F32))
    tie = (d != 0) & ((s - r.astype(F64)) == (other.astype(F64) - s)) & np.isfinite(other)
    away = tie & (e != 0) & (np.sign(e) == np.sign(d))    # the exact value lies on other's side of the midpoint
    back = tie & (e != 0) & (np.sign(e) != np.sign(d))    # ... on r's side (r may have been the even choice or not)
    # s.astype picked the even neighbour at the tie; the exact value decides instead
    lo_hi = np.where(away, other, r)
    return np.where(back, r, lo_hi).astype(F32)


def dot32(Q, T):
    """dot(q, t) of every row pair: the chain acc = fmaf(q_k, t_k, acc), k ascending from 0."""
    Q, T = np.asarray(Q, F32), np.asarray(T, F32)
    acc = np.zeros((Q.shape[0], T.shape[0]), F32)
    for k in range(Q.shape[1]):
        acc = fma32(Q[:, k, None], T[None, :, k], acc)
    return acc


def nrm32(X):
    X = np.asarray(X, F32)
    acc = np.zeros(X.shape[0], F32)
    for k in range(X.shape[1]):
        acc = fma32(X[:, k], X[:, k], acc)
    return acc


def d2_from(dot, nq, nt):
    s = (nq.astype(F32)[:, None] + nt.astype(F32)[None, :]).astype(F32)
    x = fma32(F32(-2.0), dot, s)
    return np.where(x > 0, x, F32(0.0)).astype(F32)


def d2_32(Q, T):
    return d2_from(dot32(Q, T), nrm32(Q), nrm32(T))


def sqrt32(d2):
    return np.sqrt(np.asarray(d2, F32).astype(F64)).astype(F32)


def knn_of(d2):
    """The dense 2-NN records of a (nq, nt) matrix of non-negative distances
    (float32 or float64): the two smallest (value, index) per row."""
    nq, nt = d2.shape
    out = np.zeros(nq, KNN_DTYPE)
    out["idx0"] = out["idx1"] = -1
    out["d2_0"] = out["d2_1"] = np.inf
    if nt == 0:
        return out, np.full((nq, 2), np.inf)
    order = np.lexsort((np.broadcast_to(np.arange(nt), d2.shape), d2), axis=1)[:, :2]    # by value, then index
    val = np.take_along_axis(d2, order, axis=1)
    out["idx0"], out["d2_0"] = order[:, 0], val[:, 0]
    if nt > 1:
        out["idx1"], out["d2_1"] = order[:, 1], val[:, 1]
    full = np.full((nq, 2), np.inf)
    full[:, :val.shape[1]] = val
    return out, full


def select(knn, dist0, dist1, ratio, unique, max_distance, key0):
    """Ratio test, distance cap and the unique-train filter on dense records.
    dist0 / dist1: the two distances; key0: what orders the queries of one
    train row (the smaller wins).  Returns (query, train) in (train, query)
    order."""
    surv = (knn["idx1"] >= 0) & (dist0 < ratio * dist1) & (dist0 <= max_distance)
    q = np.nonzero(surv)[0]
    t = knn["idx0"][q]
    if unique:
        order = np.lexsort((q, key0[q], t))            # by train, then key, then query
        q, t = q[order], t[order]
        keep = np.ones(q.size, bool)
        keep[1:] = t[1:] != t[:-1]
        q, t = q[keep], t[keep]
    order = np.lexsort((q, t))
    return q[order].astype(np.int32), t[order].astype(np.int32)


def match32(Q, T, ratio=0.7, unique=1, max_distance=np.inf, row_ref=None, ref_desc=None, d2=None):
    """The pinned matcher in float32: (dense records, matches)."""
    Q, T = np.asarray(Q, F32), np.asarray(T, F32)
    if d2 is None:
        d2 = d2_32(Q, T)
    knn, _ = knn_of(d2)
    d0, d1 = sqrt32(knn["d2_0"]), sqrt32(knn["d2_1"])
    # float32 operands: ratio * d1 is a float product, rounded once; the bit pattern of d2_0 orders the queries
    q, t = select(knn, d0, np.where(knn["idx1"] >= 0, d1, F32(0.0)), F32(ratio), unique, F32(max_distance),
                  np.ascontiguousarray(knn["d2_0"]).view(np.uint32).astype(np.int64))
    m = np.zeros(q.size, MATCH_DTYPE)
    m["query"], m["train"] = q, t
    m["distance"], m["second_distance"] = d0[q], d1[q]
    m["ref_distance"] = -1.0
    if row_ref is not None and q.size:
        rr = np.asarray(row_ref)[q]
        has = rr >= 0
        if has.any():
            Tr, Rr = T[t[has]], np.asarray(ref_desc, F32)[rr[has]]
            acc = np.zeros(Tr.shape[0], F32)
            for k in range(T.shape[1]):
                acc = fma32(Tr[:, k], Rr[:, k], acc)
            s = (nrm32(Tr) + nrm32(Rr)).astype(F32)
            x = fma32(F32(-2.0), acc, s)
            m["ref_distance"][has] = sqrt32(np.where(x > 0, x, F32(0.0)))
    return knn, m


# ---------------------------------------------------------------------------
# float64 brute force
# ---------------------------------------------------------------------------
def d2_64(Q, T):
    Q, T = np.asarray(Q, F64), np.asarray(T, F64)
    return ((Q[:, None, :] - T[None, :, :]) ** 2).sum(axis=2)


def match64(Q, T, ratio=0.7, unique=1, max_distance=np.inf):
    """(dense records with float64 distances as (nq, 3) sorted values, (query, train) pairs)."""
    d2 = d2_64(Q, T)
    knn, _ = knn_of(d2)
    srt = np.sort(d2, axis=1)[:, :3]
    d0 = np.sqrt(srt[:, 0]) if d2.shape[1] > 0 else np.zeros(d2.shape[0])
    d1 = np.sqrt(srt[:, 1]) if d2.shape[1] > 1 else np.zeros(d2.shape[0])
    q, t = select(knn, d0, d1, ratio, unique, max_distance, srt[:, 0] if d2.shape[1] > 0 else d0)
    return knn, srt, q, t


# ---------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------
def unit_rows(rng, n, dim):
    x = rng.standard_normal((n, dim))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(F32)


def renorm(x):
    x = np.asarray(x, F64)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F32)


class Scene:
    def __init__(self, nq, nt, dim, seed):
        rng = np.random.default_rng(seed)
        self.nq, self.nt, self.dim, self.seed = nq, nt, dim, seed
        Q, T = unit_rows(rng, nq, dim), unit_rows(rng, nt, dim)
        small = min(nq, nt)
        n_match = int(0.6 * small)
        qi = rng.permutation(nq)[:n_match]
        ti = rng.permutation(nt)[:n_match]
        if n_match:                                     # the train row is the query plus sigma = 0.02 noise
            T[ti] = renorm(Q[qi].astype(F64) + 0.02 * rng.standard_normal((n_match, dim)))
        # near-duplicates of matched queries, on rows that were distractors: train collisions
        free = np.setdiff1d(np.arange(nq), qi)
        n_dup = min(3, n_match, free.size)
        self.dup = [(int(free[k]), int(qi[k])) for k in range(n_dup)]
        for dst, src in self.dup:
            Q[dst] = renorm(Q[src:src + 1].astype(F64) + 0.005 * rng.standard_normal((1, dim)))[0]
        self.Q, self.T = np.ascontiguousarray(Q), np.ascontiguousarray(T)
        self.truth = dict(zip(qi.tolist(), ti.tolist()))
        # every third query carries a reference descriptor: its own, perturbed
        self.row_ref = np.full(nq, -1, np.int32)
        idx = np.arange(0, nq, 3)
        self.row_ref[idx] = np.arange(idx.size)
        self.ref_desc = (renorm(Q[idx].astype(F64) + 0.01 * rng.standard_normal((idx.size, dim)))
                         if idx.size else np.zeros((0, dim), F32))


# (n_q, n_t, dim): the tile edges, one tile +- 1, several tiles, train chunks
CPU_SHAPES = [(2, 2, 64), (63, 65, 64), (65, 63, 64), (64, 64, 64), (257, 130, 64), (130, 257, 128), (1, 5, 64)]
GPU_SHAPES = [(2, 2, 64), (1, 5, 64), (5, 1, 64), (0, 7, 64), (63, 65, 64), (65, 63, 64), (64, 64, 64),
              (257, 130, 64), (130, 257, 128), (600, 700, 64)]
# Seeds: the first of 0, 1, 2, .. whose scene meets the conditions that
# tests/test_match_cpu.py asserts on the scene (float64 gaps and ratio margin)
SEEDS = {(257, 130, 64): 1}


def seed_of(shape):
    return SEEDS.get(tuple(shape), 0)


@functools.lru_cache(maxsize=None)
def scene(nq, nt, dim):
    return Scene(nq, nt, dim, 1000 * seed_of((nq, nt, dim)) + 7 * nq + 3 * nt + dim)


@functools.lru_cache(maxsize=None)
def scene_d2_32(nq, nt, dim):
    """The float32 distance matrix of a scene (computed once, never modified)."""
    sc = scene(nq, nt, dim)
    d2 = d2_32(sc.Q, sc.T)
    d2.setflags(write=False)
    return d2


def tie_scene():
    """The 64 x 64 scene with a planted train row repeated exactly at the end:
    (Q, T, the row's index, the index of its copy)."""
    sc = scene(64, 64, 64)
    t = min(sc.truth.values())
    return sc.Q, np.ascontiguousarray(np.concatenate([sc.T, sc.T[t:t + 1]])), t, sc.T.shape[0]


def scene_margins(sc):
    """(smallest float64 gap d2_1 - d2_0 or d2_2 - d2_1 over the queries,
    smallest ratio margin |d_0 / d_1 - 0.7|, train collisions among the ratio
    survivors): what a float32 matcher needs to reproduce the float64 one."""
    srt = np.sort(d2_64(sc.Q, sc.T), axis=1)[:, :3]
    gap = float(np.min(np.diff(srt, axis=1))) if srt.shape[1] > 1 and srt.shape[0] else np.inf
    if srt.shape[1] < 2 or not srt.shape[0]:
        return gap, np.inf, 0
    r = np.sqrt(srt[:, 0]) / np.sqrt(srt[:, 1])
    _, _, q, t = match64(sc.Q, sc.T, unique=0)
    return gap, float(np.min(np.abs(r - 0.7))), int(q.size - np.unique(t).size)


def d2_bound(dim):
    """|d2_f32 - d2_f64| for unit-norm rows: the fma chains of dot and of the
    two norms carry at most dim roundings of relative size 2^-24 each on sums
    of magnitude <= 1 (sum |q_k t_k| <= 1), the sum of the norms and the final
    fma three more: 4 (dim + 3) 2^-24 covers -2 dot + nrm + nrm."""
    return 4.0 * (dim + 3) * 2.0 ** -24
