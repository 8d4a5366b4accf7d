"""numpy restatement of ba_icp (include/ba_hip.h; csrc/ba_icp.h is the device's
text): the float32 key-minimum nearest neighbour by brute force, the fp64
Umeyama step, the loop with PCL's convergence rules, the fitness, and the
normalisation of the reference's reconstruction error; and the scenes the
tests run on.  Nothing here is shared with the library."""
from types import SimpleNamespace

import numpy as np

f32 = np.float32
DBL_MAX = float(np.finfo(np.float64).max)
FLT_MAX = float(np.finfo(np.float32).max)
NOT_CONVERGED, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, NO_CORRESPONDENCES = range(6)
DEFAULTS = dict(max_iterations=10, max_corr_dist=np.inf, mse_abs_eps=1e-12, mse_rel_eps=0.0, transformation_eps=0.0,
                min_correspondences=3, with_scale=0, fitness_max_range=np.inf)


# ---------------------------------------------------------------------------
# correspondences
# ---------------------------------------------------------------------------
def d2_matrix(src, tgt):
    """d2[i, j] = ((dx*dx + dy*dy) + dz*dz) in float32, every operation rounded on its own."""
    s, t = np.asarray(src, f32), np.asarray(tgt, f32)
    dx = s[:, None, 0] - t[None, :, 0]
    dy = s[:, None, 1] - t[None, :, 1]
    dz = s[:, None, 2] - t[None, :, 2]
    return ((dx * dx + dy * dy) + dz * dz).astype(f32)


def nn_brute(src, tgt, gate=np.inf, chunk=512):
    """Per source point the target index of smallest (bits(d2), j), and that d2;
    -1 and +inf where d2 > gate.  argmin takes the first minimum: the lowest index."""
    src = np.asarray(src, f32).reshape(-1, 3)
    idx = np.empty(src.shape[0], np.int32)
    d2 = np.empty(src.shape[0], f32)
    for a in range(0, src.shape[0], chunk):
        D = d2_matrix(src[a:a + chunk], tgt)
        j = np.argmin(D, axis=1)
        idx[a:a + chunk] = j
        d2[a:a + chunk] = D[np.arange(D.shape[0]), j]
    drop = ~(d2 <= f32(gate))
    idx[drop] = -1
    d2[drop] = np.inf
    return idx, d2


def second_gap(src, tgt):
    """The smallest difference between the best and the second-best d2 over the source."""
    D = np.sort(d2_matrix(src, tgt).astype(np.float64), axis=1)
    return float((D[:, 1] - D[:, 0]).min())


# ---------------------------------------------------------------------------
# the step
# ---------------------------------------------------------------------------
def box_centre(tgt):
    t = np.asarray(tgt, f32).astype(np.float64)
    return (0.5 * (t.min(axis=0) + t.max(axis=0))).astype(f32)


def estimate(cur, tgt, idx, with_scale=0):
    """(M = c R, t) as float32 from the kept pairs: Umeyama in fp64 about the target's box centre."""
    keep = idx >= 0
    c0 = box_centre(tgt).astype(np.float64)
    a = cur[keep].astype(np.float64) - c0
    b = np.asarray(tgt, f32)[idx[keep]].astype(np.float64) - c0
    n = a.shape[0]
    ma, mb = a.sum(axis=0) / n, b.sum(axis=0) / n
    H = b.T @ a - n * np.outer(mb, ma)
    U, s, Vt = np.linalg.svd(H)
    S = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt)) or 1.0])
    R = U @ S @ Vt
    c = 1.0
    if not np.all(np.isfinite(R)):
        R = np.eye(3)
    elif with_scale:
        var = (a * a).sum() - n * (ma @ ma)
        c = float(np.trace(np.diag(s) @ S)) / var
    t = (c0 + mb) - c * (R @ (c0 + ma))
    return (c * R).astype(f32), t.astype(f32)


def apply(M, t, cur):
    x, y, z = cur[:, 0], cur[:, 1], cur[:, 2]
    return np.stack([((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + t[r] for r in range(3)], axis=1).astype(f32)


def compose(M, t, fin):
    out = fin.copy()
    for i in range(3):
        for j in range(4):
            out[i, j] = ((M[i, 0] * fin[0, j] + M[i, 1] * fin[1, j]) + M[i, 2] * fin[2, j]) + t[i] * fin[3, j]
    return out.astype(f32)


def ulp_up(a):
    return np.nextafter(a, f32(np.inf)).astype(f32)


def icp(src, tgt, guess=None, perturb=False, **options):
    """The loop.  perturb: every step's float M and t are moved up by one ulp
    before they are used (the sensitivity of the result to the last bit of a
    step).  Returns a namespace: final, converged, state, iterations, n_corr,
    fitness, mse (max_iterations,), cur, idx (of the last pass)."""
    o = {**DEFAULTS, **options}
    src, tgt = np.asarray(src, f32).reshape(-1, 3), np.asarray(tgt, f32).reshape(-1, 3)
    fin = np.eye(4, dtype=f32) if guess is None else np.asarray(guess, f32).reshape(4, 4).copy()
    fin[3] = (0, 0, 0, 1)
    cur = apply(fin[:3, :3], fin[:3, 3], src)
    gate = f32(o["max_corr_dist"]) * f32(o["max_corr_dist"])
    mse_log = np.zeros(o["max_iterations"])
    state, converged, iterations, n_corr, prev = NOT_CONVERGED, 0, 0, 0, DBL_MAX
    idx = None
    while state == NOT_CONVERGED:
        idx, d2 = nn_brute(cur, tgt, gate)
        keep = idx >= 0
        n_corr = int(keep.sum())
        if n_corr < o["min_correspondences"]:
            state = NO_CORRESPONDENCES
            break
        M, t = estimate(cur, tgt, idx, o["with_scale"])
        if perturb:
            M, t = ulp_up(M), ulp_up(t)
        cur = apply(M, t, cur)
        fin = compose(M, t, fin)
        iterations += 1
        mse = float(d2[keep].astype(np.float64).sum() / n_corr)
        mse_log[iterations - 1] = mse
        cos_angle = 0.5 * (float(M[0, 0]) + float(M[1, 1]) + float(M[2, 2]) - 1.0)
        t2 = float((t.astype(np.float64) ** 2).sum())
        if iterations >= o["max_iterations"]:
            state = ITERATIONS
        elif cos_angle >= 1.0 - o["transformation_eps"] and t2 <= o["transformation_eps"]:
            state = TRANSFORM
        elif abs(mse - prev) < o["mse_abs_eps"]:
            state = ABS_MSE
        elif o["mse_rel_eps"] > 0 and abs(mse - prev) / prev < o["mse_rel_eps"]:
            state = REL_MSE
        else:
            prev = mse
        converged = int(state != NOT_CONVERGED)
    fitness = DBL_MAX
    if converged:
        idx, d2 = nn_brute(cur, tgt, o["fitness_max_range"])
        keep = idx >= 0
        if keep.any():
            fitness = float(d2[keep].astype(np.float64).sum() / keep.sum())
    return SimpleNamespace(final=fin, converged=converged, state=state, iterations=iterations, n_corr=n_corr,
                           fitness=fitness, mse=mse_log, cur=cur, idx=idx)


# ---------------------------------------------------------------------------
# the reference's normalisation (ReconstructionError.cpp:93-104)
# ---------------------------------------------------------------------------
def normalise(points, target, gt_pose0=None):
    src = np.asarray(points, f32).reshape(-1, 3)
    tgt = np.asarray(target, f32).reshape(-1, 3)
    if gt_pose0 is not None:
        inv = np.linalg.inv(np.asarray(gt_pose0, np.float64)).astype(f32)
        src = apply(inv[:3, :3], inv[:3, 3], src)
    src = src - src.astype(np.float64).mean(axis=0).astype(f32)
    tgt = tgt - tgt.astype(np.float64).mean(axis=0).astype(f32)
    ext = lambda c: f32((c.max(axis=0) - c.min(axis=0)).max())
    scale = f32(ext(tgt) / ext(src))
    return (src * scale).astype(f32), tgt.astype(f32), scale


def reconstruction_error(points, target, gt_pose0=None, **options):
    src, tgt, _ = normalise(points, target, gt_pose0)
    r = icp(src, tgt, **options)
    return (r.fitness if r.converged else FLT_MAX), r


# ---------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------
def rigid(deg, axis, t):
    """4x4 float64: a rotation by deg about axis, then the translation t."""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    a = np.deg2rad(deg)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    T[:3, 3] = t
    return T


def surface(rng, n):
    """n points of a bumpy closed surface (a star-shaped blob with unequal axes)."""
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    th, ph = np.arccos(v[:, 2]), np.arctan2(v[:, 1], v[:, 0])
    r = 1.0 + 0.15 * np.sin(3 * th) * np.cos(2 * ph) + 0.1 * np.cos(5 * ph) * np.sin(th) ** 2
    return (v * r[:, None]) * np.array([1.0, 0.8, 0.6]) + np.array([0.3, -0.2, 2.0])


TRUTH = rigid(3.0, (0.3, -0.5, 0.8), (0.02, -0.012, 0.009))     # source -> target, 3 degrees / 0.02


def noisy_scene(n_src=700, n_tgt=1900, seed=11):
    """The surface sampled twice, both samples noisy; the source displaced by the inverse of TRUTH."""
    rng = np.random.default_rng(seed)
    tgt = surface(rng, n_tgt) + rng.normal(scale=0.004, size=(n_tgt, 3))
    s = surface(rng, n_src) + rng.normal(scale=0.004, size=(n_src, 3))
    inv = np.linalg.inv(TRUTH)
    src = s @ inv[:3, :3].T + inv[:3, 3]
    return SimpleNamespace(src=src.astype(f32), tgt=tgt.astype(f32), truth=TRUTH)


def clean_scene(n=300, seed=5, scale=1.0):
    """The source is the target moved by the inverse of TRUTH (and shrunk by
    `scale`), exact up to the float32 rounding of its coordinates."""
    rng = np.random.default_rng(seed)
    tgt = surface(rng, n)
    inv = np.linalg.inv(TRUTH)
    src = (tgt @ inv[:3, :3].T + inv[:3, 3]) / scale
    T = TRUTH.copy()
    T[:3, :3] *= scale
    return SimpleNamespace(src=src.astype(f32), tgt=tgt.astype(f32), truth=T)


COARSE_KINDS = ("lattice", "coplanar", "collinear")


def coarse_scene(n_src, n_tgt, kind="lattice", seed=3):
    """Coordinates on a lattice of 1/4 (targets) and 1/8 (queries), so exact
    ties abound.  Targets: every fourth one repeats an earlier one (duplicates);
    `coplanar` flattens z, `collinear` y and z; n_tgt == 1 is the single-point
    target.  Queries: query 0 is exactly midway between targets 0 and 1 when
    there are two (bitwise-equal d2, target 0 must win), the last fifth lie far
    outside the box (up to 1e4 away), the others on the finer lattice in and
    around the box."""
    rng = np.random.default_rng(seed + 1000 * n_tgt + n_src)
    tgt = rng.integers(0, 64, size=(n_tgt, 3)).astype(np.float64) * 0.25
    for j in range(3, n_tgt, 4):
        tgt[j] = tgt[rng.integers(0, j)]
    if kind in ("coplanar", "collinear"):
        tgt[:, 2] = 4.0
    if kind == "collinear":
        tgt[:, 1] = 2.5
    if n_tgt >= 2 and np.all(tgt[0] == tgt[1]):
        tgt[1, 0] += 0.5
    src = rng.integers(-16, 144, size=(n_src, 3)).astype(np.float64) * 0.125
    far = max(n_src - n_src // 5, 1)
    src[far:] = rng.choice([-1e4, -100.0, 50.0, 300.0, 1e4], size=(n_src - far, 3)) + src[far:]
    if n_tgt >= 2:
        src[0] = 0.5 * (tgt[0] + tgt[1])
    return SimpleNamespace(src=src.astype(f32), tgt=tgt.astype(f32))
