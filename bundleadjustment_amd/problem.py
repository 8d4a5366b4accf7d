"""Problem container (SoA, the C-ABI layout) and synthetic BAL-style problems.

Parameter layout is the reference's (ba_project/src/ba/Optimizer.h:54-76):
camera = [wx, wy, wz, tx, ty, tz] world->camera angle-axis + translation,
point = world XYZ; K float 3x3 column-major; fixed cameras carry a float 4x4
column-major world->camera extrinsic (PointOnlyReprojectionError,
Optimizer.h:96-107).

Synthetic problems follow SURVEY.md §8(d): seed 0xBA5E0000 + k, cameras on a
ring of radius 5 looking at the origin, points uniform in a ball of radius 2,
each point seen by exactly `obs_per_pt` cameras chosen uniformly among those
that see it in front of the camera and inside the image, 1 px Gaussian pixel
noise plus 5 % gross outliers, perturbed initial values, camera 0 anchored.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

HUBER_A = math.sqrt(5.991)  # ceres::HuberLoss(sqrt(5.991)), Optimizer.cpp:312

# Intrinsics hard-coded in the reference's VirtualSensor.h
FREIBURG = dict(fx=525.0, fy=525.0, cx=319.5, cy=239.5, w=640, h=480)   # VirtualSensor.h:160-162
REPLICA = dict(fx=600.0, fy=600.0, cx=599.5, cy=339.5, w=1200, h=680)   # VirtualSensor.h:112-114


@dataclass
class Problem:
    cams: np.ndarray                      # (C, 6) float64
    K: np.ndarray                         # (C, 9) float32, column-major
    pts: np.ndarray                       # (P, 3) float64
    obs_cam: np.ndarray                   # (N,) int32
    obs_pt: np.ndarray                    # (N,) int32
    obs_uv: np.ndarray                    # (N, 2) float32
    cam_fixed: np.ndarray | None = None   # (C,) uint8
    cam_fixed_extr: np.ndarray | None = None  # (C, 16) float32, column-major
    pt_fixed: np.ndarray | None = None    # (P,) uint8
    huber_a: float = HUBER_A
    gt_cams: np.ndarray | None = field(default=None, repr=False)
    gt_pts: np.ndarray | None = field(default=None, repr=False)
    name: str = ""

    @property
    def n_cams(self) -> int:
        return int(self.cams.shape[0])

    @property
    def n_pts(self) -> int:
        return int(self.pts.shape[0])

    @property
    def n_obs(self) -> int:
        return int(self.obs_cam.shape[0])

    def normalized(self) -> "Problem":
        """Contiguous arrays of the exact dtypes the C-ABI expects."""
        def c(a, dt, shape=None):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt)
            return a.reshape(shape) if shape is not None else a
        return Problem(
            cams=c(self.cams, np.float64, (-1, 6)), K=c(self.K, np.float32, (-1, 9)),
            pts=c(self.pts, np.float64, (-1, 3)), obs_cam=c(self.obs_cam, np.int32),
            obs_pt=c(self.obs_pt, np.int32), obs_uv=c(self.obs_uv, np.float32, (-1, 2)),
            cam_fixed=c(self.cam_fixed, np.uint8), cam_fixed_extr=c(self.cam_fixed_extr, np.float32, (-1, 16)),
            pt_fixed=c(self.pt_fixed, np.uint8), huber_a=float(self.huber_a), gt_cams=self.gt_cams,
            gt_pts=self.gt_pts, name=self.name)

    def copy(self) -> "Problem":
        cp = lambda a: None if a is None else a.copy()
        return Problem(cp(self.cams), cp(self.K), cp(self.pts), cp(self.obs_cam), cp(self.obs_pt), cp(self.obs_uv),
                       cp(self.cam_fixed), cp(self.cam_fixed_extr), cp(self.pt_fixed), self.huber_a,
                       cp(self.gt_cams), cp(self.gt_pts), self.name)


# ---------------------------------------------------------------------------
# ceres rotation.h semantics, vectorised (column-major 3x3 as (..., 3, 3)
# standard matrices here: R[..., row, col]).
# ---------------------------------------------------------------------------
def angle_axis_to_rotation(w: np.ndarray) -> np.ndarray:
    """ceres::AngleAxisToRotationMatrix (first-order branch for theta^2 <= eps)."""
    w = np.asarray(w, dtype=np.float64)
    flat = w.reshape(-1, 3)
    th2 = np.einsum("ij,ij->i", flat, flat)
    R = np.empty((flat.shape[0], 3, 3))
    big = th2 > np.finfo(np.float64).eps
    if np.any(big):
        wb = flat[big]
        th = np.sqrt(th2[big])
        wx, wy, wz = (wb / th[:, None]).T
        c, s = np.cos(th), np.sin(th)
        oc = 1.0 - c
        R[big, 0, 0] = c + wx * wx * oc
        R[big, 1, 0] = wz * s + wx * wy * oc
        R[big, 2, 0] = -(wy * s) + wx * wz * oc
        R[big, 0, 1] = wx * wy * oc - wz * s
        R[big, 1, 1] = c + wy * wy * oc
        R[big, 2, 1] = wx * s + wy * wz * oc
        R[big, 0, 2] = wy * s + wx * wz * oc
        R[big, 1, 2] = -(wx * s) + wy * wz * oc
        R[big, 2, 2] = c + wz * wz * oc
    sm = ~big
    if np.any(sm):
        a = flat[sm]
        R[sm] = np.stack([np.stack([np.ones(len(a)), -a[:, 2], a[:, 1]], -1),
                          np.stack([a[:, 2], np.ones(len(a)), -a[:, 0]], -1),
                          np.stack([-a[:, 1], a[:, 0], np.ones(len(a))], -1)], 1)
    return R.reshape(w.shape[:-1] + (3, 3))


def rotation_to_angle_axis(R: np.ndarray) -> np.ndarray:
    """ceres::RotationMatrixToAngleAxis: Shepperd quaternion, then atan2."""
    R = np.asarray(R, dtype=np.float64)
    flat = R.reshape(-1, 3, 3)
    out = np.empty((flat.shape[0], 3))
    for n, M in enumerate(flat):
        q = [0.0, 0.0, 0.0, 0.0]
        tr = M[0, 0] + M[1, 1] + M[2, 2]
        if tr >= 0.0:
            t = math.sqrt(tr + 1.0)
            q[0] = 0.5 * t
            t = 0.5 / t
            q[1] = (M[2, 1] - M[1, 2]) * t
            q[2] = (M[0, 2] - M[2, 0]) * t
            q[3] = (M[1, 0] - M[0, 1]) * t
        else:
            i = 0
            if M[1, 1] > M[0, 0]:
                i = 1
            if M[2, 2] > M[i, i]:
                i = 2
            j, k = (i + 1) % 3, (i + 2) % 3
            t = math.sqrt(M[i, i] - M[j, j] - M[k, k] + 1.0)
            q[i + 1] = 0.5 * t
            t = 0.5 / t
            q[0] = (M[k, j] - M[j, k]) * t
            q[j + 1] = (M[j, i] + M[i, j]) * t
            q[k + 1] = (M[k, i] + M[i, k]) * t
        s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
        if s2 > 0.0:
            st = math.sqrt(s2)
            ct = q[0]
            two = 2.0 * (math.atan2(-st, -ct) if ct < 0.0 else math.atan2(st, ct))
            kk = two / st
            out[n] = (q[1] * kk, q[2] * kk, q[3] * kk)
        else:
            out[n] = (q[1] * 2.0, q[2] * 2.0, q[3] * 2.0)
    return out.reshape(R.shape[:-2] + (3,))


def K_colmajor(fx, fy, cx, cy) -> np.ndarray:
    return np.array([fx, 0, 0, 0, fy, 0, cx, cy, 1], dtype=np.float32)


def extr_colmajor(R: np.ndarray, t: np.ndarray) -> np.ndarray:
    E = np.eye(4, dtype=np.float32)
    E[:3, :3] = R.astype(np.float32)
    E[:3, 3] = t.astype(np.float32)
    return E.T.reshape(16).copy()   # column-major flatten


def project(R: np.ndarray, t: np.ndarray, K9: np.ndarray, X: np.ndarray) -> np.ndarray:
    """Pinhole projection of points X (N,3) with per-row R (N,3,3), t (N,3), K (N,9) col-major."""
    p = np.einsum("nij,nj->ni", R, X) + t
    Kd = K9.astype(np.float64).reshape(-1, 3, 3).transpose(0, 2, 1)
    q = np.einsum("nij,nj->ni", Kd, p)
    return q[:, :2] / q[:, 2:3], p[:, 2]


# ---------------------------------------------------------------------------
# synthetic problems
# ---------------------------------------------------------------------------
CONFIGS = {
    # name: (cams, points, obs/pt, intrinsics, motion_only)
    "f2f": dict(n_cams=1, n_pts=500, obs_per_pt=1, intr="freiburg", motion_only=True),
    "c1": dict(n_cams=2, n_pts=500, obs_per_pt=2, intr="freiburg"),
    "c2": dict(n_cams=50, n_pts=10_000, obs_per_pt=5, intr="replica"),
    "c3": dict(n_cams=200, n_pts=100_000, obs_per_pt=10, intr="freiburg"),
    "c4": dict(n_cams=1_000, n_pts=1_000_000, obs_per_pt=10, intr="freiburg"),
    "c5": dict(n_cams=10_000, n_pts=10_000_000, obs_per_pt=10, intr="freiburg"),
}
CONFIG_INDEX = {"f2f": 0, "c1": 0, "c2": 1, "c3": 2, "c4": 3, "c5": 4}


def _look_at(center: np.ndarray, target: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    z = target - center
    z /= np.linalg.norm(z)
    up = np.array([0.0, 0.0, 1.0])
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])           # rows = camera axes in world: world->camera
    return R, -R @ center


def make_synthetic(n_cams: int, n_pts: int, obs_per_pt: int = 10, seed: int = 0xBA5E0002,
                   intr: str = "freiburg", noise_px: float = 1.0, outlier_frac: float = 0.05,
                   perturb=(0.01, 0.02, 0.02), anchor: bool = True, motion_only: bool = False,
                   name: str = "", point_seed: int | None = None) -> Problem:
    """`seed` drives the cameras (and their initial perturbation); `point_seed`
    (default: same stream) drives points, visibility, pixel noise and point
    perturbation — so point shards of one scene share identical cameras."""
    rng = np.random.default_rng(seed)
    I = FREIBURG if intr == "freiburg" else REPLICA
    W, H = I["w"], I["h"]
    K9 = K_colmajor(I["fx"], I["fy"], I["cx"], I["cy"])
    Kf = np.tile(K9, (n_cams, 1))
    # cameras on a ring of radius 5 (height jitter) looking at the origin
    if n_cams == 1:
        phis = np.array([0.0])
    else:
        phis = np.linspace(0.0, 2.0 * np.pi, n_cams, endpoint=False)
    Rs = np.empty((n_cams, 3, 3))
    ts = np.empty((n_cams, 3))
    for i, ph in enumerate(phis):
        h = rng.uniform(-1.0, 1.0) if n_cams > 2 else 0.3 * i
        if n_cams == 2:
            ph = 0.25 * i
        center = np.array([5.0 * np.cos(ph), 5.0 * np.sin(ph), h])
        target = rng.normal(0.0, 0.1, 3)
        Rs[i], ts[i] = _look_at(center, target)
    cam_noise = None
    if perturb is not None:
        cam_noise = (rng.normal(0.0, perturb[0], size=(n_cams, 3)), rng.normal(0.0, perturb[1], size=(n_cams, 3)))
    if point_seed is not None:
        rng = np.random.default_rng(point_seed)
    # points uniform in a ball of radius 2
    d = rng.normal(size=(n_pts, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    X = d * (2.0 * rng.uniform(size=(n_pts, 1)) ** (1.0 / 3.0))
    k = min(obs_per_pt, n_cams)
    # visibility-constrained uniform choice of k cameras per point
    m = n_cams if n_cams <= 512 else min(n_cams, 8 * k + 64)
    obs_c, obs_p = [], []
    chunk = max(1, 4_000_000 // max(m, 1))
    for s0 in range(0, n_pts, chunk):
        Xc = X[s0:s0 + chunk]
        nb = Xc.shape[0]
        cand = (np.tile(np.arange(n_cams), (nb, 1)) if m == n_cams
                else rng.integers(0, n_cams, size=(nb, m)))
        Rc, tc = Rs[cand], ts[cand]                                     # (nb, m, 3, 3)
        pc = np.einsum("bmij,bj->bmi", Rc, Xc) + tc
        z = pc[..., 2]
        u = I["fx"] * pc[..., 0] / z + I["cx"]
        v = I["fy"] * pc[..., 1] / z + I["cy"]
        vis = (z > 0.1) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        if m != n_cams:  # de-duplicate sampled candidates
            srt = np.sort(cand, axis=1)
            dup = np.zeros_like(vis)
            order = np.argsort(cand, axis=1, kind="stable")
            dup_sorted = np.concatenate([np.zeros((nb, 1), bool), srt[:, 1:] == srt[:, :-1]], 1)
            np.put_along_axis(dup, order, dup_sorted, axis=1)
            vis &= ~dup
        key = rng.uniform(size=vis.shape)
        key[~vis] = 2.0
        sel = np.argsort(key, axis=1)[:, :k]
        ok = np.take_along_axis(key, sel, 1) < 2.0
        cams_sel = np.take_along_axis(cand, sel, 1)
        cams_sel = np.where(ok, cams_sel, -1)
        cams_sel.sort(axis=1)
        pid = np.repeat(np.arange(s0, s0 + nb)[:, None], k, 1)
        keep = cams_sel >= 0
        obs_c.append(cams_sel[keep])
        obs_p.append(pid[keep])
    obs_cam = np.concatenate(obs_c).astype(np.int32)
    obs_pt = np.concatenate(obs_p).astype(np.int32)
    # drop points with fewer than 2 observations (unless motion-only)
    if not motion_only:
        cnt = np.bincount(obs_pt, minlength=n_pts)
        good = cnt[obs_pt] >= min(2, k)
        obs_cam, obs_pt = obs_cam[good], obs_pt[good]
    uv, _ = project(Rs[obs_cam], ts[obs_cam], Kf[obs_cam], X[obs_pt])
    n_obs = len(obs_cam)
    if noise_px > 0:
        uv = uv + rng.normal(0.0, noise_px, size=uv.shape)
    if outlier_frac > 0:
        bad = rng.uniform(size=n_obs) < outlier_frac
        uv[bad, 0] = rng.uniform(0, W, size=bad.sum())
        uv[bad, 1] = rng.uniform(0, H, size=bad.sum())
    w_gt = rotation_to_angle_axis(Rs)
    gt_cams = np.concatenate([w_gt, ts], 1)
    cams = gt_cams.copy()
    pts = X.copy()
    if perturb is not None:
        cams[:, :3] += cam_noise[0]
        cams[:, 3:] += cam_noise[1]
        if not motion_only:
            pts += rng.normal(0.0, perturb[2], size=pts.shape)
    cam_fixed = np.zeros(n_cams, np.uint8)
    extr = np.zeros((n_cams, 16), np.float32)
    if anchor and not motion_only:
        cam_fixed[0] = 1
        extr[0] = extr_colmajor(Rs[0], ts[0])
        # the anchor's angle-axis is what prepareConstraints derives from the
        # float extrinsic (Optimizer.cpp:296-299)
        Rf = extr[0].reshape(4, 4).T[:3, :3].astype(np.float64)
        cams[0, :3] = rotation_to_angle_axis(Rf)
        cams[0, 3:] = extr[0].reshape(4, 4).T[:3, 3].astype(np.float64)
    pt_fixed = None
    if motion_only:
        pt_fixed = np.ones(n_pts, np.uint8)
        pts = pts.astype(np.float32).astype(np.float64)   # Vector4f homogeneous point (Optimizer.h:158)
    return Problem(cams=cams, K=Kf, pts=pts, obs_cam=obs_cam, obs_pt=obs_pt, obs_uv=uv.astype(np.float32),
                   cam_fixed=cam_fixed, cam_fixed_extr=extr, pt_fixed=pt_fixed, huber_a=HUBER_A,
                   gt_cams=gt_cams, gt_pts=X, name=name).normalized()


def fix_camera(problem: Problem, c: int) -> Problem:
    """Anchor camera c at its current estimate the way prepareConstraints does
    for keyframe 0 (Optimizer.cpp:296-299, 314-321): the constant functor gets
    the float 4x4 extrinsic, the angle-axis block is re-derived from it."""
    R = angle_axis_to_rotation(problem.cams[c, :3])
    if problem.cam_fixed is None:
        problem.cam_fixed = np.zeros(problem.n_cams, np.uint8)
    if problem.cam_fixed_extr is None:
        problem.cam_fixed_extr = np.zeros((problem.n_cams, 16), np.float32)
    problem.cam_fixed[c] = 1
    problem.cam_fixed_extr[c] = extr_colmajor(R, problem.cams[c, 3:])
    E = problem.cam_fixed_extr[c].reshape(4, 4).T
    problem.cams[c, :3] = rotation_to_angle_axis(E[:3, :3].astype(np.float64))
    problem.cams[c, 3:] = E[:3, 3].astype(np.float64)
    return problem


def make_config(name: str, scale: float = 1.0, **overrides) -> Problem:
    """Synthetic problem of a BASELINE.json config (seed 0xBA5E0000 + config index)."""
    cfg = dict(CONFIGS[name])
    cfg.update(overrides)
    if scale != 1.0:
        cfg["n_pts"] = max(1, int(cfg["n_pts"] * scale))
    seed = cfg.pop("seed", 0xBA5E0000 + CONFIG_INDEX[name])
    return make_synthetic(seed=seed, name=name, **cfg)


@dataclass
class WindowBatch:
    """Independent small problems concatenated in the layout of the C-ABI's
    ba_window_batch: problem i owns cameras [cam_offset[i], cam_offset[i+1]),
    points [pt_offset[i], pt_offset[i+1]) and observations [obs_offset[i],
    obs_offset[i+1]); obs_cam / obs_pt stay local to their problem."""
    cam_offset: np.ndarray      # (n + 1,) int32
    pt_offset: np.ndarray       # (n + 1,) int32
    obs_offset: np.ndarray      # (n + 1,) int32
    cams: np.ndarray            # (C, 6) float64
    cam_fixed: np.ndarray       # (C,) uint8
    cam_fixed_extr: np.ndarray  # (C, 16) float32
    K: np.ndarray               # (C, 9) float32
    pts: np.ndarray             # (P, 3) float64
    pt_fixed: np.ndarray        # (P,) uint8
    obs_cam: np.ndarray         # (N,) int32
    obs_pt: np.ndarray          # (N,) int32
    obs_uv: np.ndarray          # (N, 2) float32
    huber_a: float = HUBER_A

    @property
    def n_problems(self) -> int:
        return int(self.cam_offset.shape[0]) - 1


def pack_window_batch(problems: list[Problem]) -> WindowBatch:
    """Concatenate problems for Solver.solve_window_batch (pure numpy).  A
    missing cam_fixed / pt_fixed becomes zeros, a missing cam_fixed_extr zeros
    (never read for variable cameras).  huber_a is one value per batch: the
    problems must agree on it."""
    ps = [p.normalized() for p in problems]
    huber = {float(p.huber_a) for p in ps}
    if len(huber) > 1:
        raise ValueError(f"pack_window_batch: the problems disagree on huber_a: {sorted(huber)}")

    def off(counts):
        o = np.zeros(len(ps) + 1, np.int64)
        np.cumsum(counts, out=o[1:])
        if o[-1] > np.iinfo(np.int32).max:
            raise ValueError("pack_window_batch: the batch does not fit 32-bit offsets")
        return o.astype(np.int32)

    def cat(arrs, dt, tail):
        arrs = [np.asarray(a, dt).reshape((-1,) + tail) for a in arrs]
        return np.ascontiguousarray(np.concatenate(arrs, axis=0) if arrs else np.zeros((0,) + tail, dt), dtype=dt)

    return WindowBatch(
        cam_offset=off([p.n_cams for p in ps]), pt_offset=off([p.n_pts for p in ps]),
        obs_offset=off([p.n_obs for p in ps]),
        cams=cat([p.cams for p in ps], np.float64, (6,)),
        cam_fixed=cat([np.zeros(p.n_cams, np.uint8) if p.cam_fixed is None else p.cam_fixed for p in ps], np.uint8, ()),
        cam_fixed_extr=cat([np.zeros((p.n_cams, 16), np.float32) if p.cam_fixed_extr is None else p.cam_fixed_extr
                            for p in ps], np.float32, (16,)),
        K=cat([p.K for p in ps], np.float32, (9,)),
        pts=cat([p.pts for p in ps], np.float64, (3,)),
        pt_fixed=cat([np.zeros(p.n_pts, np.uint8) if p.pt_fixed is None else p.pt_fixed for p in ps], np.uint8, ()),
        obs_cam=cat([p.obs_cam for p in ps], np.int32, ()), obs_pt=cat([p.obs_pt for p in ps], np.int32, ()),
        obs_uv=cat([p.obs_uv for p in ps], np.float32, (2,)),
        huber_a=huber.pop() if huber else HUBER_A)


def shard_points(problem: Problem, nranks: int, rank: int, bounds: list[int] | None = None) -> Problem:
    """Point-sharded slice for multi-GPU: contiguous point
    ranges balanced by observation count (or the given `bounds`, nranks + 1
    point offsets; a rank may get none); cameras replicated; the shard keeps
    only its points' observations (re-indexed)."""
    bounds = shard_bounds(problem, nranks) if bounds is None else bounds
    p0, p1 = bounds[rank], bounds[rank + 1]
    sel = (problem.obs_pt >= p0) & (problem.obs_pt < p1)
    sub = problem.copy()
    sub.pts = problem.pts[p0:p1].copy()
    sub.pt_fixed = None if problem.pt_fixed is None else problem.pt_fixed[p0:p1].copy()
    sub.obs_cam = problem.obs_cam[sel].copy()
    sub.obs_pt = (problem.obs_pt[sel] - p0).astype(np.int32)
    sub.obs_uv = problem.obs_uv[sel].copy()
    sub.gt_pts = None if problem.gt_pts is None else problem.gt_pts[p0:p1].copy()
    return sub.normalized()


def shard_bounds(problem: Problem, nranks: int) -> list[int]:
    cnt = np.bincount(problem.obs_pt, minlength=problem.n_pts).astype(np.int64)
    csum = np.concatenate([[0], np.cumsum(cnt)])
    total = csum[-1]
    b = [int(np.searchsorted(csum, total * r / nranks, side="left")) for r in range(nranks + 1)]
    b[0], b[-1] = 0, problem.n_pts
    return b


@dataclass
class TriangulationBatch:
    """The arrays of the C-ABI's ba_tri_batch: point p owns observations
    [obs_offset[p], obs_offset[p+1]), in the caller's order within a point."""
    extr: np.ndarray         # (C, 16) float32, column-major world->camera
    cam_center: np.ndarray   # (C, 3) float32 camera centres in the world (getWorldPos)
    K: np.ndarray            # (C, 9) float32
    obs_offset: np.ndarray   # (P + 1,) int32
    obs_cam: np.ndarray      # (N,) int32
    obs_uv: np.ndarray       # (N, 2) float32
    pts: np.ndarray          # (P, 3) float64: the problem's points (a start for TRI_INIT_GIVEN)
    order: np.ndarray        # (N,) the problem's observation index of each batch observation
    huber_a: float = HUBER_A


def triangulation_batch(problem: Problem) -> TriangulationBatch:
    """A Problem whose cameras are all constant as the batch arrays of
    Solver.triangulate: observations sorted by point (stable: a point's first
    observation stays its first), offsets, the float extrinsics and the camera
    centres -R^T t derived from them."""
    p = problem.normalized()
    if p.cam_fixed is None or p.cam_fixed_extr is None or not np.all(p.cam_fixed != 0):
        raise ValueError("triangulation_batch: every camera must be constant (fix_camera)")
    order = np.argsort(p.obs_pt, kind="stable")
    cnt = np.bincount(p.obs_pt, minlength=p.n_pts).astype(np.int64)
    off = np.zeros(p.n_pts + 1, np.int64)
    np.cumsum(cnt, out=off[1:])
    E = p.cam_fixed_extr.reshape(-1, 4, 4).transpose(0, 2, 1).astype(np.float64)   # [row, col]
    center = -np.einsum("cji,cj->ci", E[:, :3, :3], E[:, :3, 3])
    return TriangulationBatch(
        extr=p.cam_fixed_extr.copy(), cam_center=np.ascontiguousarray(center, dtype=np.float32), K=p.K.copy(),
        obs_offset=off.astype(np.int32), obs_cam=np.ascontiguousarray(p.obs_cam[order]),
        obs_uv=np.ascontiguousarray(p.obs_uv[order]), pts=p.pts.copy(), order=order.astype(np.int64),
        huber_a=float(p.huber_a))


# one record of Solver.match_descriptors (ba_match, include/ba_hip.h)
MATCH_DTYPE = np.dtype([("query", np.int32), ("train", np.int32), ("distance", np.float32),
                        ("second_distance", np.float32), ("ref_distance", np.float32)])
# one record of Solver.match_knn (ba_match_neighbors)
MATCH_KNN_DTYPE = np.dtype([("idx0", np.int32), ("idx1", np.int32), ("d2_0", np.float32), ("d2_1", np.float32)])


@dataclass
class MatchBatch:
    """The arrays of the C-ABI's ba_match_batch: set s owns rows
    [set_offset[s], set_offset[s+1]) of desc; pair i matches set pairs[i, 0]
    (queries) against set pairs[i, 1] (train)."""
    dim: int
    set_offset: np.ndarray         # (S + 1,) int32
    desc: np.ndarray               # (rows, dim) float32
    pairs: np.ndarray              # (P, 2) int32: (query set, train set)
    row_ref: np.ndarray | None     # (rows,) int32: index into ref_desc or -1
    ref_desc: np.ndarray | None    # (R, dim) float32


def pack_match_batch(sets, pairs, row_ref=None, ref_desc=None, dim: int | None = None) -> MatchBatch:
    """Descriptor sets (a list of (n_s, dim) arrays, empty ones allowed) and
    (query set, train set) index pairs as a MatchBatch.  row_ref: per set, an
    int array naming a row of ref_desc per descriptor (-1: none), or None for a
    set without references.  dim is needed only when every set is empty."""
    sets = [np.asarray(s, dtype=np.float32) for s in sets]
    if dim is None:
        dims = {s.shape[1] for s in sets if s.ndim == 2 and s.shape[0] > 0}
        if ref_desc is not None and np.asarray(ref_desc).ndim == 2:
            dims.add(np.asarray(ref_desc).shape[1])
        if len(dims) != 1:
            raise ValueError("pack_match_batch: the sets do not agree on one descriptor length")
        dim = dims.pop()
    sets = [s.reshape(-1, dim) for s in sets]
    off = np.zeros(len(sets) + 1, np.int64)
    np.cumsum([s.shape[0] for s in sets], out=off[1:])
    desc = np.ascontiguousarray(np.concatenate(sets, axis=0) if sets else np.zeros((0, dim)), dtype=np.float32)
    rr = None
    if row_ref is not None:
        if len(row_ref) != len(sets):
            raise ValueError("pack_match_batch: row_ref needs one entry per set")
        rr = np.full(int(off[-1]), -1, np.int32)
        for s, r in enumerate(row_ref):
            if r is not None:
                rr[off[s]:off[s + 1]] = np.asarray(r, dtype=np.int32).reshape(-1)
    rd = None if ref_desc is None else np.ascontiguousarray(ref_desc, dtype=np.float32).reshape(-1, dim)
    return MatchBatch(dim=int(dim), set_offset=off.astype(np.int32), desc=desc,
                      pairs=np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2), row_ref=rr, ref_desc=rd)


# one record of Solver.icp (ba_icp_result, include/ba_hip.h)
ICP_RESULT_DTYPE = np.dtype([("final", np.float32, (4, 4)), ("converged", np.int32), ("state", np.int32),
                             ("iterations", np.int32), ("n_corr", np.int32), ("fitness", np.float64)])


@dataclass
class IcpBatch:
    """The arrays of the C-ABI's ba_icp_batch: set s owns points
    [set_offset[s], set_offset[s+1]) of xyz; pair i aligns set pairs[i, 0]
    (the source) to set pairs[i, 1] (the target)."""
    set_offset: np.ndarray         # (S + 1,) int32
    xyz: np.ndarray                # (points, 3) float32
    pairs: np.ndarray              # (P, 2) int32: (source set, target set)
    guess: np.ndarray | None       # (P, 4, 4) float32, row-major


def pack_icp_batch(sets, pairs, guess=None) -> IcpBatch:
    """Point clouds (a list of (n_s, 3) arrays) and (source set, target set)
    index pairs as an IcpBatch.  guess: per pair a 4x4 initial transform of
    the source, or None for the identity."""
    sets = [np.asarray(s, dtype=np.float32).reshape(-1, 3) for s in sets]
    off = np.zeros(len(sets) + 1, np.int64)
    np.cumsum([s.shape[0] for s in sets], out=off[1:])
    xyz = np.ascontiguousarray(np.concatenate(sets, axis=0) if sets else np.zeros((0, 3)), dtype=np.float32)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    g = None
    if guess is not None:
        g = np.ascontiguousarray(guess, dtype=np.float32).reshape(-1, 4, 4)
        if g.shape[0] != pairs.shape[0]:
            raise ValueError("pack_icp_batch: guess needs one 4x4 per pair")
    return IcpBatch(set_offset=off.astype(np.int32), xyz=xyz, pairs=pairs, guess=g)


# one record of Solver.map_points_update (ba_map_point, include/ba_hip.h)
MAP_POINT_DTYPE = np.dtype([("status", np.int32), ("best", np.int32), ("median", np.float32), ("view_dir", np.float32, 3),
                            ("min_dist", np.float32), ("max_dist", np.float32)])
# the records of Solver.associate (ba_assoc_result, ba_fuse_result)
ASSOC_DTYPE = np.dtype([("status", np.int32), ("chi", np.float32), ("cosine", np.float32), ("world_dist", np.float32),
                        ("dist_matched", np.float32), ("dist_current", np.float32)])
FUSE_DTYPE = np.dtype([("status", np.int32), ("cosine", np.float32), ("dist", np.float32)])


def _f32(a, shape):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(shape)


def _i32(a, shape=(-1,)):
    return np.ascontiguousarray(a, dtype=np.int32).reshape(shape)


@dataclass
class MapPointBatch:
    """The arrays of the C-ABI's ba_map_point_batch: point p owns observations
    [obs_offset[p], obs_offset[p+1]), its track in caller order."""
    dim: int
    cam_center: np.ndarray         # (C, 3) float32
    pts: np.ndarray                # (P, 3) float32
    obs_offset: np.ndarray         # (P + 1,) int32
    obs_cam: np.ndarray            # (O,) int32
    obs_row: np.ndarray            # (O,) int32: row of desc
    obs_scale: np.ndarray | None   # (O,) float32
    ref_obs: np.ndarray | None     # (P,) int32: local index within the track
    desc: np.ndarray               # (R, dim) float32


def pack_map_point_batch(cam_center, pts, tracks, desc, scales=None, ref_obs=None) -> MapPointBatch:
    """tracks: per point a list of (camera, descriptor row) in the order the
    track is to be walked; scales: per point a list of pow(1.2, octave) per
    observation (None: all 1); ref_obs: per point the local index of the
    reference keyframe's observation (None: 0)."""
    desc = np.ascontiguousarray(desc, dtype=np.float32)
    if desc.ndim != 2:
        raise ValueError("pack_map_point_batch: desc must be (rows, dim)")
    off = np.zeros(len(tracks) + 1, np.int64)
    np.cumsum([len(t) for t in tracks], out=off[1:])
    flat = np.array([o for t in tracks for o in t], np.int32).reshape(-1, 2)
    sc = None
    if scales is not None:
        sc = np.array([v for t in scales for v in t], np.float32)
        if sc.size != flat.shape[0]:
            raise ValueError("pack_map_point_batch: scales needs one value per observation")
    return MapPointBatch(dim=int(desc.shape[1]), cam_center=_f32(cam_center, (-1, 3)), pts=_f32(pts, (-1, 3)),
                         obs_offset=off.astype(np.int32), obs_cam=np.ascontiguousarray(flat[:, 0]),
                         obs_row=np.ascontiguousarray(flat[:, 1]), obs_scale=sc,
                         ref_obs=None if ref_obs is None else _i32(ref_obs), desc=desc)


@dataclass
class AssocBatch:
    """The arrays of the C-ABI's ba_assoc_batch."""
    dim: int
    extr: np.ndarray               # (C, 16) float32, col-major world->camera
    cam_center: np.ndarray         # (C, 3)
    K: np.ndarray                  # (C, 9) col-major
    image_size: np.ndarray         # (C, 2) int32: width, height
    pts: np.ndarray                # (P, 3)
    pt_view_dir: np.ndarray        # (P, 3)
    pt_dist: np.ndarray            # (P, 2): min, max
    pt_desc: np.ndarray            # (P, dim)
    desc: np.ndarray               # (R, dim)
    item_cam: np.ndarray           # (I,) int32
    item_pt: np.ndarray            # (I,) int32
    item_uv: np.ndarray            # (I, 2)
    item_scale: np.ndarray | None  # (I,)
    item_row: np.ndarray           # (I,) int32
    item_cur_row: np.ndarray | None  # (I,) int32, -1: not observed
    fuse_pairs: np.ndarray         # (F, 2) int32


def pack_assoc_batch(extr, cam_center, K, image_size, pts, pt_view_dir, pt_dist, pt_desc, desc, item_cam=(), item_pt=(),
                     item_uv=(), item_row=(), item_scale=None, item_cur_row=None, fuse_pairs=()) -> AssocBatch:
    """The snapshot that Solver.associate tests: cameras, map points (view
    direction, depth bounds and descriptor as map_points_update returns them),
    keypoint descriptors, the candidate items and the fuse pairs."""
    desc = np.ascontiguousarray(desc, dtype=np.float32)
    dim = int(desc.shape[1])
    return AssocBatch(dim=dim, extr=_f32(extr, (-1, 16)), cam_center=_f32(cam_center, (-1, 3)), K=_f32(K, (-1, 9)),
                      image_size=_i32(image_size, (-1, 2)), pts=_f32(pts, (-1, 3)), pt_view_dir=_f32(pt_view_dir, (-1, 3)),
                      pt_dist=_f32(pt_dist, (-1, 2)), pt_desc=_f32(pt_desc, (-1, dim)), desc=desc,
                      item_cam=_i32(item_cam), item_pt=_i32(item_pt), item_uv=_f32(item_uv, (-1, 2)),
                      item_scale=None if item_scale is None else _f32(item_scale, (-1,)), item_row=_i32(item_row),
                      item_cur_row=None if item_cur_row is None else _i32(item_cur_row),
                      fuse_pairs=_i32(fuse_pairs, (-1, 2)))


# one record of Solver.map_graph (ba_graph_frame, include/ba_hip.h)
GRAPH_FRAME_DTYPE = np.dtype([(n, np.int32) for n in ("status", "degree", "max_weight", "n_map", "n_redundant", "cull",
                                                       "n_local", "n_fixed", "n_win_pts", "n_win_obs")])


@dataclass
class MapTable:
    """The arrays of the C-ABI's ba_map_table: a point-sorted observation table.
    Point p owns observations [obs_offset[p], obs_offset[p+1]), its track."""
    frame_id: np.ndarray               # (F,) int32: Frame::getID()
    obs_offset: np.ndarray             # (P + 1,) int32
    obs_frame: np.ndarray              # (O,) int32
    frame_is_key: np.ndarray | None = None   # (F,) uint8; None: all 1
    pt_invalid: np.ndarray | None = None     # (P,) uint8; None: all 0
    pt_ref_frame: np.ndarray | None = None   # (P,) int32; needed for the point status only
    obs_octave: np.ndarray | None = None     # (O,) int32; None: all 0
    obs_outlier: np.ndarray | None = None    # (O,) uint8; None: all 0
    order: np.ndarray | None = None          # (O,) the problem's observation index of each table observation

    @property
    def n_frames(self) -> int:
        return int(self.frame_id.shape[0])

    @property
    def n_pts(self) -> int:
        return int(self.obs_offset.shape[0]) - 1

    @property
    def n_obs(self) -> int:
        return int(self.obs_frame.shape[0])

    def normalized(self) -> "MapTable":
        u8 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)
        i32 = lambda a: None if a is None else _i32(a)
        return MapTable(frame_id=_i32(self.frame_id), obs_offset=_i32(self.obs_offset), obs_frame=_i32(self.obs_frame),
                        frame_is_key=u8(self.frame_is_key), pt_invalid=u8(self.pt_invalid),
                        pt_ref_frame=i32(self.pt_ref_frame), obs_octave=i32(self.obs_octave),
                        obs_outlier=u8(self.obs_outlier), order=self.order)


def map_table_from_problem(problem: Problem, frame_id=None, octave=None, outlier=None, frame_is_key=None,
                           pt_invalid=None, pt_ref_frame=None) -> MapTable:
    """The observation table of a Problem for Solver.map_graph: cameras are
    frames (frame_id defaults to the camera index).  octave and outlier are per
    observation in the problem's order.  The observations are put in point
    order (a stable sort; a Problem from make_synthetic already is) and
    `order` keeps the problem's index of each."""
    obs_pt = np.asarray(problem.obs_pt, np.int64)
    order = np.argsort(obs_pt, kind="stable")
    off = np.zeros(problem.n_pts + 1, np.int64)
    np.cumsum(np.bincount(obs_pt, minlength=problem.n_pts), out=off[1:])
    take = lambda a, dt: None if a is None else np.ascontiguousarray(np.asarray(a, dt).reshape(-1)[order])
    return MapTable(frame_id=_i32(np.arange(problem.n_cams) if frame_id is None else frame_id),
                    obs_offset=off.astype(np.int32), obs_frame=take(problem.obs_cam, np.int32),
                    frame_is_key=frame_is_key, pt_invalid=pt_invalid, pt_ref_frame=pt_ref_frame,
                    obs_octave=take(octave, np.int32), obs_outlier=take(outlier, np.uint8), order=order).normalized()


@dataclass
class MapGraphResult:
    """What Solver.map_graph returns: the records (GRAPH_FRAME_DTYPE, one per
    query) and the variable-length lists split per query."""
    query: np.ndarray
    records: np.ndarray
    nbr_frame: list
    nbr_weight: list
    win_cam: list
    win_cam_fixed: list
    win_pt: list
    win_obs: list
    win_obs_cam: list
    win_obs_pt: list
    pt_status: np.ndarray | None = None
    table: MapTable | None = field(default=None, repr=False)


def windows_from_graph(problem: Problem, result: MapGraphResult) -> list[Problem]:
    """The local-BA window of every query of `result` (Solver.map_graph on
    map_table_from_problem(problem) with build_windows) as a Problem that
    Solver.solve_window_batch accepts: the window's cameras, K, points and the
    uv of its observations, cam_fixed from win_cam_fixed, and for a fixed
    camera the float extrinsic and the re-derived pose as fix_camera forms
    them."""
    order = None if result.table is None else result.table.order
    out = []
    for i in range(len(result.win_cam)):
        cam, pt, obs = result.win_cam[i], result.win_pt[i], result.win_obs[i]
        src = obs if order is None else order[obs]
        w = Problem(cams=problem.cams[cam].copy(), K=problem.K[cam].copy(), pts=problem.pts[pt].copy(),
                    obs_cam=result.win_obs_cam[i].astype(np.int32), obs_pt=result.win_obs_pt[i].astype(np.int32),
                    obs_uv=problem.obs_uv[src].copy(), cam_fixed=np.zeros(cam.size, np.uint8),
                    cam_fixed_extr=np.zeros((cam.size, 16), np.float32),
                    pt_fixed=None if problem.pt_fixed is None else problem.pt_fixed[pt].copy(),
                    huber_a=problem.huber_a, name=f"{problem.name}/window{int(result.query[i])}")
        for c in np.flatnonzero(result.win_cam_fixed[i]):
            fix_camera(w, int(c))
        out.append(w.normalized())
    return out
