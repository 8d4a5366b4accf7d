"""Host-side Python handle on libba_hip.so: one `Solver` per (process, GPU).

Mirrors the ceres::Problem / ceres::Solve seam the reference uses
(ba_project/src/ba/Optimizer.cpp:225-242): build the problem, solve with the
options of BAOptimizer::configureSolver (Optimizer.cpp:80-90), read back the
parameters.  Everything numeric runs in the HIP library.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native as N
from .problem import (ASSOC_DTYPE, FUSE_DTYPE, GRAPH_FRAME_DTYPE, HUBER_A, ICP_RESULT_DTYPE, MAP_POINT_DTYPE, MATCH_DTYPE,
                      MATCH_KNN_DTYPE, AssocBatch, IcpBatch, MapGraphResult, MapPointBatch, MapTable, MatchBatch, Problem,
                      WindowBatch, pack_icp_batch, pack_match_batch, pack_window_batch)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@dataclass
class Options:
    """ceres::Solver::Options fields used by the reference (+ Ceres defaults)."""
    max_num_iterations: int = 50
    max_num_consecutive_invalid_steps: int = 5
    jacobi_scaling: bool = True
    function_tolerance: float = 1e-6
    gradient_tolerance: float = 1e-10
    parameter_tolerance: float = 1e-8
    initial_trust_region_radius: float = 1e4
    max_trust_region_radius: float = 1e16
    min_trust_region_radius: float = 1e-32
    min_relative_decrease: float = 1e-3
    min_lm_diagonal: float = 1e-6
    max_lm_diagonal: float = 1e32
    # linear solver: "DENSE_SCHUR" (the reference's, Optimizer.cpp:85) or
    # "ITERATIVE_SCHUR" (implicit Schur + PCG, for C5-scale camera counts)
    linear_solver_type: str = "DENSE_SCHUR"
    preconditioner_type: str = "JACOBI"        # ceres default; or "SCHUR_JACOBI"
    max_linear_solver_iterations: int = 500
    min_linear_solver_iterations: int = 0
    eta: float = 1e-1
    precision: str = "FP64"                    # or "MIXED_FP32" (ITERATIVE_SCHUR)

    def to_c(self) -> N.ba_options:
        o = N.ba_options()
        o.max_num_iterations = int(self.max_num_iterations)
        o.max_num_consecutive_invalid_steps = int(self.max_num_consecutive_invalid_steps)
        o.jacobi_scaling = int(bool(self.jacobi_scaling))
        o.linear_solver = {"DENSE_SCHUR": 0, "ITERATIVE_SCHUR": 1}[self.linear_solver_type]
        o.preconditioner_type = {"JACOBI": 0, "SCHUR_JACOBI": 1}[self.preconditioner_type]
        o.max_linear_solver_iterations = int(self.max_linear_solver_iterations)
        o.min_linear_solver_iterations = int(self.min_linear_solver_iterations)
        o.precision = {"FP64": 0, "MIXED_FP32": 1}[self.precision]
        o.eta = float(self.eta)
        for f in ("function_tolerance", "gradient_tolerance", "parameter_tolerance",
                  "initial_trust_region_radius", "max_trust_region_radius", "min_trust_region_radius",
                  "min_relative_decrease", "min_lm_diagonal", "max_lm_diagonal"):
            setattr(o, f, float(getattr(self, f)))
        return o


@dataclass
class Summary:
    initial_cost: float
    final_cost: float
    num_iterations: int
    num_successful_steps: int
    num_unsuccessful_steps: int
    termination_type: str
    total_time_s: float
    linearize_time_s: float
    solve_time_s: float


@dataclass
class PnpResult:
    """ba_pnp_result: status is an N.PNP_* code."""
    status: int
    n_inliers: int
    n_inliers_ransac: int
    best_hypothesis: int
    cam_ransac: np.ndarray
    refine: Summary


@dataclass
class TwoViewResult:
    """ba_two_view_result: status is an N.TV_* code, model N.TV_ESSENTIAL or
    N.TV_HOMOGRAPHY; cam = [w, t] maps frame 1 to frame 2.  best_solution_e
    (the C struct's `reserved`): with e_solver = N.TV_E_FIVE_POINT the index
    of the winning solution within best_hypothesis_e, else 0."""
    status: int
    model: int
    n_inliers: int
    n_good: int
    n_good_second: int
    best_hypothesis_e: int
    best_hypothesis_h: int
    votes_e: int
    votes_h: int
    score_e: float
    score_h: float
    E: np.ndarray
    H: np.ndarray
    cam: np.ndarray
    normal: np.ndarray
    best_solution_e: int = 0


ITER_FIELDS = [f for f, _ in N.ba_iteration._fields_]
PNP_OPTION_FIELDS = [f for f, _ in N.ba_pnp_options._fields_ if f != "reserved"]
TV_OPTION_FIELDS = [f for f, _ in N.ba_two_view_options._fields_ if f != "reserved"]


class Solver:
    """A ba_ctx on one HIP device."""

    def __init__(self, device: int = 0):
        self.lib = N.load_library()
        h = C.c_void_p()
        st = self.lib.ba_create(C.byref(h), int(device))
        if st != N.BA_OK:
            raise N.BAError(st, f"ba_create(device={device}) failed")
        self.h = h
        self.problem: Problem | None = None
        self._keep = []

    def close(self):
        if getattr(self, "h", None):
            self.lib.ba_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, st: int, what: str):
        if st != N.BA_OK:
            raise N.BAError(st, f"{what}: {self.lib.ba_last_error(self.h).decode(errors='replace')}")

    def _times(self, getter) -> np.ndarray:
        """What a ba_*_times getter holds (ms), as an array."""
        n = getter(self.h, None, 0)
        out = np.empty(max(n, 0))
        if n > 0:
            getter(self.h, _ptr(out), n)
        return out

    @staticmethod
    def _set_options(p, options: dict, fields: dict, who: str):
        """Keyword options into the ctypes options struct p; fields: name -> conversion."""
        for key, val in options.items():
            if key not in fields:
                raise TypeError(f"{who}: unknown option {key!r}")
            setattr(p, key, fields[key](val))
        return p

    # -- multi-GPU ------------------------------------------------------
    @staticmethod
    def unique_id() -> bytes:
        lib = N.load_library()
        buf = C.create_string_buffer(128)
        st = lib.ba_comm_unique_id(buf)
        if st != N.BA_OK:
            raise N.BAError(st, "ba_comm_unique_id")
        return buf.raw

    def comm_init(self, uid: bytes, nranks: int, rank: int):
        assert len(uid) == 128
        self._check(self.lib.ba_comm_init(self.h, C.c_char_p(uid), int(nranks), int(rank)), "ba_comm_init")

    def comm_init_host(self, allreduce, nranks: int, rank: int):
        """Host-staged transport for the multi-rank exchange (test hook, see
        ba_comm_init_host): `allreduce(values: np.ndarray, op: str)` reduces the
        float64 array in place across the ranks ("sum" / "max")."""
        def cb(_user, ptr, n, op):
            try:
                allreduce(np.ctypeslib.as_array(ptr, shape=(int(n),)), "max" if op == 1 else "sum")
                return 0
            except Exception:   # noqa: BLE001 - reported as BA_ERR_COMM
                return 1
        self._host_cb = N.HOST_ALLREDUCE_FN(cb)   # kept alive with the solver
        self._check(self.lib.ba_comm_init_host(self.h, C.cast(self._host_cb, C.c_void_p), None, int(nranks),
                                               int(rank)), "ba_comm_init_host")

    def allreduce_host(self, values, op: str = "sum") -> np.ndarray:
        """In-place RCCL reduction of a few host doubles across ranks (identity
        without a communicator)."""
        v = np.ascontiguousarray(values, dtype=np.float64).copy()
        self._check(self.lib.ba_comm_allreduce_host(self.h, _ptr(v), int(v.size), 0 if op == "sum" else 1),
                    "ba_comm_allreduce_host")
        return v

    def barrier(self):
        self._check(self.lib.ba_comm_allreduce_host(self.h, None, 0, 0), "ba_comm_allreduce_host")

    # -- problem ----------------------------------------------------------
    def set_problem(self, problem: Problem):
        p = problem.normalized()
        s = N.ba_problem()
        s.n_cams, s.n_pts, s.n_obs = p.n_cams, p.n_pts, p.n_obs
        s.cams, s.K, s.pts = _ptr(p.cams), _ptr(p.K), _ptr(p.pts)
        s.cam_fixed, s.cam_fixed_extr, s.pt_fixed = _ptr(p.cam_fixed), _ptr(p.cam_fixed_extr), _ptr(p.pt_fixed)
        s.obs_cam, s.obs_pt, s.obs_uv = _ptr(p.obs_cam), _ptr(p.obs_pt), _ptr(p.obs_uv)
        s.huber_a = p.huber_a
        self._check(self.lib.ba_set_problem(self.h, C.byref(s)), "ba_set_problem")
        self.problem = p

    def set_params(self, cams: np.ndarray | None, pts: np.ndarray | None):
        c = None if cams is None else np.ascontiguousarray(cams, np.float64)
        q = None if pts is None else np.ascontiguousarray(pts, np.float64)
        self._check(self.lib.ba_set_params(self.h, _ptr(c), _ptr(q)), "ba_set_params")

    def solve(self, options: Options | None = None) -> Summary:
        o = (options or Options()).to_c()
        s = N.ba_summary()
        self._check(self.lib.ba_solve(self.h, C.byref(o), C.byref(s)), "ba_solve")
        return Summary(s.initial_cost, s.final_cost, s.num_iterations, s.num_successful_steps,
                       s.num_unsuccessful_steps, N.TERMINATION_NAMES.get(s.termination_type, str(s.termination_type)),
                       s.total_time_s, s.linearize_time_s, s.solve_time_s)

    def params(self) -> tuple[np.ndarray, np.ndarray]:
        p = self.problem
        cams = np.empty((p.n_cams, 6))
        pts = np.empty((p.n_pts, 3))
        self._check(self.lib.ba_get_params(self.h, _ptr(cams), _ptr(pts)), "ba_get_params")
        return cams, pts

    def iteration_log(self) -> list[dict]:
        n = self.lib.ba_get_iteration_log(self.h, None, 0)
        arr = (N.ba_iteration * max(n, 1))()
        self.lib.ba_get_iteration_log(self.h, arr, n)
        return [{f: getattr(arr[i], f) for f in ITER_FIELDS} for i in range(n)]

    def residuals(self) -> tuple[np.ndarray, float]:
        r = np.empty((self.problem.n_obs, 2))
        cost = C.c_double()
        self._check(self.lib.ba_eval_residuals(self.h, _ptr(r), C.byref(cost)), "ba_eval_residuals")
        return r, cost.value

    def linearize(self) -> tuple[np.ndarray, np.ndarray, float]:
        n = self.problem.n_obs
        r = np.empty((n, 2))
        J = np.empty((n, 2, 9))
        cost = C.c_double()
        self._check(self.lib.ba_linearize(self.h, _ptr(r), _ptr(J), C.byref(cost)), "ba_linearize")
        return r, J, cost.value

    def debug_blocks(self, radius: float = 1e4, with_s: bool = True) -> dict:
        """The blocks of one DENSE_SCHUR step at the current parameters
        (iteration-0 Jacobi scaling, trust-region radius `radius`), as the
        solve's own kernels form them (ba_debug_blocks): Hpp [n_pts, 6], gp
        [n_pts, 3], Hcc [n_cams, 21] (lower, row-major), gc [n_cams, 6], and
        with_s: the reduced system S [n, n] (lower triangle) and rhs [n]."""
        p = self.problem
        Hpp, gp = np.empty((p.n_pts, 6)), np.empty((p.n_pts, 3))
        Hcc, gc = np.empty((p.n_cams, 21)), np.empty((p.n_cams, 6))
        n = C.c_int(0)
        if with_s:   # size of the variable-camera system: ask first (S, rhs NULL)
            self._check(self.lib.ba_debug_blocks(self.h, float(radius), None, None, None, None, None, None,
                                                 C.byref(n)), "ba_debug_blocks")
        S = np.empty((n.value, n.value)) if with_s else None
        rhs = np.empty(n.value) if with_s else None
        self._check(self.lib.ba_debug_blocks(self.h, float(radius), _ptr(Hpp), _ptr(gp), _ptr(Hcc), _ptr(gc),
                                             _ptr(S) if with_s else None, _ptr(rhs) if with_s else None,
                                             C.byref(n)), "ba_debug_blocks")
        return {"Hpp": Hpp, "gp": gp, "Hcc": Hcc, "gc": gc, "S": S, "rhs": rhs, "n": n.value}

    def debug_plan(self) -> dict:
        """The dispatch decisions the host made for the current problem as of
        the last solve / debug_blocks (ba_debug_plan: host state only, nothing
        built or launched): N.DEBUG_PLAN_FIELDS as a dict of ints."""
        out = (C.c_int32 * len(N.DEBUG_PLAN_FIELDS))()
        self._check(self.lib.ba_debug_plan(self.h, out, len(out)), "ba_debug_plan")
        return dict(zip(N.DEBUG_PLAN_FIELDS, (int(v) for v in out)))

    def reduced_order(self) -> int:
        """Order n of the current problem's reduced camera system: 6 x the
        variable cameras that have an observation."""
        p = self.problem
        used = np.zeros(p.n_cams, bool)
        used[p.obs_cam] = True
        if p.cam_fixed is not None:
            used &= np.asarray(p.cam_fixed) == 0
        return 6 * int(used.sum())

    def debug_factor(self, S, rhs) -> dict:
        """The DENSE_SCHUR factorisation + back substitution of a solve's step
        on a caller-supplied system of the current problem's order
        (ba_debug_factor; the form is the one the order and the BA_CHOL_*
        knobs select).  S [n, n] (lower triangle read), rhs [n].  Returns L
        [n + 1, n] (rows < n: the factor's tiles left of the diagonal
        64-blocks, which the kernels never store: zeros there; row n: z =
        L^-1 rhs), V [T, 64, 64] (the inverses of the diagonal blocks), y [n]
        (the solution), ok (False: a non-positive pivot was reported) and n."""
        n = self.reduced_order()
        S = np.ascontiguousarray(S, dtype=np.float64)
        rhs = np.ascontiguousarray(rhs, dtype=np.float64)
        if S.shape != (n, n) or rhs.shape != (n,):
            raise ValueError(f"debug_factor: the problem's reduced system has order {n}, got S {S.shape}, "
                             f"rhs {rhs.shape}")
        T = (n + 63) // 64
        L, V, y = np.empty((n + 1, n)), np.empty((T, 64, 64)), np.empty(n)
        ok = C.c_int(0)
        self._check(self.lib.ba_debug_factor(self.h, _ptr(S), _ptr(rhs), _ptr(L), _ptr(V), _ptr(y), C.byref(ok)),
                    "ba_debug_factor")
        return {"L": L, "V": V, "y": y, "ok": bool(ok.value), "n": n}

    def covariance(self, cam_pairs=None, points=None) -> tuple[np.ndarray, np.ndarray]:
        """Marginal covariances at the current parameters (ba_covariance:
        ceres::Covariance with its defaults, (J^T J)^-1 over the variable
        blocks, no damping).  cam_pairs [m, 2]: camera index pairs (i, j), any
        order; None: every (i, i).  points [k]: point indices; None: none.
        Returns (cam_cov [m, 6, 6] with cam_cov[q] = Cov(cam_i, cam_j),
        pt_cov [k, 3, 3]); blocks of constant cameras / points are zero.
        Raises BAError (BA_ERR_SINGULAR when the system is not positive
        definite: the caller must have removed the gauge)."""
        if cam_pairs is None:
            i = np.arange(self.problem.n_cams, dtype=np.int32)
            cam_pairs = np.stack([i, i], axis=1)
        cp = np.ascontiguousarray(cam_pairs, dtype=np.int32).reshape(-1, 2)
        pt = np.ascontiguousarray(points if points is not None else [], dtype=np.int32).reshape(-1)
        cam_cov = np.empty((cp.shape[0], 6, 6))
        pt_cov = np.empty((pt.size, 3, 3))
        req = N.ba_covariance_request(n_cam_pairs=cp.shape[0], n_points=pt.size, cam_pairs=_ptr(cp),
                                      cam_cov=_ptr(cam_cov), points=_ptr(pt), pt_cov=_ptr(pt_cov))
        self._check(self.lib.ba_covariance(self.h, C.byref(req)), "ba_covariance")
        return cam_cov, pt_cov

    def covariance_ex(self, cam_pairs=None, points=None, cam_pt=None, pt_pairs=None, leverage_obs=None) -> dict:
        """Any covariance block and observation leverages from one
        factorisation (ba_covariance_ex).  cam_pairs [m, 2] and points [k] as
        in covariance(), except that None requests nothing; cam_pt [a, 2]:
        (camera, point) pairs; pt_pairs [b, 2]: point pairs (p, q), p == q
        allowed; leverage_obs [l]: observation indices, or "all" for every
        observation in the problem's order.  Returns a dict of arrays:
        cam_cov [m, 6, 6], pt_cov [k, 3, 3], cam_pt_cov [a, 6, 3] =
        Cov(cam, pt), pt_pt_cov [b, 3, 3] = Cov(p, q), leverage [l, 2, 2] =
        J_o Sigma J_o^T.  Blocks of constant cameras / points are zero."""
        def idx(a, cols):
            a = np.ascontiguousarray(a if a is not None else [], dtype=np.int32)
            return a.reshape(-1, cols) if cols > 1 else a.reshape(-1)
        cp, pt, cq, pq = idx(cam_pairs, 2), idx(points, 1), idx(cam_pt, 2), idx(pt_pairs, 2)
        every = isinstance(leverage_obs, str)
        if every and leverage_obs != "all":
            raise ValueError(f"covariance_ex: leverage_obs = {leverage_obs!r}")
        lo = None if every else idx(leverage_obs, 1)
        n_lev = self.problem.n_obs if every else lo.size
        out = {"cam_cov": np.empty((cp.shape[0], 6, 6)), "pt_cov": np.empty((pt.size, 3, 3)),
               "cam_pt_cov": np.empty((cq.shape[0], 6, 3)), "pt_pt_cov": np.empty((pq.shape[0], 3, 3)),
               "leverage": np.empty((n_lev, 2, 2))}
        base = N.ba_covariance_request(n_cam_pairs=cp.shape[0], n_points=pt.size, cam_pairs=_ptr(cp),
                                       cam_cov=_ptr(out["cam_cov"]), points=_ptr(pt), pt_cov=_ptr(out["pt_cov"]))
        req = N.ba_covariance_request_ex(base=base, n_cam_pt=cq.shape[0], n_pt_pairs=pq.shape[0], cam_pt=_ptr(cq),
                                         cam_pt_cov=_ptr(out["cam_pt_cov"]), pt_pairs=_ptr(pq),
                                         pt_pt_cov=_ptr(out["pt_pt_cov"]), n_lev=n_lev, reserved=0,
                                         lev_obs=_ptr(lo), leverage=_ptr(out["leverage"]))
        self._check(self.lib.ba_covariance_ex(self.h, C.byref(req)), "ba_covariance_ex")
        return out

    def covariance_iterative(self, cam_pairs=None, points=None, *, preconditioner: str = "schur_jacobi",
                             max_iterations: int = 500, tolerance: float = 1e-10
                             ) -> tuple[np.ndarray, np.ndarray, dict]:
        """covariance()'s request without the dense factor
        (ba_covariance_iterative): the blocks come from block columns of the
        inverse reduced camera system, each column solved by preconditioned
        conjugate gradients on the implicit system until |r|_2 <= tolerance
        or max_iterations.  Serves problems too large for DENSE_SCHUR.
        cam_pairs / points as in covariance(); preconditioner "jacobi" or
        "schur_jacobi".  Returns (cam_cov [m, 6, 6], pt_cov [k, 3, 3], info)
        with info: n_columns, n_converged, max_iterations_used, max_residual
        (the largest true |e - S x|_2 over the columns) and ms (device time
        of setup, CG, residual check + gathers, copies).  A column that does
        not converge is reported in info, not raised."""
        kinds = {"jacobi": 0, "schur_jacobi": 1}
        if preconditioner not in kinds:
            raise ValueError(f"covariance_iterative: preconditioner = {preconditioner!r}")
        if cam_pairs is None:
            i = np.arange(self.problem.n_cams, dtype=np.int32)
            cam_pairs = np.stack([i, i], axis=1)
        cp = np.ascontiguousarray(cam_pairs, dtype=np.int32).reshape(-1, 2)
        pt = np.ascontiguousarray(points if points is not None else [], dtype=np.int32).reshape(-1)
        cam_cov = np.empty((cp.shape[0], 6, 6))
        pt_cov = np.empty((pt.size, 3, 3))
        req = N.ba_covariance_request(n_cam_pairs=cp.shape[0], n_points=pt.size, cam_pairs=_ptr(cp),
                                      cam_cov=_ptr(cam_cov), points=_ptr(pt), pt_cov=_ptr(pt_cov))
        opt = N.ba_cov_iter_options(preconditioner_type=kinds[preconditioner], max_iterations=int(max_iterations),
                                    tolerance=float(tolerance))
        info = N.ba_cov_iter_info()
        self._check(self.lib.ba_covariance_iterative(self.h, C.byref(req), C.byref(opt), C.byref(info)),
                    "ba_covariance_iterative")
        return cam_cov, pt_cov, {"n_columns": info.n_columns, "n_converged": info.n_converged,
                                 "max_iterations_used": info.max_iterations_used,
                                 "max_residual": info.max_residual, "ms": [float(x) for x in info.ms]}

    def covariance_iterative_bench(self, cols: int, reps: int = 20, warmup: int = 3) -> np.ndarray:
        """Device time (ms) of `reps` implicit matvecs on covariance_iterative's
        W records: cols = 0 the single-vector matvec of ITERATIVE_SCHUR, cols =
        1, 2, 4 the multi-column one with that many column cameras
        (ba_covariance_iterative_bench).  Diagnostic."""
        ms = np.empty(int(reps))
        self._check(self.lib.ba_covariance_iterative_bench(self.h, int(cols), int(reps), int(warmup), _ptr(ms)),
                    "ba_covariance_iterative_bench")
        return ms

    def covariance_times(self) -> np.ndarray:
        """Device time (ms) of the phases of the last covariance() / covariance_ex() call:
        linearisation + reduced system, factorisation, inverse, gathers."""
        return self._times(self.lib.ba_covariance_times)

    def prune(self, extr, cam_center, K, obs_cam, obs_X, obs_uv, obs_inv_sigma, obs_dist) -> np.ndarray:
        """pruneCorrespondences (Optimizer.cpp:6-79) on the device for a batch of
        (keyframe, keypoint) pairs; returns a uint8 ba_prune_result per pair."""
        arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in (extr, cam_center, K)]
        oc = np.ascontiguousarray(obs_cam, dtype=np.int32)
        oarrs = [np.ascontiguousarray(a, dtype=np.float32) for a in (obs_X, obs_uv, obs_inv_sigma, obs_dist)]
        n_cams, n_obs = arrs[0].size // 16, oc.size
        pp = N.ba_prune_problem(n_cams=n_cams, n_obs=n_obs, extr=_ptr(arrs[0]), cam_center=_ptr(arrs[1]),
                                K=_ptr(arrs[2]), obs_cam=_ptr(oc), obs_X=_ptr(oarrs[0]), obs_uv=_ptr(oarrs[1]),
                                obs_inv_sigma=_ptr(oarrs[2]), obs_dist=_ptr(oarrs[3]))
        out = np.empty(n_obs, np.uint8)
        self._check(self.lib.ba_prune(self.h, C.byref(pp), _ptr(out)), "ba_prune")
        return out

    def solve_pose_batch(self, obs_offset, cams, K, pts, obs_uv, options: Options | None = None,
                         huber_a: float = HUBER_A) -> tuple[np.ndarray, list[Summary]]:
        """Batched pose-only solves (MotionOnlyBAOptimizerAngles' Ceres solve,
        Optimizer.cpp:417-442, for many frames in one launch).  Problem i owns
        observations [obs_offset[i], obs_offset[i+1]) of constant points
        pts[o] with pixels obs_uv[o]; returns (cams (n, 6), summaries)."""
        off = np.ascontiguousarray(obs_offset, dtype=np.int32)
        n = off.size - 1
        c = np.ascontiguousarray(cams, dtype=np.float64).reshape(n, 6)
        k = np.ascontiguousarray(K, dtype=np.float32).reshape(n, 9)
        x = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        uv = np.ascontiguousarray(obs_uv, dtype=np.float32).reshape(-1, 2)
        b = N.ba_pose_batch(n_problems=n, reserved=0, obs_offset=_ptr(off), cams=_ptr(c), K=_ptr(k), pts=_ptr(x),
                            obs_uv=_ptr(uv), huber_a=float(huber_a))
        o = (options or Options()).to_c()
        out = np.empty((n, 6))
        sums = (N.ba_summary * max(n, 1))()
        self._check(self.lib.ba_solve_pose_batch(self.h, C.byref(b), C.byref(o), _ptr(out), sums),
                    "ba_solve_pose_batch")
        res = [Summary(s.initial_cost, s.final_cost, s.num_iterations, s.num_successful_steps,
                       s.num_unsuccessful_steps, N.TERMINATION_NAMES.get(s.termination_type, str(s.termination_type)),
                       s.total_time_s, s.linearize_time_s, s.solve_time_s) for s in list(sums)[:n]]
        return out, res

    def solve_window_batch(self, problems, options: Options | None = None
                           ) -> tuple[list[tuple[np.ndarray, np.ndarray]], list[Summary]]:
        """Many independent small problems (variable cameras and points, at
        most BA_WINDOW_MAX_CAMS variable observed cameras each) with solve()'s
        DENSE_SCHUR semantics, the whole LM loop of each problem in one kernel
        launch (ba_solve_window_batch).  `problems`: a list of Problem (packed
        with pack_window_batch) or a WindowBatch.  Returns ([(cams, pts) per
        problem], summaries); window_iteration_log(i) has problem i's log."""
        b = problems if isinstance(problems, WindowBatch) else pack_window_batch(list(problems))
        n = b.n_problems
        w = N.ba_window_batch(
            n_problems=n, reserved=0, cam_offset=_ptr(b.cam_offset), pt_offset=_ptr(b.pt_offset),
            obs_offset=_ptr(b.obs_offset), cams=_ptr(b.cams), cam_fixed=_ptr(b.cam_fixed),
            cam_fixed_extr=_ptr(b.cam_fixed_extr), K=_ptr(b.K), pts=_ptr(b.pts), pt_fixed=_ptr(b.pt_fixed),
            obs_cam=_ptr(b.obs_cam), obs_pt=_ptr(b.obs_pt), obs_uv=_ptr(b.obs_uv), huber_a=float(b.huber_a))
        o = (options or Options()).to_c()
        cams = np.empty_like(b.cams)
        pts = np.empty_like(b.pts)
        sums = (N.ba_summary * max(n, 1))()
        self._check(self.lib.ba_solve_window_batch(self.h, C.byref(w), C.byref(o), _ptr(cams), _ptr(pts), sums),
                    "ba_solve_window_batch")
        co, po = b.cam_offset, b.pt_offset
        out = [(cams[co[i]:co[i + 1]].copy(), pts[po[i]:po[i + 1]].copy()) for i in range(n)]
        res = [Summary(s.initial_cost, s.final_cost, s.num_iterations, s.num_successful_steps,
                       s.num_unsuccessful_steps, N.TERMINATION_NAMES.get(s.termination_type, str(s.termination_type)),
                       s.total_time_s, s.linearize_time_s, s.solve_time_s) for s in list(sums)[:n]]
        return out, res

    def window_iteration_log(self, i: int) -> list[dict]:
        """Iteration log of problem i of the last solve_window_batch."""
        n = self.lib.ba_get_window_iteration_log(self.h, int(i), None, 0)
        if n < 0:
            raise N.BAError(-n, f"ba_get_window_iteration_log: no problem {i} in the last batch")
        arr = (N.ba_iteration * max(n, 1))()
        self.lib.ba_get_window_iteration_log(self.h, int(i), arr, n)
        return [{f: getattr(arr[k], f) for f in ITER_FIELDS} for k in range(n)]

    def window_times(self) -> np.ndarray:
        """Times (ms) of the last solve_window_batch: host preparation (wall),
        the kernel (device), the whole call (wall)."""
        return self._times(self.lib.ba_window_times)

    def triangulate(self, extr, K, obs_offset, obs_cam, obs_uv, *, cam_center=None, obs_scale=None, pts_init=None,
                    refine: bool = False, options: Options | None = None, huber_a: float = HUBER_A,
                    min_views: int = 2, checks: int = N.TRI_CHECK_ALL, behind_rule: int = 0, init: int | None = None,
                    with_summaries: bool | None = None
                    ) -> tuple[np.ndarray, np.ndarray, list[Summary] | None]:
        """Batched multi-view triangulation (ba_triangulate): SfMHelper::
        triangulatePoints for any number of views per point, optionally with a
        per-point LM refinement against the constant cameras, in one launch.
        extr [C, 16] (col-major world->camera), K [C, 9]; point p owns
        observations [obs_offset[p], obs_offset[p+1]) of obs_cam / obs_uv;
        cam_center [C, 3] and obs_scale [N] (1.2^octave; None: all 1) feed the
        scale test, pts_init [P, 3] starts from the caller's points instead of
        the DLT (init overrides the choice: N.TRI_INIT_DLT / TRI_INIT_GIVEN).
        checks: N.TRI_CHECK_* bits; behind_rule 0: behind every camera (the
        reference's), 1: behind any.  Returns (pts [P, 3] float64, status [P]
        uint8 (N.TRI_*), summaries or None); summaries default to refine."""
        e = np.ascontiguousarray(extr, dtype=np.float32).reshape(-1, 16)
        k = np.ascontiguousarray(K, dtype=np.float32).reshape(-1, 9)
        off = np.ascontiguousarray(obs_offset, dtype=np.int32).reshape(-1)
        oc = np.ascontiguousarray(obs_cam, dtype=np.int32).reshape(-1)
        uv = np.ascontiguousarray(obs_uv, dtype=np.float32).reshape(-1, 2)
        ctr = None if cam_center is None else np.ascontiguousarray(cam_center, dtype=np.float32).reshape(-1, 3)
        sc = None if obs_scale is None else np.ascontiguousarray(obs_scale, dtype=np.float32).reshape(-1)
        x0 = None if pts_init is None else np.ascontiguousarray(pts_init, dtype=np.float64).reshape(-1, 3)
        n = max(off.size - 1, 0)
        if k.shape[0] != e.shape[0] or (ctr is not None and ctr.shape[0] != e.shape[0]):
            raise ValueError("triangulate: extr, K and cam_center disagree on the number of cameras")
        if uv.shape[0] != oc.size or (sc is not None and sc.size != oc.size) or (n and off[-1] > oc.size):
            raise ValueError("triangulate: obs_cam, obs_uv, obs_scale and obs_offset disagree on the number of observations")
        if x0 is not None and x0.shape[0] != n:
            raise ValueError("triangulate: pts_init must have one row per point")
        b = N.ba_tri_batch(n_cams=e.shape[0], n_pts=n, extr=_ptr(e), cam_center=_ptr(ctr), K=_ptr(k),
                           obs_offset=_ptr(off), obs_cam=_ptr(oc), obs_uv=_ptr(uv), obs_scale=_ptr(sc),
                           pts_init=_ptr(x0), huber_a=float(huber_a))
        if init is None:
            init = N.TRI_INIT_GIVEN if x0 is not None else N.TRI_INIT_DLT
        t = N.ba_tri_options(init=int(init), refine=int(refine), min_views=int(min_views), checks=int(checks),
                             behind_rule=int(behind_rule), reserved=0)
        o = (options or Options()).to_c()
        pts = np.zeros((n, 3))
        status = np.zeros(n, np.uint8)
        want = bool(refine) if with_summaries is None else bool(with_summaries)
        sums = (N.ba_summary * max(n, 1))() if want else None
        self._check(self.lib.ba_triangulate(self.h, C.byref(b), C.byref(t), C.byref(o), _ptr(pts), _ptr(status), sums),
                    "ba_triangulate")
        res = None
        if want:
            res = [Summary(s.initial_cost, s.final_cost, s.num_iterations, s.num_successful_steps,
                           s.num_unsuccessful_steps,
                           N.TERMINATION_NAMES.get(s.termination_type, str(s.termination_type)),
                           s.total_time_s, s.linearize_time_s, s.solve_time_s) for s in list(sums)[:n]]
        return pts, status, res

    def triangulate_times(self) -> np.ndarray:
        """Times (ms) of the last triangulate: host preparation (wall), the
        kernels (device), the whole call (wall)."""
        return self._times(self.lib.ba_triangulate_times)

    # -- robust absolute pose ---------------------------------------------
    def _pnp_batch(self, obs_offset, cams, K, pts, obs_uv, huber_a, pnp_options):
        off = np.ascontiguousarray(obs_offset, dtype=np.int32).reshape(-1)
        n = max(off.size - 1, 0)
        c = None if cams is None else np.ascontiguousarray(cams, dtype=np.float64).reshape(n, 6)
        k = np.ascontiguousarray(K, dtype=np.float32).reshape(n, 9)
        x = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
        uv = np.ascontiguousarray(obs_uv, dtype=np.float32).reshape(-1, 2)
        if x.shape[0] != uv.shape[0] or (n and off[-1] > uv.shape[0]):
            raise ValueError("pnp: pts, obs_uv and obs_offset disagree on the number of observations")
        b = N.ba_pose_batch(n_problems=n, reserved=0, obs_offset=_ptr(off), cams=_ptr(c), K=_ptr(k), pts=_ptr(x),
                            obs_uv=_ptr(uv), huber_a=float(huber_a))
        p = N.ba_pnp_options()
        self.lib.ba_pnp_defaults(C.byref(p))
        self._set_options(p, pnp_options, {f: float if f == "threshold_px" else int for f in PNP_OPTION_FIELDS}, "pnp")
        return b, p, n, uv.shape[0], (off, c, k, x, uv)

    def pnp_ransac(self, obs_offset, cams, K, pts, obs_uv, *, options: Options | None = None,
                   huber_a: float = HUBER_A, **pnp_options
                   ) -> tuple[np.ndarray, np.ndarray, list[PnpResult]]:
        """Batched robust absolute pose (ba_pnp_ransac): P3P RANSAC on the
        device, the whole hypothesis budget scored in parallel, then the pose
        LM of solve_pose_batch on the consensus set.  The arguments are
        solve_pose_batch's; cams is the prior (None with use_prior=0).
        pnp_options: max_hypotheses, min_points, min_inliers, use_prior,
        refine, seed, threshold_px (defaults: ba_pnp_defaults); options: the
        LM's.  Returns (cams (n, 6), inlier mask (n_obs,) bool in caller
        order, results)."""
        b, p, n, n_obs, _keep = self._pnp_batch(obs_offset, cams, K, pts, obs_uv, huber_a, pnp_options)
        o = (options or Options()).to_c()
        out = np.zeros((n, 6))
        inl = np.zeros(n_obs, np.uint8)
        res = (N.ba_pnp_result * max(n, 1))()
        self._check(self.lib.ba_pnp_ransac(self.h, C.byref(b), C.byref(p), C.byref(o), _ptr(out), _ptr(inl), res),
                    "ba_pnp_ransac")
        results = []
        for r in list(res)[:n]:
            s = r.refine
            results.append(PnpResult(
                r.status, r.n_inliers, r.n_inliers_ransac, r.best_hypothesis, np.array(r.cam_ransac[:]),
                Summary(s.initial_cost, s.final_cost, s.num_iterations, s.num_successful_steps,
                        s.num_unsuccessful_steps, N.TERMINATION_NAMES.get(s.termination_type, str(s.termination_type)),
                        s.total_time_s, s.linearize_time_s, s.solve_time_s)))
        return out, inl.astype(bool), results

    def pnp_hypotheses(self, obs_offset, cams, K, pts, obs_uv, problem: int, h0: int, n: int, **pnp_options) -> dict:
        """Hypotheses h0 .. h0+n-1 of one problem exactly as pnp_ransac forms
        and scores them (ba_pnp_hypotheses): sample (n, 3) local observation
        indices (-1: the prior), n_sol (n,), R (n, 4, 3, 3), t (n, 4, 3) and
        count (n, 4), solutions in their fixed order."""
        b, p, _n, _no, _keep = self._pnp_batch(obs_offset, cams, K, pts, obs_uv, 0.0, pnp_options)
        m = max(int(n), 0)
        sample = np.zeros((m, 3), np.int32)
        n_sol = np.zeros(m, np.int32)
        Rt = np.zeros((m, 4, 12))
        count = np.zeros((m, 4), np.int32)
        self._check(self.lib.ba_pnp_hypotheses(self.h, C.byref(b), C.byref(p), int(problem), int(h0), int(n),
                                               _ptr(sample), _ptr(n_sol), _ptr(Rt), _ptr(count)), "ba_pnp_hypotheses")
        return {"sample": sample, "n_sol": n_sol, "R": Rt[:, :, :9].reshape(m, 4, 3, 3).copy(),
                "t": Rt[:, :, 9:].copy(), "count": count}

    def pnp_times(self) -> np.ndarray:
        """Times (ms) of the last pnp_ransac: host preparation (wall), the
        kernels (device), the whole call (wall)."""
        return self._times(self.lib.ba_pnp_times)

    # -- two-view relative pose -------------------------------------------
    def _two_view_batch(self, match_offset, K1, K2, uv1, uv2, tv_options):
        off = np.ascontiguousarray(match_offset, dtype=np.int32).reshape(-1)
        n = max(off.size - 1, 0)
        k1 = np.ascontiguousarray(K1, dtype=np.float32).reshape(n, 9)
        k2 = None if K2 is None else np.ascontiguousarray(K2, dtype=np.float32).reshape(n, 9)
        a = np.ascontiguousarray(uv1, dtype=np.float32).reshape(-1, 2)
        b2 = np.ascontiguousarray(uv2, dtype=np.float32).reshape(-1, 2)
        if a.shape[0] != b2.shape[0] or (n and off[-1] > a.shape[0]):
            raise ValueError("two_view: uv1, uv2 and match_offset disagree on the number of matches")
        b = N.ba_two_view_batch(n_pairs=n, reserved=0, match_offset=_ptr(off), K1=_ptr(k1), K2=_ptr(k2), uv1=_ptr(a),
                                uv2=_ptr(b2))
        p = N.ba_two_view_options()
        self.lib.ba_two_view_defaults(C.byref(p))
        for key, val in tv_options.items():
            if key == "e_solver":                       # the C member keeps the name `reserved`
                p.reserved = int(val)
                continue
            if key not in TV_OPTION_FIELDS:
                raise TypeError(f"two_view: unknown option {key!r}")
            setattr(p, key, float(val) if key in ("threshold_px", "h_ratio") else int(val))
        return b, p, n, a.shape[0], (off, k1, k2, a, b2)

    def two_view_ransac(self, match_offset, K1, K2, uv1, uv2, **tv_options
                        ) -> tuple[np.ndarray, list[TwoViewResult]]:
        """Batched two-view relative pose (ba_two_view_ransac): E and H RANSAC
        on the device, the reference's model choice, decomposition and the
        positive-depth vote.  Pair i owns matches match_offset[i] ..
        match_offset[i+1]; K1 / K2 (n, 9) col-major (K2 None: K1); uv1 / uv2
        (n_matches, 2) float32 pixels.  tv_options: max_hypotheses,
        min_points, min_inliers, min_good, model, seed, threshold_px, h_ratio,
        e_solver (N.TV_E_EIGHT_POINT, the default, or N.TV_E_FIVE_POINT)
        (defaults: ba_two_view_defaults).  Returns (inlier mask (n_matches,)
        bool, results)."""
        b, p, n, nm, _keep = self._two_view_batch(match_offset, K1, K2, uv1, uv2, tv_options)
        inl = np.zeros(nm, np.uint8)
        res = (N.ba_two_view_result * max(n, 1))()
        self._check(self.lib.ba_two_view_ransac(self.h, C.byref(b), C.byref(p), _ptr(inl), res), "ba_two_view_ransac")
        results = [TwoViewResult(r.status, r.model, r.n_inliers, r.n_good, r.n_good_second, r.best_hypothesis_e,
                                 r.best_hypothesis_h, r.votes_e, r.votes_h, r.score_e, r.score_h,
                                 np.array(r.E[:]).reshape(3, 3), np.array(r.H[:]).reshape(3, 3), np.array(r.cam[:]),
                                 np.array(r.normal[:]), r.reserved) for r in list(res)[:n]]
        return inl.astype(bool), results

    def two_view_hypotheses(self, match_offset, K1, K2, uv1, uv2, pair: int, h0: int, n: int, **tv_options) -> dict:
        """Hypotheses h0 .. h0+n-1 of one pair exactly as two_view_ransac forms
        and scores them (ba_two_view_hypotheses): sample (n, 8) local match
        indices, E and H (n, 3, 3), valid and count (n, 2) as (E, H)."""
        b, p, _n, _nm, _keep = self._two_view_batch(match_offset, K1, K2, uv1, uv2, tv_options)
        m = max(int(n), 0)
        sample = np.zeros((m, 8), np.int32)
        E = np.zeros((m, 3, 3))
        H = np.zeros((m, 3, 3))
        valid = np.zeros((m, 2), np.int32)
        count = np.zeros((m, 2), np.int32)
        self._check(self.lib.ba_two_view_hypotheses(self.h, C.byref(b), C.byref(p), int(pair), int(h0), int(n),
                                                    _ptr(sample), _ptr(E), _ptr(H), _ptr(valid), _ptr(count)),
                    "ba_two_view_hypotheses")
        return {"sample": sample, "E": E, "H": H, "valid": valid, "count": count}

    def two_view_hypotheses_e5(self, match_offset, K1, K2, uv1, uv2, pair: int, h0: int, n: int, **tv_options) -> dict:
        """Hypotheses h0 .. h0+n-1 of one pair exactly as two_view_ransac forms
        and scores them with e_solver = N.TV_E_FIVE_POINT
        (ba_two_view_hypotheses_e5): sample (n, 8) local match indices (the
        first five are used), n_sol (n,), E (n, 10, 3, 3) with zeros past
        n_sol, count (n, 10)."""
        b, p, _n, _nm, _keep = self._two_view_batch(match_offset, K1, K2, uv1, uv2, tv_options)
        m = max(int(n), 0)
        sample = np.zeros((m, 8), np.int32)
        n_sol = np.zeros(m, np.int32)
        E = np.zeros((m, 10, 3, 3))
        count = np.zeros((m, 10), np.int32)
        self._check(self.lib.ba_two_view_hypotheses_e5(self.h, C.byref(b), C.byref(p), int(pair), int(h0), int(n),
                                                       _ptr(sample), _ptr(n_sol), _ptr(E), _ptr(count)),
                    "ba_two_view_hypotheses_e5")
        return {"sample": sample, "n_sol": n_sol, "E": E, "count": count}

    def two_view_times(self) -> np.ndarray:
        """Times (ms) of the last two_view_ransac: host preparation (wall), the
        kernels (device), the whole call (wall)."""
        return self._times(self.lib.ba_two_view_times)

    # -- descriptor matching ------------------------------------------------
    def _match_batch(self, batch: MatchBatch):
        mb = batch
        pq = np.ascontiguousarray(mb.pairs[:, 0])
        pt = np.ascontiguousarray(mb.pairs[:, 1])
        b = N.ba_match_batch(dim=int(mb.dim), n_sets=mb.set_offset.size - 1, n_pairs=mb.pairs.shape[0],
                             n_ref=0 if mb.ref_desc is None else mb.ref_desc.shape[0], set_offset=_ptr(mb.set_offset),
                             desc=_ptr(mb.desc), pair_query=_ptr(pq), pair_train=_ptr(pt), row_ref=_ptr(mb.row_ref),
                             ref_desc=_ptr(mb.ref_desc))
        return b, (pq, pt, mb)

    def match_descriptors(self, sets, pairs=None, row_ref=None, ref_desc=None, **match_options
                          ) -> tuple[np.ndarray, np.ndarray]:
        """Batched descriptor matching (ba_match_descriptors): the exact 2-NN
        of every query, Lowe's ratio test and the one-match-per-train filter,
        on the device.  sets: a MatchBatch, or a list of (n_s, dim) float32
        descriptor arrays with pairs (P, 2) of (query set, train set) indices
        (row_ref / ref_desc: pack_match_batch).  match_options: ratio, unique,
        max_distance (defaults: ba_match_defaults).  Returns (match_offset
        (P + 1,) int32, matches: a MATCH_DTYPE record array); pair i owns
        matches[match_offset[i]:match_offset[i+1]], in increasing (train,
        query)."""
        mb = sets if isinstance(sets, MatchBatch) else pack_match_batch(sets, pairs, row_ref, ref_desc)
        b, _keep = self._match_batch(mb)
        p = N.ba_match_options()
        self.lib.ba_match_defaults(C.byref(p))
        self._set_options(p, match_options, {"ratio": float, "unique": int, "max_distance": float}, "match_descriptors")
        cap = 0
        if mb.pairs.size and mb.set_offset.size > 1:      # (a bad index or offset is the library's to report)
            n = np.maximum(np.diff(mb.set_offset.astype(np.int64)), 0)
            nq, nt = (n[np.clip(mb.pairs[:, k], 0, n.size - 1)] for k in (0, 1))
            cap = int((np.minimum(nq, nt) if p.unique else nq).sum())
        off = np.zeros(mb.pairs.shape[0] + 1, np.int32)
        out = np.zeros(max(cap, 1), MATCH_DTYPE)
        self._check(self.lib.ba_match_descriptors(self.h, C.byref(b), C.byref(p), _ptr(off), _ptr(out)),
                    "ba_match_descriptors")
        return off, out[:int(off[-1])].copy()

    def match_knn(self, sets, pairs=None, pair: int = 0) -> np.ndarray:
        """The dense 2-NN record of every query of one pair exactly as
        match_descriptors forms it, before any filtering (ba_match_knn): a
        MATCH_KNN_DTYPE record array (index -1 and d2 = inf: no neighbour)."""
        mb = sets if isinstance(sets, MatchBatch) else pack_match_batch(sets, pairs)
        b, _keep = self._match_batch(mb)
        nq = 0
        if 0 <= int(pair) < mb.pairs.shape[0]:
            s = int(mb.pairs[int(pair), 0])
            if 0 <= s < mb.set_offset.size - 1:
                nq = int(mb.set_offset[s + 1] - mb.set_offset[s])
        out = np.zeros(max(nq, 1), MATCH_KNN_DTYPE)
        self._check(self.lib.ba_match_knn(self.h, C.byref(b), int(pair), _ptr(out)), "ba_match_knn")
        return out[:nq].copy()

    def match_times(self) -> np.ndarray:
        """Times (ms) of the last match_descriptors: host preparation (wall),
        the kernels (device), the whole call (wall), then the kernels' phases:
        norms, the 2-NN contraction, merge / ratio / unique / compaction."""
        return self._times(self.lib.ba_match_times)

    # -- point-cloud ICP -------------------------------------------------------
    _ICP_ROUTES = {"AUTO": N.ICP_ROUTE_AUTO, "GRID": N.ICP_ROUTE_GRID, "BRUTE": N.ICP_ROUTE_BRUTE}
    _ICP_OPTIONS = {"max_iterations": int, "max_corr_dist": float, "mse_abs_eps": float, "mse_rel_eps": float,
                    "transformation_eps": float, "min_correspondences": int, "with_scale": int,
                    "fitness_max_range": float, "cell": float,
                    "route": lambda v: Solver._ICP_ROUTES[v] if isinstance(v, str) else int(v)}

    def _icp_batch(self, ib: IcpBatch, icp_options: dict, who: str):
        ps = np.ascontiguousarray(ib.pairs[:, 0])
        pt = np.ascontiguousarray(ib.pairs[:, 1])
        b = N.ba_icp_batch(n_sets=ib.set_offset.size - 1, n_pairs=ib.pairs.shape[0], set_offset=_ptr(ib.set_offset),
                           xyz=_ptr(ib.xyz), pair_src=_ptr(ps), pair_tgt=_ptr(pt), guess=_ptr(ib.guess))
        p = N.ba_icp_options()
        self.lib.ba_icp_defaults(C.byref(p))
        self._set_options(p, icp_options, self._ICP_OPTIONS, who)
        return b, p, (ps, pt, ib)

    def icp(self, sets, pairs=None, guess=None, **icp_options) -> tuple[np.ndarray, np.ndarray]:
        """Batched point-to-point ICP and its fitness score (ba_icp): exact
        nearest neighbours, the Umeyama step and PCL's convergence rules, on
        the device.  sets: an IcpBatch, or a list of (n_s, 3) float32 clouds
        with pairs (P, 2) of (source set, target set) indices and an optional
        guess (P, 4, 4).  icp_options: max_iterations, max_corr_dist,
        mse_abs_eps, mse_rel_eps, transformation_eps, min_correspondences,
        with_scale, fitness_max_range, route ("AUTO" / "GRID" / "BRUTE"), cell
        (defaults: ba_icp_defaults).  Returns (an ICP_RESULT_DTYPE record
        array (P,), mse (P, max_iterations))."""
        ib = sets if isinstance(sets, IcpBatch) else pack_icp_batch(sets, pairs, guess)
        b, p, _keep = self._icp_batch(ib, icp_options, "icp")
        n = ib.pairs.shape[0]
        out = np.zeros(max(n, 1), ICP_RESULT_DTYPE)
        mse = np.zeros((max(n, 1), max(int(p.max_iterations), 1)))
        self._check(self.lib.ba_icp(self.h, C.byref(b), C.byref(p), _ptr(out), _ptr(mse)), "ba_icp")
        return out[:n].copy(), mse[:n].copy()

    def icp_nn(self, sets, pairs=None, guess=None, pair: int = 0, **icp_options) -> tuple[np.ndarray, np.ndarray]:
        """One correspondence pass of one pair on guess * source through the
        route the options select (ba_icp_nn): (idx (n_src,) int32 with -1 for
        a point that is not kept, d2 (n_src,) float32)."""
        ib = sets if isinstance(sets, IcpBatch) else pack_icp_batch(sets, pairs, guess)
        b, p, _keep = self._icp_batch(ib, icp_options, "icp_nn")
        ns = 0
        if 0 <= int(pair) < ib.pairs.shape[0]:
            s = int(ib.pairs[int(pair), 0])
            if 0 <= s < ib.set_offset.size - 1:
                ns = max(int(ib.set_offset[s + 1] - ib.set_offset[s]), 0)
        idx = np.zeros(max(ns, 1), np.int32)
        d2 = np.zeros(max(ns, 1), np.float32)
        self._check(self.lib.ba_icp_nn(self.h, C.byref(b), int(pair), C.byref(p), _ptr(idx), _ptr(d2)), "ba_icp_nn")
        return idx[:ns].copy(), d2[:ns].copy()

    def icp_times(self) -> np.ndarray:
        """Times (ms) of the last icp: host preparation (wall), the kernels
        (device), the whole call (wall), the kernels per enqueued round."""
        return self._times(self.lib.ba_icp_times)

    # -- map-point upkeep and association gates --------------------------------
    def _map_point_batch(self, mb: MapPointBatch):
        return N.ba_map_point_batch(dim=int(mb.dim), n_cams=mb.cam_center.shape[0], n_pts=mb.pts.shape[0],
                                    n_rows=mb.desc.shape[0], cam_center=_ptr(mb.cam_center), pts=_ptr(mb.pts),
                                    obs_offset=_ptr(mb.obs_offset), obs_cam=_ptr(mb.obs_cam), obs_row=_ptr(mb.obs_row),
                                    obs_scale=_ptr(mb.obs_scale), ref_obs=_ptr(mb.ref_obs), desc=_ptr(mb.desc))

    def map_points_update(self, batch: MapPointBatch, want_desc: bool = True, **mp_options):
        """Map-point upkeep (ba_map_points_update): per point the
        representative descriptor of its track, the mean viewing direction and
        the depth bounds.  mp_options: median_rule, max_scale (defaults:
        ba_map_points_defaults).  Returns (records: a MAP_POINT_DTYPE array,
        desc_out (P, dim) float32 or None)."""
        b = self._map_point_batch(batch)
        p = N.ba_map_point_options()
        self.lib.ba_map_points_defaults(C.byref(p))
        self._set_options(p, mp_options, {"median_rule": int, "max_scale": float, "reserved": int, "reserved_f": float},
                          "map_points_update")
        n = batch.pts.shape[0]
        out = np.zeros(max(n, 1), MAP_POINT_DTYPE)
        desc_out = np.zeros((max(n, 1), int(batch.dim)), np.float32) if want_desc else None
        self._check(self.lib.ba_map_points_update(self.h, C.byref(b), C.byref(p), _ptr(out), _ptr(desc_out)),
                    "ba_map_points_update")
        return out[:n].copy(), (desc_out[:n].copy() if want_desc else None)

    def map_points_distances(self, batch: MapPointBatch, point: int):
        """The dense (n, n) distance matrix and the n row medians of one point
        exactly as map_points_update forms them (ba_map_points_distances)."""
        b = self._map_point_batch(batch)
        n = 0
        if 0 <= int(point) < batch.pts.shape[0]:
            n = max(int(batch.obs_offset[int(point) + 1] - batch.obs_offset[int(point)]), 0)
        D = np.zeros((max(n, 1), max(n, 1)), np.float32)
        m = np.zeros(max(n, 1), np.float32)
        self._check(self.lib.ba_map_points_distances(self.h, C.byref(b), int(point), _ptr(D), _ptr(m)),
                    "ba_map_points_distances")
        return D[:n, :n].copy(), m[:n].copy()

    def map_points_times(self) -> np.ndarray:
        """Times (ms) of the last map_points_update: host preparation (wall),
        the kernels (device), the whole call (wall)."""
        return self._times(self.lib.ba_map_points_times)

    def associate(self, batch: AssocBatch, **assoc_options):
        """The gates of searchInNeighbors per candidate item and fuse pair
        (ba_associate).  assoc_options: chi2, min_cos, max_desc_dist,
        fuse_min_cos, fuse_max_desc_dist (defaults: ba_associate_defaults).
        Returns (items: an ASSOC_DTYPE array, fuse: a FUSE_DTYPE array)."""
        ab = batch
        b = N.ba_assoc_batch(dim=int(ab.dim), n_cams=ab.extr.shape[0], n_pts=ab.pts.shape[0], n_rows=ab.desc.shape[0],
                             n_items=ab.item_cam.shape[0], n_fuse=ab.fuse_pairs.shape[0], extr=_ptr(ab.extr),
                             cam_center=_ptr(ab.cam_center), K=_ptr(ab.K), image_size=_ptr(ab.image_size), pts=_ptr(ab.pts),
                             pt_view_dir=_ptr(ab.pt_view_dir), pt_dist=_ptr(ab.pt_dist), pt_desc=_ptr(ab.pt_desc),
                             desc=_ptr(ab.desc), item_cam=_ptr(ab.item_cam), item_pt=_ptr(ab.item_pt),
                             item_uv=_ptr(ab.item_uv), item_scale=_ptr(ab.item_scale), item_row=_ptr(ab.item_row),
                             item_cur_row=_ptr(ab.item_cur_row), fuse_pairs=_ptr(ab.fuse_pairs))
        p = N.ba_assoc_options()
        self.lib.ba_associate_defaults(C.byref(p))
        self._set_options(p, assoc_options, {"chi2": float, "min_cos": float, "max_desc_dist": float, "fuse_min_cos": float,
                                             "fuse_max_desc_dist": float, "reserved": int}, "associate")
        ni, nf = ab.item_cam.shape[0], ab.fuse_pairs.shape[0]
        items = np.zeros(max(ni, 1), ASSOC_DTYPE)
        fuse = np.zeros(max(nf, 1), FUSE_DTYPE)
        self._check(self.lib.ba_associate(self.h, C.byref(b), C.byref(p), _ptr(items), _ptr(fuse)), "ba_associate")
        return items[:ni].copy(), fuse[:nf].copy()

    # -- covisibility lists, culling votes, local-BA windows ---------------------
    _GRAPH_OPTIONS = {"th": int, "n_best": int, "order": int, "build_windows": int, "current_frame_id": int,
                      "debug_tile_frames": int, "debug_chunk_queries": int, "reserved": int, "redundant_fraction": float}

    def _map_table(self, table: MapTable):
        t = table.normalized()
        return t, N.ba_map_table(n_frames=t.n_frames, n_pts=t.n_pts, n_obs=t.n_obs, reserved=0, frame_id=_ptr(t.frame_id),
                                 frame_is_key=_ptr(t.frame_is_key), pt_invalid=_ptr(t.pt_invalid),
                                 pt_ref_frame=_ptr(t.pt_ref_frame), obs_offset=_ptr(t.obs_offset),
                                 obs_frame=_ptr(t.obs_frame), obs_octave=_ptr(t.obs_octave), obs_outlier=_ptr(t.obs_outlier))

    def _graph_options(self, fn: str, options: dict):
        p = N.ba_graph_options()
        self.lib.ba_map_graph_defaults(C.byref(p))
        return self._set_options(p, options, self._GRAPH_OPTIONS, fn)

    def map_graph(self, table: MapTable, queries, pt_status: bool = False, lists: bool = True, **options) -> MapGraphResult:
        """Covisibility lists, culling votes and local-BA windows of the query
        frames (ba_map_graph).  options: th, n_best, order, build_windows,
        redundant_fraction, current_frame_id (read with pt_status), and the
        debug fields (defaults: ba_map_graph_defaults).  Returns a
        MapGraphResult: the records and, with `lists`, the lists split per
        query (ba_map_graph_lists)."""
        t, b = self._map_table(table)
        p = self._graph_options("map_graph", options)
        q = np.ascontiguousarray(queries, dtype=np.int32).reshape(-1)
        nq = q.size
        rec = np.zeros(max(nq, 1), GRAPH_FRAME_DTYPE)
        status = np.zeros(max(t.n_pts, 1), np.uint8) if pt_status else None
        self._check(self.lib.ba_map_graph(self.h, C.byref(b), _ptr(q), nq, C.byref(p), _ptr(rec), _ptr(status)),
                    "ba_map_graph")
        rec = rec[:nq].copy()
        res = MapGraphResult(query=q, records=rec, nbr_frame=[], nbr_weight=[], win_cam=[], win_cam_fixed=[], win_pt=[],
                             win_obs=[], win_obs_cam=[], win_obs_pt=[],
                             pt_status=None if status is None else status[:t.n_pts].copy(), table=t)
        if not lists:
            return res
        n_cam = rec["n_local"].astype(np.int64) + rec["n_fixed"]
        counts = {"nbr_frame": rec["degree"], "nbr_weight": rec["degree"], "win_cam": n_cam, "win_cam_fixed": n_cam,
                  "win_pt": rec["n_win_pts"], "win_obs": rec["n_win_obs"], "win_obs_cam": rec["n_win_obs"],
                  "win_obs_pt": rec["n_win_obs"]}
        flat = {k: np.zeros(max(int(np.sum(c, dtype=np.int64)), 1), np.uint8 if k == "win_cam_fixed" else np.int32)
                for k, c in counts.items()}
        out = N.ba_graph_lists(**{k: _ptr(a) for k, a in flat.items()})
        self._check(self.lib.ba_map_graph_lists(self.h, C.byref(out)), "ba_map_graph_lists")
        for k, c in counts.items():
            cuts = np.cumsum(np.asarray(c, np.int64))
            setattr(res, k, [a.copy() for a in np.split(flat[k][:int(cuts[-1]) if nq else 0], cuts[:-1])] if nq else [])
        return res

    def map_graph_weights(self, table: MapTable, frame: int, **options) -> np.ndarray:
        """The raw weight row W_frame (n_frames,) int32 exactly as map_graph
        forms it (ba_map_graph_weights)."""
        t, b = self._map_table(table)
        p = self._graph_options("map_graph_weights", options)
        W = np.zeros(max(t.n_frames, 1), np.int32)
        self._check(self.lib.ba_map_graph_weights(self.h, C.byref(b), int(frame), C.byref(p), _ptr(W)),
                    "ba_map_graph_weights")
        return W[:t.n_frames].copy()

    def map_graph_times(self) -> np.ndarray:
        """Times (ms) of the last map_graph: host preparation (wall), the
        kernels (device), the whole call (wall)."""
        return self._times(self.lib.ba_map_graph_times)

    def synchronize(self):
        self._check(self.lib.ba_synchronize(self.h), "ba_synchronize")

    def bench_iterations(self, iters: int, radius: float = 1e4, options: Options | None = None,
                         with_linear_iters: bool = False, time_rj: bool = True):
        """Device time of `iters` LM iterations at a fixed radius: returns
        (ms per iteration, ms of the residual+Jacobian kernel[, mean linear
        solver iterations per LM iteration]).  time_rj=False: no event pair
        around the residual+Jacobian kernel (its ms is then None)."""
        ms = C.c_double()
        rj = C.c_double()
        li = C.c_double()
        o = (options or Options()).to_c()
        self._check(self.lib.ba_bench_iterations(self.h, C.byref(o), int(iters), float(radius), C.byref(ms),
                                                 C.byref(rj) if time_rj else None, C.byref(li)),
                    "ba_bench_iterations")
        r = rj.value if time_rj else None
        if with_linear_iters:
            return ms.value, r, li.value
        return ms.value, r

    def bench_iteration_times(self) -> np.ndarray:
        """Host wall time (ms) of each LM iteration of the last
        bench_iterations call (scalar record to scalar record)."""
        return self._times(self.lib.ba_bench_iteration_times)

    def stream_copy(self, nbytes: int = 1 << 30, reps: int = 10) -> float:
        """Measured device copy bandwidth in GB/s (read + write bytes), the
        STREAM-copy figure SURVEY.md §8d asks for beside the HBM peak."""
        g = C.c_double()
        self._check(self.lib.ba_stream_copy(self.h, C.c_size_t(int(nbytes)), int(reps), C.byref(g)), "ba_stream_copy")
        return g.value


def solve(problem: Problem, options: Options | None = None, device: int = 0):
    """One-shot convenience: returns (cams, pts, summary, iteration_log)."""
    with Solver(device) as s:
        s.set_problem(problem)
        summ = s.solve(options)
        cams, pts = s.params()
        return cams, pts, summ, s.iteration_log()
