"""ctypes binding of libba_hip.so (include/ba_hip.h).

The product path has no CPU fallback: if the HIP library is missing or fails
to load, every entry point raises ``NativeLibraryError``.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = PKG_DIR / "libba_hip.so"

BA_OK = 0
BA_ABI_VERSION = 2          # include/ba_hip.h
STATUS_NAMES = {0: "BA_OK", 1: "BA_ERR_INVALID_ARGUMENT", 2: "BA_ERR_DEVICE", 3: "BA_ERR_OUT_OF_MEMORY",
                4: "BA_ERR_NO_PROBLEM", 5: "BA_ERR_COMM", 6: "BA_ERR_SINGULAR"}
TERMINATION_NAMES = {0: "CONVERGENCE", 1: "NO_CONVERGENCE", 2: "FAILURE"}
# ba_debug_plan's int32 values, in the header's order (BA_DEBUG_PLAN_FIELDS of them)
DEBUG_PLAN_FIELDS = ["nvc", "nblocks", "neblocks", "s_memset", "dup_diag", "chol_persist", "ov_ok", "wcompact",
                     "jdiag", "jrfree", "have_dense", "have_pcg", "npchunks", "pcg_ndup", "pcgc", "pacc", "pcgjf"]


class NativeLibraryError(RuntimeError):
    pass


class BAError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {msg}")
        self.status = status


class ba_problem(C.Structure):
    _fields_ = [
        ("n_cams", C.c_int32), ("n_pts", C.c_int32), ("n_obs", C.c_int32), ("reserved", C.c_int32),
        ("cams", C.c_void_p), ("cam_fixed", C.c_void_p), ("cam_fixed_extr", C.c_void_p), ("K", C.c_void_p),
        ("pts", C.c_void_p), ("pt_fixed", C.c_void_p), ("obs_cam", C.c_void_p), ("obs_pt", C.c_void_p),
        ("obs_uv", C.c_void_p), ("huber_a", C.c_double),
    ]


class ba_options(C.Structure):
    _fields_ = [
        ("max_num_iterations", C.c_int32), ("max_num_consecutive_invalid_steps", C.c_int32),
        ("jacobi_scaling", C.c_int32), ("linear_solver", C.c_int32),
        ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
        ("parameter_tolerance", C.c_double), ("initial_trust_region_radius", C.c_double),
        ("max_trust_region_radius", C.c_double), ("min_trust_region_radius", C.c_double),
        ("min_relative_decrease", C.c_double), ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double),
        ("preconditioner_type", C.c_int32), ("max_linear_solver_iterations", C.c_int32),
        ("min_linear_solver_iterations", C.c_int32), ("precision", C.c_int32), ("eta", C.c_double),
    ]


class ba_summary(C.Structure):
    _fields_ = [
        ("initial_cost", C.c_double), ("final_cost", C.c_double), ("num_iterations", C.c_int32),
        ("num_successful_steps", C.c_int32), ("num_unsuccessful_steps", C.c_int32),
        ("termination_type", C.c_int32), ("total_time_s", C.c_double), ("linearize_time_s", C.c_double),
        ("solve_time_s", C.c_double),
    ]


class ba_iteration(C.Structure):
    _fields_ = [
        ("iteration", C.c_int32), ("step_is_valid", C.c_int32), ("step_is_successful", C.c_int32),
        ("linear_solver_iterations", C.c_int32), ("cost", C.c_double), ("cost_change", C.c_double),
        ("gradient_max_norm", C.c_double), ("gradient_norm", C.c_double), ("step_norm", C.c_double),
        ("relative_decrease", C.c_double), ("trust_region_radius", C.c_double),
        ("model_cost_change", C.c_double), ("iteration_time_s", C.c_double),
    ]


class ba_prune_problem(C.Structure):
    _fields_ = [
        ("n_cams", C.c_int32), ("n_obs", C.c_int32),
        ("extr", C.c_void_p), ("cam_center", C.c_void_p), ("K", C.c_void_p), ("obs_cam", C.c_void_p),
        ("obs_X", C.c_void_p), ("obs_uv", C.c_void_p), ("obs_inv_sigma", C.c_void_p), ("obs_dist", C.c_void_p),
    ]


class ba_pose_batch(C.Structure):
    _fields_ = [
        ("n_problems", C.c_int32), ("reserved", C.c_int32), ("obs_offset", C.c_void_p), ("cams", C.c_void_p),
        ("K", C.c_void_p), ("pts", C.c_void_p), ("obs_uv", C.c_void_p), ("huber_a", C.c_double),
    ]


BA_WINDOW_MAX_CAMS = 16     # include/ba_hip.h


class ba_window_batch(C.Structure):
    _fields_ = [
        ("n_problems", C.c_int32), ("reserved", C.c_int32),
        ("cam_offset", C.c_void_p), ("pt_offset", C.c_void_p), ("obs_offset", C.c_void_p),
        ("cams", C.c_void_p), ("cam_fixed", C.c_void_p), ("cam_fixed_extr", C.c_void_p), ("K", C.c_void_p),
        ("pts", C.c_void_p), ("pt_fixed", C.c_void_p), ("obs_cam", C.c_void_p), ("obs_pt", C.c_void_p),
        ("obs_uv", C.c_void_p), ("huber_a", C.c_double),
    ]


class ba_tri_batch(C.Structure):
    _fields_ = [
        ("n_cams", C.c_int32), ("n_pts", C.c_int32),
        ("extr", C.c_void_p), ("cam_center", C.c_void_p), ("K", C.c_void_p), ("obs_offset", C.c_void_p),
        ("obs_cam", C.c_void_p), ("obs_uv", C.c_void_p), ("obs_scale", C.c_void_p), ("pts_init", C.c_void_p),
        ("huber_a", C.c_double),
    ]


class ba_tri_options(C.Structure):
    _fields_ = [
        ("init", C.c_int32), ("refine", C.c_int32), ("min_views", C.c_int32), ("checks", C.c_int32),
        ("behind_rule", C.c_int32), ("reserved", C.c_int32),
    ]


# enum ba_tri_status / ba_tri_init / ba_tri_check (include/ba_hip.h)
TRI_STATUS_NAMES = {0: "OK", 1: "FEW_VIEWS", 2: "DEGENERATE", 3: "BEHIND", 4: "CHI2", 5: "SCALE"}
TRI_OK, TRI_FEW_VIEWS, TRI_DEGENERATE, TRI_BEHIND, TRI_CHI2, TRI_SCALE = range(6)
TRI_INIT_DLT, TRI_INIT_GIVEN = 0, 1
TRI_CHECK_CHEIRALITY, TRI_CHECK_CHI2, TRI_CHECK_SCALE = 1, 2, 4
TRI_CHECK_ALL = 7


class ba_pnp_options(C.Structure):
    _fields_ = [
        ("max_hypotheses", C.c_int32), ("min_points", C.c_int32), ("min_inliers", C.c_int32),
        ("use_prior", C.c_int32), ("refine", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64),
        ("threshold_px", C.c_double),
    ]


class ba_pnp_result(C.Structure):
    _fields_ = [
        ("status", C.c_int32), ("n_inliers", C.c_int32), ("n_inliers_ransac", C.c_int32),
        ("best_hypothesis", C.c_int32), ("cam_ransac", C.c_double * 6), ("refine", ba_summary),
    ]


# enum ba_pnp_status (include/ba_hip.h)
PNP_STATUS_NAMES = {0: "OK", 1: "FEW_POINTS", 2: "NO_MODEL", 3: "REFINE_FAILED"}
PNP_OK, PNP_FEW_POINTS, PNP_NO_MODEL, PNP_REFINE_FAILED = range(4)


class ba_two_view_batch(C.Structure):
    _fields_ = [
        ("n_pairs", C.c_int32), ("reserved", C.c_int32), ("match_offset", C.c_void_p), ("K1", C.c_void_p),
        ("K2", C.c_void_p), ("uv1", C.c_void_p), ("uv2", C.c_void_p),
    ]


class ba_two_view_options(C.Structure):
    _fields_ = [
        ("max_hypotheses", C.c_int32), ("min_points", C.c_int32), ("min_inliers", C.c_int32), ("min_good", C.c_int32),
        ("model", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64), ("threshold_px", C.c_double),
        ("h_ratio", C.c_double),
    ]


class ba_two_view_result(C.Structure):
    _fields_ = [
        ("status", C.c_int32), ("model", C.c_int32), ("n_inliers", C.c_int32), ("n_good", C.c_int32),
        ("n_good_second", C.c_int32), ("best_hypothesis_e", C.c_int32), ("best_hypothesis_h", C.c_int32),
        ("votes_e", C.c_int32), ("votes_h", C.c_int32), ("reserved", C.c_int32), ("score_e", C.c_double),
        ("score_h", C.c_double), ("E", C.c_double * 9), ("H", C.c_double * 9), ("cam", C.c_double * 6),
        ("normal", C.c_double * 3),
    ]


# enum ba_tv_status, ba_tv_model, ba_tv_e_solver (include/ba_hip.h)
TV_STATUS_NAMES = {0: "OK", 1: "FEW_POINTS", 2: "NO_MODEL", 3: "NO_POSE"}
TV_OK, TV_FEW_POINTS, TV_NO_MODEL, TV_NO_POSE = range(4)
TV_AUTO, TV_ESSENTIAL, TV_HOMOGRAPHY = range(3)
TV_E_EIGHT_POINT, TV_E_FIVE_POINT = range(2)     # ba_two_view_options.reserved


class ba_match_batch(C.Structure):
    _fields_ = [
        ("dim", C.c_int32), ("n_sets", C.c_int32), ("n_pairs", C.c_int32), ("n_ref", C.c_int32),
        ("set_offset", C.c_void_p), ("desc", C.c_void_p), ("pair_query", C.c_void_p), ("pair_train", C.c_void_p),
        ("row_ref", C.c_void_p), ("ref_desc", C.c_void_p),
    ]


class ba_match_options(C.Structure):
    _fields_ = [("ratio", C.c_float), ("unique", C.c_int32), ("max_distance", C.c_float), ("reserved", C.c_int32)]


class ba_match(C.Structure):
    _fields_ = [
        ("query", C.c_int32), ("train", C.c_int32), ("distance", C.c_float), ("second_distance", C.c_float),
        ("ref_distance", C.c_float),
    ]


class ba_match_neighbors(C.Structure):
    _fields_ = [("idx0", C.c_int32), ("idx1", C.c_int32), ("d2_0", C.c_float), ("d2_1", C.c_float)]


class ba_icp_batch(C.Structure):
    _fields_ = [
        ("n_sets", C.c_int32), ("n_pairs", C.c_int32), ("set_offset", C.c_void_p), ("xyz", C.c_void_p),
        ("pair_src", C.c_void_p), ("pair_tgt", C.c_void_p), ("guess", C.c_void_p),
    ]


class ba_icp_options(C.Structure):
    _fields_ = [
        ("max_iterations", C.c_int32), ("max_corr_dist", C.c_float), ("mse_abs_eps", C.c_double),
        ("mse_rel_eps", C.c_double), ("transformation_eps", C.c_double), ("min_correspondences", C.c_int32),
        ("with_scale", C.c_int32), ("fitness_max_range", C.c_float), ("route", C.c_int32), ("cell", C.c_float),
        ("reserved", C.c_int32),
    ]


class ba_icp_result(C.Structure):
    _fields_ = [
        ("final", C.c_float * 16), ("converged", C.c_int32), ("state", C.c_int32), ("iterations", C.c_int32),
        ("n_corr", C.c_int32), ("fitness", C.c_double),
    ]


ICP_ROUTE_AUTO, ICP_ROUTE_GRID, ICP_ROUTE_BRUTE = range(3)
(ICP_NOT_CONVERGED, ICP_ITERATIONS, ICP_TRANSFORM, ICP_ABS_MSE, ICP_REL_MSE, ICP_NO_CORRESPONDENCES) = range(6)


class ba_map_point_batch(C.Structure):
    _fields_ = [
        ("dim", C.c_int32), ("n_cams", C.c_int32), ("n_pts", C.c_int32), ("n_rows", C.c_int32),
        ("cam_center", C.c_void_p), ("pts", C.c_void_p), ("obs_offset", C.c_void_p), ("obs_cam", C.c_void_p),
        ("obs_row", C.c_void_p), ("obs_scale", C.c_void_p), ("ref_obs", C.c_void_p), ("desc", C.c_void_p),
    ]


class ba_map_point_options(C.Structure):
    _fields_ = [("median_rule", C.c_int32), ("reserved", C.c_int32), ("max_scale", C.c_float), ("reserved_f", C.c_float)]


class ba_map_point(C.Structure):
    _fields_ = [
        ("status", C.c_int32), ("best", C.c_int32), ("median", C.c_float), ("view_dir", C.c_float * 3),
        ("min_dist", C.c_float), ("max_dist", C.c_float),
    ]


BA_MP_MAX_TRACK = 1024
MP_OK, MP_EMPTY = range(2)                        # ba_mp_status
MP_MEDIAN_REFERENCE, MP_MEDIAN_FLOAT = range(2)   # ba_mp_median


class ba_assoc_batch(C.Structure):
    _fields_ = [
        ("dim", C.c_int32), ("n_cams", C.c_int32), ("n_pts", C.c_int32), ("n_rows", C.c_int32), ("n_items", C.c_int32),
        ("n_fuse", C.c_int32),
        ("extr", C.c_void_p), ("cam_center", C.c_void_p), ("K", C.c_void_p), ("image_size", C.c_void_p),
        ("pts", C.c_void_p), ("pt_view_dir", C.c_void_p), ("pt_dist", C.c_void_p), ("pt_desc", C.c_void_p),
        ("desc", C.c_void_p), ("item_cam", C.c_void_p), ("item_pt", C.c_void_p), ("item_uv", C.c_void_p),
        ("item_scale", C.c_void_p), ("item_row", C.c_void_p), ("item_cur_row", C.c_void_p), ("fuse_pairs", C.c_void_p),
    ]


class ba_assoc_options(C.Structure):
    _fields_ = [
        ("chi2", C.c_float), ("min_cos", C.c_float), ("max_desc_dist", C.c_float), ("fuse_min_cos", C.c_float),
        ("fuse_max_desc_dist", C.c_float), ("reserved", C.c_int32),
    ]


class ba_assoc_result(C.Structure):
    _fields_ = [
        ("status", C.c_int32), ("chi", C.c_float), ("cosine", C.c_float), ("world_dist", C.c_float),
        ("dist_matched", C.c_float), ("dist_current", C.c_float),
    ]


class ba_fuse_result(C.Structure):
    _fields_ = [("status", C.c_int32), ("cosine", C.c_float), ("dist", C.c_float)]


(AS_ADD, AS_REPLACE, AS_BEHIND, AS_BOUNDS, AS_CHI2, AS_ANGLE, AS_DEPTH, AS_DESC, AS_WORSE) = range(9)   # ba_assoc_status
FUSE_OK, FUSE_ANGLE, FUSE_DESC = range(3)                                                              # ba_fuse_status


class ba_map_table(C.Structure):
    _fields_ = [
        ("n_frames", C.c_int32), ("n_pts", C.c_int32), ("n_obs", C.c_int32), ("reserved", C.c_int32),
        ("frame_id", C.c_void_p), ("frame_is_key", C.c_void_p), ("pt_invalid", C.c_void_p), ("pt_ref_frame", C.c_void_p),
        ("obs_offset", C.c_void_p), ("obs_frame", C.c_void_p), ("obs_octave", C.c_void_p), ("obs_outlier", C.c_void_p),
    ]


class ba_graph_options(C.Structure):
    _fields_ = [
        ("th", C.c_int32), ("n_best", C.c_int32), ("order", C.c_int32), ("build_windows", C.c_int32),
        ("current_frame_id", C.c_int32), ("debug_tile_frames", C.c_int32), ("debug_chunk_queries", C.c_int32),
        ("reserved", C.c_int32), ("redundant_fraction", C.c_double),
    ]


class ba_graph_frame(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("status", "degree", "max_weight", "n_map", "n_redundant", "cull", "n_local",
                                         "n_fixed", "n_win_pts", "n_win_obs")]


class ba_graph_lists(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("nbr_frame", "nbr_weight", "win_cam", "win_cam_fixed", "win_pt", "win_obs",
                                          "win_obs_cam", "win_obs_pt")]


GRAPH_OK, GRAPH_FALLBACK, GRAPH_ISOLATED = range(3)                              # ba_graph_status
GRAPH_WEAKEST_FIRST, GRAPH_STRONGEST_FIRST = range(2)                            # ba_graph_order
GRAPH_PT_RECENT, GRAPH_PT_MATURE, GRAPH_PT_ERASE, GRAPH_PT_INVALID = range(4)    # ba_graph_pt_status


class ba_covariance_request(C.Structure):
    _fields_ = [
        ("n_cam_pairs", C.c_int32), ("n_points", C.c_int32), ("cam_pairs", C.c_void_p), ("cam_cov", C.c_void_p),
        ("points", C.c_void_p), ("pt_cov", C.c_void_p),
    ]


class ba_covariance_request_ex(C.Structure):
    _fields_ = [
        ("base", ba_covariance_request),
        ("n_cam_pt", C.c_int32), ("n_pt_pairs", C.c_int32), ("cam_pt", C.c_void_p), ("cam_pt_cov", C.c_void_p),
        ("pt_pairs", C.c_void_p), ("pt_pt_cov", C.c_void_p),
        ("n_lev", C.c_int32), ("reserved", C.c_int32), ("lev_obs", C.c_void_p), ("leverage", C.c_void_p),
    ]


class ba_cov_iter_options(C.Structure):
    _fields_ = [("preconditioner_type", C.c_int32), ("max_iterations", C.c_int32), ("tolerance", C.c_double)]


class ba_cov_iter_info(C.Structure):
    _fields_ = [
        ("n_columns", C.c_int32), ("n_converged", C.c_int32), ("max_iterations_used", C.c_int32),
        ("reserved", C.c_int32), ("max_residual", C.c_double), ("ms", C.c_double * 4),
    ]


# int (*)(void* user, double* values, int64_t n, int op) of ba_comm_init_host
HOST_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int64, C.c_int)

PRUNE_NAMES = {0: "INLIER", 1: "OUTLIER_BEHIND", 2: "OUTLIER_DEPTH", 3: "OUTLIER_CHI2"}


# (name, restype, argtypes) — every symbol declared in include/ba_hip.h
SIGNATURES = [
    ("ba_abi_version", C.c_int, []),
    ("ba_default_options", None, [C.POINTER(ba_options)]),
    ("ba_create", C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    ("ba_destroy", C.c_int, [C.c_void_p]),
    ("ba_last_error", C.c_char_p, [C.c_void_p]),
    ("ba_comm_unique_id", C.c_int, [C.c_char_p]),
    ("ba_comm_init", C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_int]),
    ("ba_comm_allreduce_host", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    ("ba_comm_init_host", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    ("ba_set_problem", C.c_int, [C.c_void_p, C.POINTER(ba_problem)]),
    ("ba_set_params", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ba_solve", C.c_int, [C.c_void_p, C.POINTER(ba_options), C.POINTER(ba_summary)]),
    ("ba_get_params", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ba_get_iteration_log", C.c_int, [C.c_void_p, C.POINTER(ba_iteration), C.c_int]),
    ("ba_eval_residuals", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    ("ba_linearize", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    ("ba_bench_iteration_times", C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    ("ba_debug_blocks", C.c_int, [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    ("ba_debug_factor", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.POINTER(C.c_int)]),
    ("ba_debug_plan", C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    ("ba_prune", C.c_int, [C.c_void_p, C.POINTER(ba_prune_problem), C.c_void_p]),
    ("ba_solve_pose_batch", C.c_int, [C.c_void_p, C.POINTER(ba_pose_batch), C.POINTER(ba_options), C.c_void_p,
                                      C.POINTER(ba_summary)]),
    ("ba_solve_window_batch", C.c_int, [C.c_void_p, C.POINTER(ba_window_batch), C.POINTER(ba_options), C.c_void_p,
                                        C.c_void_p, C.POINTER(ba_summary)]),
    ("ba_get_window_iteration_log", C.c_int, [C.c_void_p, C.c_int, C.POINTER(ba_iteration), C.c_int]),
    ("ba_window_times", C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    ("ba_triangulate_defaults", None, [C.POINTER(ba_tri_options)]),
    ("ba_triangulate", C.c_int, [C.c_void_p, C.POINTER(ba_tri_batch), C.POINTER(ba_tri_options),
                                 C.POINTER(ba_options), C.c_void_p, C.c_void_p, C.POINTER(ba_summary)]),
    ("ba_triangulate_times", C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    ("ba_pnp_defaults", None, [C.POINTER(ba_pnp_options)]),
    ("ba_pnp_ransac", C.c_int, [C.c_void_p, C.POINTER(ba_pose_batch), C.POINTER(ba_pnp_options),
                                C.POINTER(ba_options), C.c_void_p, C.c_void_p, C.POINTER(ba_pnp_result)]),
    ("ba_pnp_times", C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    ("ba_pnp_hypotheses", C.c_int, [C.c_void_p, C.POINTER(ba_pose_batch), C.POINTER(ba_pnp_options), C.c_int,
                                    C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("ba_two_view_defaults", None, [C.POINTER(ba_two_view_options)]),
    ("ba_two_view_ransac", C.c_int, [C.c_void_p, C.POINTER(ba_two_view_batch), C.POINTER(ba_two_view_options),
                                     C.c_void_p, C.POINTER(ba_two_view_result)]),
    ("ba_two_view_times", C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    ("ba_two_view_hypotheses", C.c_int, [C.c_void_p, C.POINTER(ba_two_view_batch), C.POINTER(ba_two_view_options),
                                         C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    ("ba_match_defaults", None, [C.POINTER(ba_match_options)]),
    ("ba_match_descriptors", C.c_int, [C.c_void_p, C.POINTER(ba_match_batch), C.POINTER(ba_match_options), C.c_void_p,
                                       C.c_void_p]),
    ("ba_match_times", C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    ("ba_match_knn", C.c_int, [C.c_void_p, C.POINTER(ba_match_batch), C.c_int, C.c_void_p]),
    ("ba_map_points_defaults", None, [C.POINTER(ba_map_point_options)]),
    ("ba_map_points_update", C.c_int, [C.c_void_p, C.POINTER(ba_map_point_batch), C.POINTER(ba_map_point_options),
                                       C.c_void_p, C.c_void_p]),
    ("ba_map_points_times", C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    ("ba_map_points_distances", C.c_int, [C.c_void_p, C.POINTER(ba_map_point_batch), C.c_int, C.c_void_p, C.c_void_p]),
    ("ba_associate_defaults", None, [C.POINTER(ba_assoc_options)]),
    ("ba_associate", C.c_int, [C.c_void_p, C.POINTER(ba_assoc_batch), C.POINTER(ba_assoc_options), C.c_void_p,
                               C.c_void_p]),
    ("ba_map_graph_defaults", None, [C.POINTER(ba_graph_options)]),
    ("ba_map_graph", C.c_int, [C.c_void_p, C.POINTER(ba_map_table), C.c_void_p, C.c_int, C.POINTER(ba_graph_options),
                               C.c_void_p, C.c_void_p]),
    ("ba_map_graph_lists", C.c_int, [C.c_void_p, C.POINTER(ba_graph_lists)]),
    ("ba_map_graph_weights", C.c_int, [C.c_void_p, C.POINTER(ba_map_table), C.c_int, C.POINTER(ba_graph_options),
                                       C.c_void_p]),
    ("ba_map_graph_times", C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    ("ba_icp_defaults", None, [C.POINTER(ba_icp_options)]),
    ("ba_icp", C.c_int, [C.c_void_p, C.POINTER(ba_icp_batch), C.POINTER(ba_icp_options), C.c_void_p, C.c_void_p]),
    ("ba_icp_times", C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    ("ba_icp_nn", C.c_int, [C.c_void_p, C.POINTER(ba_icp_batch), C.c_int, C.POINTER(ba_icp_options), C.c_void_p,
                            C.c_void_p]),
    ("ba_covariance", C.c_int, [C.c_void_p, C.POINTER(ba_covariance_request)]),
    ("ba_covariance_ex", C.c_int, [C.c_void_p, C.POINTER(ba_covariance_request_ex)]),
    ("ba_covariance_times", C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    ("ba_covariance_iterative_defaults", None, [C.POINTER(ba_cov_iter_options)]),
    ("ba_covariance_iterative", C.c_int, [C.c_void_p, C.POINTER(ba_covariance_request),
                                          C.POINTER(ba_cov_iter_options), C.POINTER(ba_cov_iter_info)]),
    ("ba_covariance_iterative_bench", C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    ("ba_synchronize", C.c_int, [C.c_void_p]),
    ("ba_bench_iterations", C.c_int, [C.c_void_p, C.POINTER(ba_options), C.c_int, C.c_double,
                                      C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("ba_stream_copy", C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_double)]),
]

# Entry points whose names carry a digit.  tests/test_abi.py compares SIGNATURES with the header's names
# matching ba_[a-z_]+, which such a name does not; they are bound like the others.
SIGNATURES_DIGIT = [
    ("ba_two_view_hypotheses_e5", C.c_int, [C.c_void_p, C.POINTER(ba_two_view_batch), C.POINTER(ba_two_view_options),
                                            C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
]

_LIB = None


def load_library(path: str | os.PathLike | None = None):
    """Load libba_hip.so (in-tree).  Raises NativeLibraryError if absent."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    # BA_HIP_LIB: load another build of the same ABI (A/B kernel comparisons)
    p = Path(path) if path else Path(os.environ.get("BA_HIP_LIB", str(LIB_PATH)))
    if not p.exists():
        raise NativeLibraryError(
            f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    try:
        lib = C.CDLL(str(p), mode=C.RTLD_GLOBAL)
    except OSError as e:  # pragma: no cover - environment specific
        raise NativeLibraryError(f"failed to load {p}: {e}") from e
    for name, res, args in SIGNATURES + SIGNATURES_DIGIT:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.ba_abi_version() != BA_ABI_VERSION:
        raise NativeLibraryError("ABI version mismatch")
    if path is None:
        _LIB = lib
    return lib


def default_options() -> ba_options:
    o = ba_options()
    load_library().ba_default_options(C.byref(o))
    return o
