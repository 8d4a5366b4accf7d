/*
 * ba_hip.h — C-ABI of libba_hip.so, the MI355X-native replacement for the
 * reference's Ceres Problem/Solve bundle-adjustment path.
 *
 * Reference seam being replaced (MatteoWohlrapp/BundleAdjustment,
 * ba_project/src/ba):
 *   ceres::Problem problem;                                 Optimizer.cpp:229
 *   problem.AddResidualBlock(cost, HuberLoss(sqrt(5.991)),  Optimizer.cpp:312-329
 *                            cam6*, pt3*)                   (also :486-490, :645-691)
 *   configureSolver(options)  -> LM, DENSE_SCHUR, ...       Optimizer.cpp:80-90
 *   ceres::Solve(options, &problem, &summary)               Optimizer.cpp:242, 442, 570
 *
 * Conventions (match the reference's parameter layout, Optimizer.h:54-76):
 *   camera block  double[6] = [wx, wy, wz, tx, ty, tz]: world->camera,
 *                 angle-axis + translation, additive update (no manifold).
 *   point block   double[3] world position.
 *   K             float[9]  column-major 3x3 (Eigen Matrix3f storage).
 *   fixed camera  float[16] column-major 4x4 world->camera extrinsic, used
 *                 exactly like PointOnlyReprojectionError (Optimizer.h:96-107).
 *   observation   (camera index, point index, float2 pixel).
 *   Residual kind per observation (chosen like prepareConstraints,
 *   Optimizer.cpp:306-329 / 472-490 / 668-691):
 *     camera variable, point variable -> AngleReprojectionError      (2x[6,3])
 *     camera fixed,    point variable -> PointOnlyReprojectionError  (2x[3])
 *     camera variable, point fixed    -> PoseOnlyAngleReprojectionError (2x[6])
 *     both fixed                      -> constant block (cost only)
 *   Each residual carries ceres::HuberLoss(huber_a) (huber_a <= 0: no loss).
 *
 * Error behaviour: no exceptions cross the ABI.  Every call returns a status
 * (BA_OK == 0); ba_last_error(ctx) describes the last failure.  Solver
 * non-convergence is NOT an error: it is reported in ba_summary exactly like
 * ceres::Solver::Summary::termination_type (which the reference ignores).
 *
 * Threading: a ba_ctx is not thread-safe; use one context per calling thread.
 * All calls block until their results are on the host.
 */
#ifndef BA_HIP_H_
#define BA_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BA_ABI_VERSION 2

enum ba_status {
  BA_OK = 0,
  BA_ERR_INVALID_ARGUMENT = 1,
  BA_ERR_DEVICE = 2,          /* HIP runtime / kernel failure */
  BA_ERR_OUT_OF_MEMORY = 3,
  BA_ERR_NO_PROBLEM = 4,      /* ba_solve before ba_set_problem */
  BA_ERR_COMM = 5,            /* RCCL failure */
  BA_ERR_SINGULAR = 6         /* ba_covariance: the system is not positive definite */
};

enum ba_termination {          /* ceres::TerminationType subset */
  BA_CONVERGENCE = 0,
  BA_NO_CONVERGENCE = 1,
  BA_FAILURE = 2
};

enum ba_linear_solver {
  BA_DENSE_SCHUR = 0,          /* ceres::DENSE_SCHUR (Optimizer.cpp:85): explicit reduced camera
                                  system, dense Cholesky (MFMA) */
  BA_ITERATIVE_SCHUR = 1       /* ceres::ITERATIVE_SCHUR: implicit Schur complement + PCG
                                  (C5 scale; one 6C all-reduce per CG step) */
};

enum ba_preconditioner {       /* ceres::PreconditionerType (ITERATIVE_SCHUR only) */
  BA_JACOBI = 0,               /* ceres default: block diagonal of F'F + D^2 */
  BA_SCHUR_JACOBI = 1          /* block diagonal of the Schur complement */
};

enum ba_precision {
  BA_FP64 = 0,                 /* everything fp64 (the reference's Jets are double) */
  BA_MIXED_FP32 = 1            /* ITERATIVE_SCHUR: fp32 storage of the per-observation Schur
                                  blocks W read by every CG step; fp64 accumulation and CG vectors */
};

typedef struct ba_ctx ba_ctx;

/* Problem description (caller-owned host SoA; copied to the device by
 * ba_set_problem).  Replaces the AddResidualBlock loop of prepareConstraints. */
typedef struct {
  int32_t n_cams, n_pts, n_obs, reserved;
  const double*  cams;            /* [6*n_cams]                             */
  const uint8_t* cam_fixed;       /* [n_cams] 1 = constant (may be NULL)    */
  const float*   cam_fixed_extr;  /* [16*n_cams] col-major; read for fixed cams (may be NULL if none) */
  const float*   K;               /* [9*n_cams] col-major                   */
  const double*  pts;             /* [3*n_pts]                              */
  const uint8_t* pt_fixed;        /* [n_pts] 1 = constant (may be NULL)     */
  const int32_t* obs_cam;         /* [n_obs]                                */
  const int32_t* obs_pt;          /* [n_obs]                                */
  const float*   obs_uv;          /* [2*n_obs]                              */
  double huber_a;                 /* sqrt(5.991) in the reference           */
} ba_problem;

/* ceres::Solver::Options fields the reference touches (configureSolver,
 * Optimizer.cpp:80-90) plus the Ceres defaults it inherits. */
typedef struct {
  int32_t max_num_iterations;                 /* m_nMaxItPerBA (Optimizer.h:203,212) */
  int32_t max_num_consecutive_invalid_steps;  /* 5  */
  int32_t jacobi_scaling;                     /* 1  */
  int32_t linear_solver;                      /* BA_DENSE_SCHUR */
  double function_tolerance;                  /* 1e-6  */
  double gradient_tolerance;                  /* 1e-10 */
  double parameter_tolerance;                 /* 1e-8  */
  double initial_trust_region_radius;         /* 1e4   */
  double max_trust_region_radius;             /* 1e16  */
  double min_trust_region_radius;             /* 1e-32 */
  double min_relative_decrease;               /* 1e-3  */
  double min_lm_diagonal;                     /* 1e-6  */
  double max_lm_diagonal;                     /* 1e32  */
  /* ITERATIVE_SCHUR (ceres::Solver::Options defaults; unused by DENSE_SCHUR) */
  int32_t preconditioner_type;                /* BA_JACOBI */
  int32_t max_linear_solver_iterations;       /* 500 */
  int32_t min_linear_solver_iterations;       /* 0   */
  int32_t precision;                          /* BA_FP64 */
  double eta;                                 /* 1e-1: CG q_tolerance (LevenbergMarquardtStrategy) */
} ba_options;

/* ceres::Solver::Summary subset */
typedef struct {
  double initial_cost;
  double final_cost;
  int32_t num_iterations;
  int32_t num_successful_steps;
  int32_t num_unsuccessful_steps;
  int32_t termination_type;        /* enum ba_termination */
  double total_time_s;             /* wall time of ba_solve */
  double linearize_time_s;         /* device time: residual+Jacobian+assembly */
  double solve_time_s;             /* device time: Schur + reduced solve + back-sub + candidate */
} ba_summary;

/* ceres::IterationSummary subset (one record per minimizer iteration,
 * iteration 0 = initial evaluation). */
typedef struct {
  int32_t iteration;
  int32_t step_is_valid;
  int32_t step_is_successful;
  int32_t linear_solver_iterations; /* CG iterations (ITERATIVE_SCHUR), 1 for DENSE_SCHUR */
  double cost;
  double cost_change;
  double gradient_max_norm;
  double gradient_norm;
  double step_norm;
  double relative_decrease;
  double trust_region_radius;
  double model_cost_change;
  double iteration_time_s;
} ba_iteration;

int ba_abi_version(void);
void ba_default_options(ba_options* opt);       /* Ceres defaults, max_num_iterations = 50 */

/* Context on one HIP device (the process's GPU).  Owns device buffers, the
 * HIP stream and (after ba_comm_init) the RCCL communicator. */
int ba_create(ba_ctx** ctx, int device);
int ba_destroy(ba_ctx* ctx);
const char* ba_last_error(const ba_ctx* ctx);

/* Multi-GPU (points sharded across ranks; cameras replicated).  Every rank
 * calls ba_comm_init with the same 128-byte id produced by ba_comm_unique_id
 * on rank 0 (exchange it with any host transport, e.g. torch.distributed).
 * Per LM iteration the ranks all-reduce the camera-side system over RCCL. */
int ba_comm_unique_id(char id[128]);
int ba_comm_init(ba_ctx* ctx, const char id[128], int nranks, int rank);

/* Host-visible collective over the context's communicator (RCCL): in-place
 * reduction of n doubles across ranks (op 0 = sum, 1 = max); blocks until the
 * result is on the host.  With n = 0 it is a barrier.  Without a
 * communicator it is the identity.  Used for the bench's max-over-ranks
 * timing, so no second GPU runtime is needed for host-side rendezvous. */
int ba_comm_allreduce_host(ba_ctx* ctx, double* values, int n, int op);

/* Host-staged transport for the same exchange (test hook, not the product
 * path): every all-reduce of the multi-rank LM iteration is copied to the
 * host and handed to fn(user, values, n, op) (op 0 = sum, 1 = max; in place;
 * return 0 on success), e.g. torch.distributed over gloo.  It lets several
 * ranks share one GPU — RCCL refuses duplicate devices — so the multi-rank
 * HIP path (packing, folding, replicated decisions) runs on a 1-GPU box.
 * Replaces any RCCL communicator of the context. */
typedef int (*ba_host_allreduce_fn)(void* user, double* values, int64_t n, int op);
int ba_comm_init_host(ba_ctx* ctx, ba_host_allreduce_fn fn, void* user, int nranks, int rank);

/* Copy a problem to the device and build its (fixed) structure. */
int ba_set_problem(ba_ctx* ctx, const ba_problem* problem);

/* Replace the parameter values of the current problem (same structure). */
int ba_set_params(ba_ctx* ctx, const double* cams, const double* pts);

/* Levenberg-Marquardt with DENSE_SCHUR or ITERATIVE_SCHUR (ceres::Solve
 * semantics; opt->linear_solver). */
int ba_solve(ba_ctx* ctx, const ba_options* opt, ba_summary* summary);

/* Current parameters (after ba_solve: the returned minimum). */
int ba_get_params(ba_ctx* ctx, double* cams, double* pts);

/* Iteration log of the last ba_solve: copies min(n, available) records,
 * returns the number available (or <0 on error). */
int ba_get_iteration_log(ba_ctx* ctx, ba_iteration* out, int n);

/* Raw functor residuals r[2*n_obs] in caller observation order and the total
 * robustified cost 0.5*sum(rho) (used for pruning and tests). */
int ba_eval_residuals(ba_ctx* ctx, double* r, double* cost);

/* Linearisation at the current parameters in caller order: Huber-corrected
 * residuals r[2*n_obs] and Jacobian J[n_obs][2][9] (camera 6 | point 3;
 * zero blocks for constant parameter blocks).  Test/inspection entry point. */
int ba_linearize(ba_ctx* ctx, double* r, double* J, double* cost);

/* pruneCorrespondences (BAOptimizer, Optimizer.cpp:6-79) for a batch of
 * (keyframe, keypoint) pairs, evaluated in float like the reference:
 *   c = hnormalized(extr * [X;1]); outlier if c.z <= 0;
 *   outlier if |X - cam_center| > max_dist or < min_dist;
 *   outlier if |hnormalized(K c) - uv| * inv_sigma > 5.991 (a norm, not a
 *   squared norm: Optimizer.cpp:56-59); otherwise inlier.
 * Operation order (fixed here; Eigen's is not pinned): matrix-vector products
 * accumulate column by column, norms as sqrt((x*x + y*y) + z*z), no fused
 * multiply-adds, IEEE division and square root.
 * The caller selects which pairs to evaluate (considerOutlier) and applies
 * the results with Frame::setOutlier / setInlier. */
typedef struct {
  int32_t n_cams, n_obs;
  const float*   extr;            /* [16*n_cams] col-major world->camera = getPose().inverse() */
  const float*   cam_center;      /* [3*n_cams]  getWorldPos()                   */
  const float*   K;               /* [9*n_cams]  col-major getIntrinsics()      */
  const int32_t* obs_cam;         /* [n_obs]                                     */
  const float*   obs_X;           /* [3*n_obs]   MapPoint::getPosition()          */
  const float*   obs_uv;          /* [2*n_obs]   getKeypoint(i)->pt               */
  const float*   obs_inv_sigma;   /* [n_obs]     (float)(1.0 / pow(1.2, octave))  */
  const float*   obs_dist;        /* [2*n_obs]   getMinDistance, getMaxDistance   */
} ba_prune_problem;

enum ba_prune_result {
  BA_INLIER = 0,
  BA_OUTLIER_BEHIND = 1,          /* camspacePos.z() <= 0        (Optimizer.cpp:36-41) */
  BA_OUTLIER_DEPTH = 2,           /* outside [minDist, maxDist]  (:43-51) */
  BA_OUTLIER_CHI2 = 3             /* reprojection test           (:53-64) */
};

/* result[n_obs] receives a ba_prune_result per pair (runs on the device). */
int ba_prune(ba_ctx* ctx, const ba_prune_problem* problem, uint8_t* result);

/* Batched frame-to-frame pose-only solves.
 * Replaces, per frame, the ceres::Problem + ceres::Solve of
 * MotionOnlyBAOptimizerAngles::optimizeCameraPose (Optimizer.cpp:417-442;
 * residuals from MotionOnlyBAOptimizerAngles::prepareConstraints,
 * Optimizer.cpp:459-498: PoseOnlyAngleReprojectionError, Optimizer.h:163-182,
 * with HuberLoss(huber_a)).  Problem i owns observations
 * [obs_offset[i], obs_offset[i+1]) against its own camera; the points are
 * constant.  Same Levenberg-Marquardt semantics as ba_solve on the
 * equivalent one-camera problem (options and termination rules included),
 * but the whole trust-region loop of every problem runs in one kernel
 * launch (one wavefront per problem), so a frame costs one host round trip
 * instead of two per LM iteration.  cams_out[6*i] receives the solution
 * (may alias cams); summaries[i] (may be NULL) the per-problem summary
 * (time fields: the batch's wall time). */
typedef struct {
  int32_t n_problems;
  int32_t reserved;
  const int32_t* obs_offset;      /* [n_problems + 1], obs_offset[0] = 0, non-decreasing */
  const double*  cams;            /* [6*n_problems] initial [w, t] (world->camera)      */
  const float*   K;               /* [9*n_problems] col-major                           */
  const double*  pts;             /* [3*obs_offset[n]] constant world points (float values
                                     of MapPoint::getPosition in the reference)          */
  const float*   obs_uv;          /* [2*obs_offset[n]]                                  */
  double huber_a;                 /* sqrt(5.991); <= 0: no loss                         */
} ba_pose_batch;

int ba_solve_pose_batch(ba_ctx* ctx, const ba_pose_batch* batch, const ba_options* opt, double* cams_out,
                        ba_summary* summaries);

/* Batched small-window bundle adjustment: many independent problems, each
 * with variable cameras AND variable points, solved with ba_solve's
 * DENSE_SCHUR semantics; the whole Levenberg-Marquardt loop of a problem runs
 * inside one kernel launch (one workgroup per problem).  Replaces, per
 * window, the ceres::Problem + ceres::Solve of LocalBAOptimizerAngles
 * (Optimizer.cpp:500-698: the current keyframe and its covisible frames
 * variable, the other observers as PointOnlyReprojectionError) and of the
 * small global BAs.
 *
 * Problem i owns cameras [cam_offset[i], cam_offset[i+1]), points
 * [pt_offset[i], pt_offset[i+1]) and observations [obs_offset[i],
 * obs_offset[i+1]) of the concatenated arrays (those of ba_problem);
 * obs_cam / obs_pt index the problem's own cameras and points.  It is solved
 * as ba_set_problem + ba_solve (BA_DENSE_SCHUR, BA_FP64) + ba_get_params
 * would solve the equivalent ba_problem: the four residual kinds, Huber loss,
 * Jacobi scaling from iteration 0, clamped LM diagonal, the same termination
 * rules, invalid-step handling and radius updates.  Duplicate observations
 * are allowed; parameter blocks without observations are returned untouched.
 * At most BA_WINDOW_MAX_CAMS variable cameras with observations per problem
 * (constant cameras are not limited).
 *
 * cams_out[6*n_cams] / pts_out[3*n_pts] receive all parameter blocks (may
 * alias the inputs); summaries[i] (may be NULL) the per-problem summary (time
 * fields: the batch's wall time).  Non-convergence or a numeric failure of
 * one problem is reported in its summary only (a non-finite cost: BA_FAILURE,
 * parameters as last accepted) and does not affect its neighbours.  A
 * problem's result is bitwise reproducible and does not depend on its place
 * in the batch or on the other problems.
 *
 * Errors (the context stays usable; its current problem is not touched, a
 * ba_solve before and after is bit for bit what it would have been; no
 * collective is used):
 *   BA_ERR_INVALID_ARGUMENT  an offset array that decreases, a local index
 *                            out of range, more than BA_WINDOW_MAX_CAMS
 *                            variable observed cameras (the message names the
 *                            problem); linear_solver != BA_DENSE_SCHUR;
 *                            precision != BA_FP64,
 *   BA_ERR_OUT_OF_MEMORY     the scratch cannot be allocated. */
#define BA_WINDOW_MAX_CAMS 16   /* variable, observed cameras per problem (reference: <= 11) */

typedef struct {
  int32_t n_problems, reserved;
  const int32_t* cam_offset;   /* [n_problems+1], [0] = 0, non-decreasing */
  const int32_t* pt_offset;    /* [n_problems+1] */
  const int32_t* obs_offset;   /* [n_problems+1] */
  /* the arrays of ba_problem, concatenated over the problems */
  const double*  cams;  const uint8_t* cam_fixed;  const float* cam_fixed_extr;  const float* K;
  const double*  pts;   const uint8_t* pt_fixed;
  const int32_t* obs_cam;      /* index LOCAL to the problem: 0 .. n_cams(i)-1 */
  const int32_t* obs_pt;       /* local: 0 .. n_pts(i)-1 */
  const float*   obs_uv;
  double huber_a;              /* per batch, as in ba_pose_batch */
} ba_window_batch;

int ba_solve_window_batch(ba_ctx* ctx, const ba_window_batch* batch, const ba_options* opt, double* cams_out,
                          double* pts_out, ba_summary* summaries /* may be NULL */);
/* Iteration log of problem `problem` of the last ba_solve_window_batch; same
 * contract as ba_get_iteration_log (iteration_time_s is 0). */
int ba_get_window_iteration_log(ba_ctx* ctx, int problem, ba_iteration* out, int n);
/* Times (ms) of the last successful ba_solve_window_batch: [0] host
 * preparation (structure, staging, upload enqueue; wall), [1] the kernel
 * (device, HIP events), [2] the whole call (wall).  Copies min(n, 3) values,
 * returns 3 (0 before the first call).  Diagnostic. */
int ba_window_times(ba_ctx* ctx, double* ms, int n);

/* Batched multi-view triangulation with structure-only refinement: the
 * creation of map points.  Replaces SfMHelper::triangulatePoints
 * (SfMHelper.cpp:759-878: cv::triangulatePoints, then three float acceptance
 * tests per point) for any number of views per point, and is the dual of
 * ba_solve_pose_batch: many points, each refined independently against
 * constant cameras, in one kernel launch (a fixed group of 8 lanes per point).
 * Point p owns observations [obs_offset[p], obs_offset[p+1]).
 *
 * Initialisation (init == BA_TRI_INIT_DLT): per view P = K E(0:3, :) in double
 * from the float values, the rows u P2 - P0 and v P2 - P1 (the construction of
 * cv::triangulatePoints), M = A^T A (4x4, fp64, fixed summation order), the
 * eigenvector v of M's smallest eigenvalue by cyclic Jacobi rotations (pair
 * order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); a sweep starts only while the
 * squared off-diagonal mass exceeds 1e-36 of the squared diagonal mass, at
 * most 16 sweeps), X = v[0:3] / v[3] (independent of v's sign).  When the
 * second smallest eigenvalue is <= 1e-12 of the largest (all rays coincide:
 * no point is determined) X is NaN.  BA_TRI_INIT_GIVEN starts from pts_init.
 *
 * Refinement (refine == 1): point p is solved as ba_set_problem + ba_solve
 * (BA_DENSE_SCHUR, BA_FP64) + ba_get_params would solve the ba_problem with
 * all n_cams cameras constant (cam_fixed_extr = extr), one variable point at
 * the start value and the point's observations (PointOnlyReprojectionError,
 * HuberLoss(huber_a), Jacobi scaling from iteration 0, the clamped LM
 * diagonal, the same termination rules, invalid-step handling and radius
 * updates; opt = the LM options).  A camera may observe a point more than
 * once: each observation counts.  Non-convergence is reported in the summary
 * only.
 *
 * Acceptance tests, in the reference's order on the float-rounded result
 * (float)X with ba_prune's pinned float arithmetic; the first failing test
 * gives the status:
 *   camCoord = hnormalized(extr [X;1]); cheirality: z <= 0 in every view
 *   (behind_rule 0, the reference's `&&`) or in any view (behind_rule 1);
 *   chi2: |hnormalized(K camCoord) - uv| * invSigma > 5.991f in any view (a
 *   norm, not a squared norm, as in ba_prune), invSigma = (float)(1.0 /
 *   (double)obs_scale);
 *   scale: view 0 (the point's first observation) against every other view
 *   j, with d = |X - cam_center|: rejected if d_0 == 0 || d_j == 0, if
 *   (d_0 / d_j) * 1.5f < s_j / s_0, or if d_0 / d_j > (s_j / s_0) * 1.5f.
 * With two views and the defaults this is triangulatePoints line for line.
 *
 * pts_out[3*n_pts] receives the (refined) points in double, status[n_pts] a
 * ba_tri_status each, summaries[n_pts] (may be NULL; meaningful when refine)
 * the per-point summary (time fields: the call's wall time).  A FEW_VIEWS
 * point is returned as pts_init (GIVEN) or zeros (DLT), its summary is
 * BA_CONVERGENCE with 0 iterations.  A point's output bits depend only on its
 * own observations, the cameras and the options, not on its place in the
 * batch or on the other points; two calls give bitwise equal output.  The
 * call does not touch the context's current problem (a ba_solve before and
 * after is bit for bit what it would have been), uses no collective and
 * blocks until the results are on the host.
 *
 * Errors (the context stays usable; nothing is launched; all validation is on
 * the host):
 *   BA_ERR_INVALID_ARGUMENT  a NULL required array, obs_offset[0] != 0 or a
 *                            decreasing obs_offset (the message names the
 *                            point), obs_cam out of range (names the
 *                            observation), init GIVEN without pts_init, the
 *                            scale test without cam_center, unknown option
 *                            values; with refine: linear_solver !=
 *                            BA_DENSE_SCHUR or precision != BA_FP64,
 *   BA_ERR_OUT_OF_MEMORY     the scratch cannot be allocated. */
enum ba_tri_status {
  BA_TRI_OK = 0,
  BA_TRI_FEW_VIEWS = 1,    /* fewer than max(2, min_views) observations */
  BA_TRI_DEGENERATE = 2,   /* non-finite point (homogeneous w == 0, coincident rays, ...) or the refinement ended BA_FAILURE */
  BA_TRI_BEHIND = 3,       /* SfMHelper.cpp:806-813 */
  BA_TRI_CHI2 = 4,         /* :815-838 */
  BA_TRI_SCALE = 5         /* :840-858 */
};
enum ba_tri_init { BA_TRI_INIT_DLT = 0, BA_TRI_INIT_GIVEN = 1 };
enum ba_tri_check { BA_TRI_CHECK_CHEIRALITY = 1, BA_TRI_CHECK_CHI2 = 2, BA_TRI_CHECK_SCALE = 4 };

typedef struct {
  int32_t n_cams, n_pts;
  const float*   extr;        /* [16*n_cams] col-major world->camera = getPose().inverse() (as ba_prune_problem) */
  const float*   cam_center;  /* [3*n_cams]  getWorldPos(); may be NULL when the scale test is off */
  const float*   K;           /* [9*n_cams]  col-major */
  const int32_t* obs_offset;  /* [n_pts+1], [0] = 0, non-decreasing */
  const int32_t* obs_cam;     /* [n_obs] */
  const float*   obs_uv;      /* [2*n_obs] */
  const float*   obs_scale;   /* [n_obs] (float)pow(1.2, octave); NULL = all 1 */
  const double*  pts_init;    /* [3*n_pts]; read when init == BA_TRI_INIT_GIVEN */
  double huber_a;             /* refinement loss, as ba_pose_batch */
} ba_tri_batch;

typedef struct {
  int32_t init;        /* BA_TRI_INIT_DLT (default) | BA_TRI_INIT_GIVEN */
  int32_t refine;      /* 0 (default: the reference's path) | 1: per-point LM */
  int32_t min_views;   /* default 2 */
  int32_t checks;      /* ba_tri_check bits; default all three */
  int32_t behind_rule; /* 0 (default, the reference's): z <= 0 in EVERY view; 1: in ANY view */
  int32_t reserved;
} ba_tri_options;

void ba_triangulate_defaults(ba_tri_options* opt);
int ba_triangulate(ba_ctx* ctx, const ba_tri_batch* batch, const ba_tri_options* topt /* NULL = defaults */,
                   const ba_options* opt /* LM options, NULL = defaults; read when refine */,
                   double* pts_out /* [3*n_pts] */, uint8_t* status /* [n_pts] */,
                   ba_summary* summaries /* [n_pts], may be NULL */);
/* Times (ms) of the last successful ba_triangulate: [0] host preparation
 * (validation, staging, upload enqueue; wall), [1] the kernels (device, HIP
 * events), [2] the whole call (wall).  Copies min(n, 3) values, returns 3 (0
 * before the first call).  Diagnostic. */
int ba_triangulate_times(ba_ctx* ctx, double* ms, int n);

/* Batched robust absolute pose: P3P RANSAC on the device, refined by the pose
 * LM of ba_solve_pose_batch.  This is the reference's EstimationType::PNP row
 * (SfMHelper::estimatePoseUsingPnP, SfMHelper.cpp:16-104), which wanted
 * cv::solvePnPRansac(..., true, 1000, 8.0, 0.99, inliers) (line 72), fell back
 * to plain solvePnP and never fills its inlier vector.  The input is a
 * ba_pose_batch: problem i owns observations [obs_offset[i], obs_offset[i+1])
 * of constant points; cams is the prior (useExtrinsicGuess) and may be NULL
 * only when use_prior == 0.
 *
 * Sampling, pinned so that any implementation draws the same triples and
 * independent of the problem's place in the batch.  With n the problem's
 * observation count and mix() the splitmix64 finaliser
 *   mix(z): z ^= z>>30; z *= 0xBF58476D1CE4E5B9; z ^= z>>27; z *= 0x94D049BB133111EB; z ^= z>>31
 *   draw(h, j, m) = ((mix(seed + (4h + j + 1) * 0x9E3779B97F4A7C15) >> 32) * m) >> 32   (uint64, wrapping)
 *   a = draw(h, 0, n)
 *   b = draw(h, 1, n-1);  if b >= a: ++b
 *   c = draw(h, 2, n-2);  if c >= min(a, b): ++c;  then if c >= max(a, b): ++c
 * hypothesis h samples the local observations (a, b, c), always distinct.
 * With use_prior, hypothesis 0 is the prior itself and hypotheses 1 ..
 * max_hypotheses-1 sample with their own h.
 *
 * Minimal solver (csrc/ba_p3p.h, the same text on the device and in host
 * programs): P3P in fp64 on the unit bearings K^-1 [u, v, 1] of the float
 * pixels promoted to double.  With the distances s_i to the three points it
 * eliminates u = s2/s1 from the two conics the law of cosines gives in (u, v =
 * s3/s1), solves the resultant quartic in v in closed form (resolvent cubic,
 * two real quadratics, two Newton steps per root), recovers u linearly,
 * polishes (s1, s2, s3) by five Newton steps on the three distance equations
 * and takes the rigid motion between the triads of the two triangles.  It
 * returns 0-4 world->camera poses (R, t) with all three sample points at
 * positive depth.  The order of a hypothesis's solutions is fixed: increasing
 * quartic root v = s3/s1.  A double root may be returned twice.
 *
 * Scoring: an observation is an inlier of a pose iff, with p = R X + t and
 * q = K p accumulated as the pose LM accumulates its candidate residual,
 * q2 > 0 and (q0/q2 - u)^2 + (q1/q2 - v)^2 <= threshold_px^2.  A solution's
 * score is its inlier count, a hypothesis's score its best solution (ties: the
 * lower solution index), the winner the best hypothesis (ties: the lower h).
 * Counts are integers, so the result does not depend on a reduction order.
 * There is no confidence parameter: the whole budget is evaluated in parallel,
 * so an early exit would save nothing.
 *
 * After the vote the winner is converted to angle-axis
 * (ceres::RotationMatrixToAngleAxis): cam_ransac = [w, t]; when the prior wins
 * it is returned with its own bits.  The consensus set
 * is the predicate at cam_ransac through ceres::AngleAxisToRotationMatrix, as
 * every residual of the library; n_inliers_ransac is its size.  With refine,
 * cams_out is bit for bit what ba_solve_pose_batch returns for the consensus
 * observations in caller order, started at cam_ransac, with lm and huber_a;
 * without, cams_out = cam_ransac.  inlier[o] (caller order) is the predicate
 * at cams_out, n_inliers its sum per problem.
 *
 * Statuses: a problem with fewer than max(4, min_points) observations is
 * BA_PNP_FEW_POINTS (SfMHelper.cpp:46 keeps the prior for size() <= 6); a best
 * consensus (the winner's vote) below max(4, min_inliers) is BA_PNP_NO_MODEL.
 * Both return the prior in cams_out (zeros without a prior) and in cam_ransac,
 * inlier all 0, best_hypothesis -1 and a zero summary.  If the LM ends
 * BA_FAILURE the status is BA_PNP_REFINE_FAILED and cams_out = cam_ransac.  A
 * problem's status never affects its neighbours.
 *
 * Contract, as ba_triangulate: a problem's output bits depend only on its own
 * data and the options, not on its place in the batch or on the other
 * problems; two calls give bitwise equal output; the context's current problem
 * is untouched (a ba_solve before and after is bit for bit what it would have
 * been); no collective; the call blocks until the results are on the host.
 *
 * Errors (the context stays usable; nothing is launched; all validation is on
 * the host):
 *   BA_ERR_INVALID_ARGUMENT  a NULL required array, obs_offset[0] != 0 or a
 *                            decreasing obs_offset (the message names the
 *                            problem), max_hypotheses outside 1 .. 65536,
 *                            negative min_points / min_inliers, use_prior or
 *                            refine not 0 / 1, a threshold_px that is not
 *                            positive and finite, cams == NULL with
 *                            use_prior; with refine: linear_solver !=
 *                            BA_DENSE_SCHUR or precision != BA_FP64,
 *   BA_ERR_OUT_OF_MEMORY     the scratch cannot be allocated. */
enum ba_pnp_status { BA_PNP_OK = 0, BA_PNP_FEW_POINTS = 1, BA_PNP_NO_MODEL = 2, BA_PNP_REFINE_FAILED = 3 };

typedef struct {
  int32_t max_hypotheses;  /* default 1000 (the reference's commented call); 1 .. 65536 */
  int32_t min_points;      /* default 7: fewer than max(4, min_points) observations is FEW_POINTS */
  int32_t min_inliers;     /* default 6: best consensus below max(4, min_inliers) is NO_MODEL */
  int32_t use_prior;       /* default 1: hypothesis 0 is batch->cams[problem] (useExtrinsicGuess), not a sample */
  int32_t refine;          /* default 1: LM on the consensus set */
  int32_t reserved;
  uint64_t seed;           /* default 0 */
  double  threshold_px;    /* default 8.0; inlier iff r0^2 + r1^2 <= threshold_px^2 */
} ba_pnp_options;

typedef struct {
  int32_t status;             /* ba_pnp_status */
  int32_t n_inliers;          /* of `inlier`, at cams_out */
  int32_t n_inliers_ransac;   /* consensus set at cam_ransac */
  int32_t best_hypothesis;    /* index h of the winner; -1 without a model */
  double  cam_ransac[6];      /* the winner as [w, t], before refinement */
  ba_summary refine;          /* the LM's summary (zeros when refine == 0 or no model; time fields: the call's wall time) */
} ba_pnp_result;

void ba_pnp_defaults(ba_pnp_options* opt);
int ba_pnp_ransac(ba_ctx* ctx, const ba_pose_batch* batch, const ba_pnp_options* popt /* NULL = defaults */,
                  const ba_options* lm /* NULL = defaults; read when refine */,
                  double* cams_out /* [6*n_problems] */, uint8_t* inlier /* [n_obs], caller order */,
                  ba_pnp_result* results /* [n_problems], may be NULL */);
/* Times (ms) of the last successful ba_pnp_ransac: [0] host preparation
 * (validation, staging, upload enqueue; wall), [1] the kernels (device, HIP
 * events), [2] the whole call (wall).  Copies min(n, 3) values, returns 3 (0
 * before the first call).  Diagnostic. */
int ba_pnp_times(ba_ctx* ctx, double* ms, int n);
/* Test / inspection entry point: hypotheses h0 .. h0+n-1 (within
 * max_hypotheses) of problem `problem` exactly as ba_pnp_ransac forms and
 * scores them (min_points is not applied; the problem needs 3 observations
 * unless only the prior is asked for).  sample: the local observation indices
 * (-1 x3 for the prior); n_sol: 0 .. 4; Rt: the solutions in their fixed
 * order, R row-major, then t (unused entries zero); count: their consensus
 * counts at threshold_px.  Same errors as ba_pnp_ransac, plus a problem or
 * hypothesis range out of bounds. */
int ba_pnp_hypotheses(ba_ctx* ctx, const ba_pose_batch* batch, const ba_pnp_options* popt, int problem, int h0, int n,
                      int32_t* sample /* [3*n] */, int32_t* n_sol /* [n] */, double* Rt /* [n][4][12] */,
                      int32_t* count /* [n][4] */);

/* Batched two-view relative pose: essential-matrix and homography RANSAC on
 * the device, the model choice, the decomposition and the positive-depth vote.
 * This is the reference's EstimationType "2d2d" row (SfMHelper::recoverPose,
 * SfMHelper.cpp:498-742: cv::findEssentialMat, cv::findHomography, the
 * ORB-SLAM-style scores, cv::recoverPose / cv::decomposeHomographyMat).  Pair
 * i owns matches [match_offset[i], match_offset[i+1]); uv1 / uv2 are the
 * matched pixels of frame 1 / frame 2.  The semantics are pinned here, not
 * taken from a third-party library.
 *
 * Sampling.  With n the pair's match count and mix() the splitmix64 finaliser
 * of ba_pnp_ransac
 *   draw(h, j, m) = ((mix(seed + (16h + j + 1) * 0x9E3779B97F4A7C15) >> 32) * m) >> 32   (uint64, wrapping)
 * hypothesis h takes eight distinct local indices: for j = 0 .. 7,
 * c = draw(h, j, n - j); for each earlier pick p in increasing order,
 * if c >= p: ++c.  The essential hypothesis uses all eight, the homography
 * hypothesis the first four.  There is no prior hypothesis.
 *
 * Minimal solvers (csrc/ba_two_view.h, the same text on the device and in
 * host programs), fp64 on the float pixels promoted to double.
 *   E: the normalised eight-point on the bearings K^-1 [u, v, 1] dehomogenised
 *      to (x, y, 1): each side Hartley-normalised over the eight samples, the
 *      null vector of the 8x9 system, E = T2^T E^ T1 scaled to Frobenius norm
 *      1 (either sign).
 *   H: the four-point DLT on Hartley-normalised pixels: the null vector of
 *      the 8x9 system, H = T2^-1 H^ T1 scaled to norm 1 with the sign that
 *      transfers the first sample with w > 0 (x2 ~ H x1).
 * The null vector is x = H_0 .. H_7 e_8 of the Householder QR of the
 * transposed system (reflector k from the remainder of row k): it works on
 * the matrix itself and is backward stable.  A model with a non-finite entry
 * is invalid; H is also invalid if |det H| <= 1e-10 r0 r1 r2 (r_i the norms
 * of its rows).  An invalid model scores 0 and cannot win.
 *
 * Vote.  With K^-1 by cofactors, F = K2^-T (E K1^-1) (row-major products, the
 * inner index increasing) and x = [u, v, 1]:
 *   a = F x1 (a_i = F_i0 u1 + F_i1 v1 + F_i2), d2^2 = (u2 a0 + v2 a1 + a2)^2 / (a0^2 + a1^2)
 *   b = F^T x2 likewise,                       d1^2 = (u1 b0 + v1 b1 + b2)^2 / (b0^2 + b1^2)
 *   E-inlier iff d1^2 <= threshold_px^2 and d2^2 <= threshold_px^2.
 *   p = H x1 (p_i = H_i0 u1 + H_i1 v1 + H_i2), e2^2 = (u2 - p0/p2)^2 + (v2 - p1/p2)^2,
 *   e1^2 the same with H^-1 (cofactors / determinant) on x2 against x1; a
 *   transfer with w = p2 <= 0 is an outlier;
 *   H-inlier iff e1^2 <= threshold_px^2 and e2^2 <= threshold_px^2.
 * Votes are integer counts over all matches of the pair; the winner per model
 * is the largest count, ties to the lower h.
 *
 * After the vote, per pair.  A model is available if its winner's vote is at
 * least max(8, min_inliers); a model that is not reports its vote, hypothesis
 * -1 and a zero matrix.  The E winner is projected to the essential
 * manifold (3x3 SVD by one-sided Jacobi, singular values (1, 1, 0) / sqrt 2,
 * U and V made rotations by u3 = u1 x u2, v3 = v1 x v2).  The final masks are
 * the predicates at the projected E and at H, tightened as the reference's
 * post-marking: an E-inlier also needs d1^2, d2^2 <= 3.841 (lines 611-629), an
 * H-inlier both transfer errors <= 5.991 (lines 559-577).  S_E = sum over the
 * E-mask of (5.991 - d1^2) + (5.991 - d2^2), S_H the same over the H-mask with
 * (e1^2, e2^2); both are summed in a fixed order (lane l takes matches l,
 * l + 64, ..; then an xor butterfly 32, 16, .., 1).  BA_TV_AUTO picks the
 * homography iff (float)(S_H / (S_H + S_E)) > h_ratio (line 642), else E; a
 * chosen (or forced) model that is not available is BA_TV_NO_MODEL.
 * Candidates, in this order:
 *   E (4): (U W V^T, +u3), (U W V^T, -u3), (U W^T V^T, +u3), (U W^T V^T, -u3),
 *          W = [0 -1 0; 1 0 0; 0 0 1];
 *   H (8): the SVD decomposition of K2^-1 H K1 = U diag(d1, d2, d3) V^T
 *          (Faugeras, in the form of ORB-SLAM's ReconstructH): candidates
 *          0 .. 3 the case d' = +d2, 4 .. 7 the case d' = -d2, within each the
 *          signs (e1, e3) = (+,+) (+,-) (-,+) (-,-) of the normal's first and
 *          third SVD coordinate; n is returned with n_z >= 0, |t| = 1.  There
 *          are none when d1 / d2 < 1.00001 or d2 / d3 < 1.00001.
 * A candidate's vote is the number of mask inliers with positive depth in
 * both views: (l1, l2) from the 2x2 least-squares solve of l2 b2 = l1 R b1 + t
 * on the dehomogenised bearings; a determinant <= 1e-12 |R b1|^2 |b2|^2 is not
 * good.  The best vote wins; ties go to the larger |n_z| for H (the
 * reference's heuristic, lines 697-711), then to the lower candidate index.
 * n_good < max(1, min_good) is BA_TV_NO_POSE.  cam = [w, t] maps frame 1 to
 * frame 2 (x2 ~ R x1 + t, |t| = 1, w = ceres::RotationMatrixToAngleAxis(R));
 * the reference's pose is its inverse.  No refit follows: callers refine with
 * ba_triangulate and the window BA.
 *
 * The five-point essential solver (e_solver = BA_TV_E_FIVE_POINT; opt-in: with
 * BA_TV_E_EIGHT_POINT, the default, every output bit is what it was before
 * the selector existed).  cv::findEssentialMat is a five-point RANSAC: a
 * hypothesis is an essential matrix by construction, so the projection after
 * the vote changes the winner at rounding level only.  The sampler, the
 * homography hypotheses and everything after the vote are untouched: H,
 * votes_h, best_hypothesis_h and score_h are bitwise those of the eight-point
 * mode.  Per hypothesis (csrc/ba_two_view.h, tv_solve_e5):
 *   Sample: the first five of the eight picks.
 *   Null space: rows [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1] of the
 *     dehomogenised bearings; X, Y, Z, W = H_0 .. H_4 e_j, j = 5 .. 8, of the
 *     Householder QR of the transposed 5x9 system (orthonormal whatever the
 *     rank).  E = xX + yY + zZ + W.
 *   Constraints: a 10x20 matrix; rows 0 .. 8 are the entries of 2 E E^T E -
 *     tr(E E^T) E, row-major, row 9 is det E (cofactors of the first row).
 *     Columns (Nister's order, the first ten are eliminated):
 *       x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1.
 *   Elimination: Gauss-Jordan on the first ten columns with partial pivoting
 *     (the largest |entry| of the column at or below the diagonal, ties to
 *     the lower row).  A pivot at or below 1e-13 times the largest |entry| of
 *     the matrix ends the elimination without solutions.  Only rows 4 .. 9 are
 *     read afterwards (rows 0 .. 3 are not reduced further once pivoted).
 *   Hidden variable: the elimination is run for the three turns of the basis
 *     ((x, y, z) on (X, Y, Z), (Y, Z, X), (Z, X, Y)); the turn whose reduced
 *     rows 4 .. 9 have the smallest largest |entry| is kept (ties: the
 *     earlier): the cancellation in the determinant below grows with those
 *     entries.  No turn eliminated: no solutions.
 *   Polynomial: <k> = row 4 - z row 5, <l> = row 6 - z row 7, <m> = row 8 -
 *     z row 9 are x px(z) + y py(z) + p1(z) of degrees 3, 3, 4; the
 *     tenth-degree polynomial p is the determinant of the 3x3 matrix
 *     [px py p1], expanded by its third column, scaled by its largest
 *     |coefficient|.
 *   Roots: all real roots in [-B, B], B = min(1e25, Fujiwara's bound
 *     2 max_k |p_(10-k) / p_10|^(1/k)).  For d = 1 .. 10 the roots of the
 *     (10 - d)-th derivative are sought between the roots of the derivative
 *     before (and -B, B), where the polynomial is monotonic: a sign change
 *     (v < 0 against v >= 0, by Horner; for d = 10 the 3x3 determinant
 *     itself is evaluated at z instead of its expansion) brackets the one
 *     root, found by at most 64 bisections on the ordered integers of the
 *     doubles (to adjacent doubles; the end with the smaller |v|); an interval
 *     without a sign change hands its upper end on as a placeholder.  There is
 *     no recursion, and every loop has a fixed cap: 10 levels, at most 10
 *     intervals each, 64 bisections, 12 polishing steps.
 *   Back-substitution: (x, y, 1) is the cross product of the two rows of
 *     [px py p1](z) whose third component is the largest in magnitude (ties:
 *     (0,1), (0,2), (1,2)).  Then (x, y, z) takes Gauss-Newton steps on the
 *     nine cubic constraints, cost |C(E)|^2 / |E|^6: at most 12, ending at a
 *     cost <= 1e-30 or at the first step that does not lower the cost.
 *   Solutions: E scaled to Frobenius norm 1 (either sign); a non-finite one is
 *     dropped; order: increasing root of the hidden variable.  Up to ten.
 *   Vote: every (hypothesis, solution) is scored by the E predicate above
 *     over all matches.  The largest count wins; ties go to the lower h, then
 *     to the lower solution index.  best_solution (the result's `reserved`)
 *     is the winner's index within its hypothesis.
 *
 * Statuses: fewer than max(8, min_points) matches is BA_TV_FEW_POINTS.  Every
 * failure returns cam = 0, normal = 0, n_inliers = 0, inlier all 0 and both
 * best_hypothesis fields -1; FEW_POINTS and NO_MODEL zero the rest of the
 * record, NO_POSE keeps model, votes, scores, E, H, n_good and n_good_second.
 * A pair's status never affects its neighbours.
 *
 * Contract, as ba_pnp_ransac: a pair's output bits depend only on its own
 * data and the options, not on its place in the batch or on the other pairs;
 * two calls give bitwise equal output; the context's current problem is
 * untouched; no collective; the call blocks until the results are on the host.
 *
 * Errors (the context stays usable; nothing is launched; all validation is on
 * the host):
 *   BA_ERR_INVALID_ARGUMENT  a NULL required array (K2 may be NULL),
 *                            match_offset[0] != 0 or a decreasing match_offset
 *                            (the message names the pair), max_hypotheses
 *                            outside 1 .. 65536, negative min_points /
 *                            min_inliers / min_good, an unknown model, an
 *                            unknown e_solver (the field `reserved`), a
 *                            threshold_px that is not positive and finite, an
 *                            h_ratio outside [0, 1],
 *   BA_ERR_OUT_OF_MEMORY     the scratch cannot be allocated. */
enum ba_tv_status { BA_TV_OK = 0, BA_TV_FEW_POINTS = 1, BA_TV_NO_MODEL = 2, BA_TV_NO_POSE = 3 };
enum ba_tv_model  { BA_TV_AUTO = 0, BA_TV_ESSENTIAL = 1, BA_TV_HOMOGRAPHY = 2 };
enum ba_tv_e_solver { BA_TV_E_EIGHT_POINT = 0, BA_TV_E_FIVE_POINT = 1 };

typedef struct {            /* pair i owns matches [match_offset[i], match_offset[i+1]) */
  int32_t n_pairs, reserved;
  const int32_t* match_offset;   /* [n_pairs+1], [0] = 0, non-decreasing */
  const float*   K1;             /* [9*n_pairs] col-major, frame 1 */
  const float*   K2;             /* [9*n_pairs]; NULL = K1 (the reference uses frame1's for both) */
  const float*   uv1;            /* [2*n_matches] keypoints1[queryIdx].pt */
  const float*   uv2;            /* [2*n_matches] keypoints2[trainIdx].pt */
} ba_two_view_batch;

typedef struct {
  int32_t max_hypotheses;  /* default 1000; 1 .. 65536 */
  int32_t min_points;      /* default 8: fewer than max(8, min_points) matches is FEW_POINTS */
  int32_t min_inliers;     /* default 8: a winner's vote below max(8, min_inliers) is NO_MODEL */
  int32_t min_good;        /* default 101: the reference's `inliers <= 100 -> false` (SfMHelper.cpp:656) */
  int32_t model;           /* default BA_TV_AUTO */
  int32_t reserved;        /* the E solver, enum ba_tv_e_solver: default BA_TV_E_EIGHT_POINT (0); the member keeps its name */
  uint64_t seed;           /* default 0 */
  double  threshold_px;    /* default 1.0: the reference's RANSAC thresholds (lines 532, 536) */
  double  h_ratio;         /* default 0.4 (line 643) */
} ba_two_view_options;

typedef struct {
  int32_t status, model;               /* model: the one the pose came from (ESSENTIAL / HOMOGRAPHY) */
  int32_t n_inliers;                   /* of `inlier`, final mask of the chosen model */
  int32_t n_good, n_good_second;       /* positive-depth votes: best and runner-up candidate */
  int32_t best_hypothesis_e, best_hypothesis_h;   /* -1 without a model */
  int32_t votes_e, votes_h;            /* the winners' RANSAC votes */
  int32_t reserved;                    /* five-point: the winning solution's index within best_hypothesis_e; 0 in
                                          eight-point mode and whenever best_hypothesis_e is -1 */
  double  score_e, score_h;            /* S_E, S_H */
  double  E[9], H[9];                  /* row-major, Frobenius norm 1; E after the essential projection */
  double  cam[6];                      /* [w, t]: frame 1 -> frame 2 (x2 ~ R x1 + t), |t| = 1, ceres angle-axis */
  double  normal[3];                   /* plane normal in frame 1 (HOMOGRAPHY), else 0 */
} ba_two_view_result;

void ba_two_view_defaults(ba_two_view_options* opt);
int ba_two_view_ransac(ba_ctx* ctx, const ba_two_view_batch* batch, const ba_two_view_options* opt /* NULL = defaults */,
                       uint8_t* inlier /* [n_matches] */, ba_two_view_result* results /* [n_pairs] */);
/* Times (ms) of the last successful ba_two_view_ransac, as ba_pnp_times:
 * [0] host preparation, [1] the kernels (device), [2] the whole call. */
int ba_two_view_times(ba_ctx* ctx, double* ms, int n);
/* Test / inspection entry point: hypotheses h0 .. h0+n-1 (within
 * max_hypotheses) of pair `pair` exactly as ba_two_view_ransac forms and
 * scores them (min_points is not applied; the pair needs 8 matches).  sample:
 * the eight local match indices; E, H: the models, row-major (zeros when
 * invalid), E the eight-point one whatever the selector; valid and count:
 * (E, H) per hypothesis.  Same errors as
 * ba_two_view_ransac, plus a pair or hypothesis range out of bounds. */
int ba_two_view_hypotheses(ba_ctx* ctx, const ba_two_view_batch* batch, const ba_two_view_options* opt, int pair, int h0,
                           int n, int32_t* sample /* [8*n] */, double* E /* [9*n] */, double* H /* [9*n] */,
                           int32_t* valid /* [2*n]: E, H */, int32_t* count /* [2*n] */);
/* Test / inspection entry point of the five-point solver, on the model of
 * ba_pnp_hypotheses: hypotheses h0 .. h0+n-1 of pair `pair` exactly as
 * ba_two_view_ransac forms and scores them with e_solver =
 * BA_TV_E_FIVE_POINT (whatever opt's selector says).  sample: the eight local
 * match indices (the first five are used); n_sol: 0 .. 10; E: the solutions
 * in their fixed order, row-major, Frobenius norm 1 (unused entries zero);
 * count: their votes at threshold_px (0 past n_sol).  Same errors as
 * ba_two_view_hypotheses. */
int ba_two_view_hypotheses_e5(ba_ctx* ctx, const ba_two_view_batch* batch, const ba_two_view_options* opt, int pair, int h0,
                              int n, int32_t* sample /* [8*n] */, int32_t* n_sol /* [n] */, double* E /* [n][10][9] */,
                              int32_t* count /* [n][10] */);

/* ---------------------------------------------------------------------------
 * ba_match_descriptors: batched descriptor matching on the device: exact
 * 2-nearest-neighbour search, Lowe's ratio test and the one-match-per-train
 * filter.  This is the reference's FeatureProcessor::matchFeatures
 * (FeatureProcessor.cpp:39-95: FLANN knnMatch(k = 2), ratio 0.7, sort by
 * trainIdx and keep the first of each run), which feeds every geometric entry
 * above.  FLANN's randomised kd-trees are approximate and unseeded; the exact
 * brute-force answer is what they approximate, and it is what is pinned here
 * (csrc/ba_match.h is the text, the same on the device and in host programs).
 *
 * Batch.  n_sets descriptor sets in CSR form: set s owns rows
 * [set_offset[s], set_offset[s+1]) of desc (row-major, dim floats per row,
 * dim 64 or 128).  Pair i matches the rows of set pair_query[i] (the queries)
 * against those of set pair_train[i]; a set may appear in any number of pairs
 * and is uploaded once.  Match indices are local to their sets.  Optional
 * association input: row_ref[r] >= 0 names a reference descriptor
 * ref_desc[row_ref[r]] of row r (the map point's own descriptor); -1 is none.
 * Descriptors are expected finite.
 *
 * Distance (float32 throughout).
 *   dot(q, t) = the chain acc = fmaf(q_k, t_k, acc), k = 0 .. dim-1 ascending, from 0
 *   nrm(x)    = dot(x, x)
 *   x         = fmaf(-2, dot(q, t), nrm(q) + nrm(t))      (the sum rounded first)
 *   d2        = x > 0 ? x : 0
 *   distance  = (float)sqrt((double)d2)                   (the correctly rounded float root)
 * A descriptor against itself gives exactly 0.
 *
 * 2-NN.  Per query the two smallest keys (bits(d2) << 32 | train) over the
 * train set (d2 >= 0, so its bit pattern orders like its value; ties go to the
 * lower train index).  Partial lists merge exactly under that order, so the
 * result does not depend on tiling or on how a pair is split over workgroups.
 * A missing neighbour has index -1 and d2 = +inf.
 *
 * Ratio.  A query with two neighbours survives when
 *   distance0 < ratio * distance1   (a float product, rounded once)   and
 *   distance0 <= max_distance.
 * A pair whose train set has fewer than two rows yields no matches (the
 * reference indexes knn_matches[i][1] unguarded there).
 *
 * Unique train (unique = 1).  Per train index the surviving query of smallest
 * (bits(d2_0) << 32 | query) wins (the reference's std::sort is unstable, so
 * which query it keeps is unspecified).  unique = 0 returns every survivor.
 *
 * Output.  Pair i owns matches [match_offset[i], match_offset[i+1]) in
 * increasing (train, query): the order the reference returns.  `matches`
 * must hold the sum over the pairs of min(n_q, n_t) records with unique = 1,
 * of n_q with unique = 0.  ref_distance: for a query row with a reference
 * descriptor, the distance (same formulas) from the match's *train*
 * descriptor to that reference (the test of BundleAdjustment.cpp:135-137; the
 * threshold stays with the caller); -1 without one.
 *
 * Contract, as ba_two_view_ransac: a pair's output bits depend only on its own
 * data and the options, not on its place in the batch or on the other pairs;
 * two calls give bitwise equal output; the only atomics are integer minima
 * and counts; the context's current problem is untouched; no collective; the
 * call blocks until the results are on the host.  Empty sets and an empty
 * batch are valid.
 *
 * Errors (the context stays usable; nothing is launched; all validation is on
 * the host):
 *   BA_ERR_INVALID_ARGUMENT  a NULL required array, dim other than 64 / 128,
 *                            negative counts, set_offset[0] != 0 or a
 *                            decreasing set_offset (the message names the
 *                            set), a pair's set index out of range, a row_ref
 *                            outside -1 .. n_ref-1, a set of more than
 *                            8388480 rows, a ratio that is negative or not
 *                            finite, a max_distance that is negative or NaN,
 *                            unique other than 0 / 1, reserved != 0,
 *   BA_ERR_OUT_OF_MEMORY     the scratch cannot be allocated. */
typedef struct {
  int32_t dim;                   /* 64 or 128 */
  int32_t n_sets, n_pairs, n_ref;
  const int32_t* set_offset;     /* [n_sets+1], [0] = 0, non-decreasing: rows of desc */
  const float*   desc;           /* [rows * dim] */
  const int32_t* pair_query;     /* [n_pairs] set index of the queries */
  const int32_t* pair_train;     /* [n_pairs] set index of the train rows */
  const int32_t* row_ref;        /* [rows] index into ref_desc or -1; NULL = none */
  const float*   ref_desc;       /* [n_ref * dim]; may be NULL when no row_ref is >= 0 */
} ba_match_batch;

typedef struct {
  float   ratio;                 /* default 0.7f (FeatureProcessor.cpp:58) */
  int32_t unique;                /* default 1 */
  float   max_distance;          /* default +inf */
  int32_t reserved;              /* 0 */
} ba_match_options;

typedef struct {
  int32_t query, train;          /* local row indices of the pair's two sets */
  float   distance, second_distance;
  float   ref_distance;          /* -1 without a reference descriptor */
} ba_match;

typedef struct {                 /* ba_match_knn: one query, before any filtering */
  int32_t idx0, idx1;            /* -1: none */
  float   d2_0, d2_1;            /* squared distances; +inf: none */
} ba_match_neighbors;

void ba_match_defaults(ba_match_options* opt);
int ba_match_descriptors(ba_ctx* ctx, const ba_match_batch* batch, const ba_match_options* opt /* NULL = defaults */,
                         int32_t* match_offset /* [n_pairs+1] */, ba_match* matches /* capacity: see Output */);
/* Times (ms) of the last successful ba_match_descriptors: [0] host
 * preparation, [1] the kernels (device), [2] the whole call, then the phases
 * of [1]: [3] norms, [4] the 2-NN contraction, [5] merge, ratio, unique filter
 * and compaction.  As ba_pnp_times otherwise. */
int ba_match_times(ba_ctx* ctx, double* ms, int n);
/* Test / inspection entry point, in the role of ba_two_view_hypotheses: the
 * dense 2-NN record of every query of pair `pair` exactly as
 * ba_match_descriptors forms it, before the ratio test.  Same errors as
 * ba_match_descriptors (no options are read), plus a pair out of range. */
int ba_match_knn(ba_ctx* ctx, const ba_match_batch* batch, int pair, ba_match_neighbors* out /* [n_q of the pair] */);

/* ---------------------------------------------------------------------------
 * ba_map_points_update: the upkeep of every map point on the device: its
 * representative descriptor (MapPoint::computeDescriptor, MapPoint.cpp:202-252),
 * its mean viewing direction and its depth bounds
 * (MapPoint::computeViewingDirection, MapPoint.cpp:166-200).  The reference
 * runs both for every map point after every BA (SfMHelper::eraseOutlier) and
 * on every addObservation / replaceObservation / fuse.  The outputs are what
 * ba_prune (obs_dist), ba_match_descriptors (ref_desc) and ba_associate read.
 * csrc/ba_map_points.h is the text, the same on the device and in host
 * programs.
 *
 * Batch.  Point p owns observations [obs_offset[p], obs_offset[p+1]): its
 * track, n observations, at most BA_MP_MAX_TRACK.  Observation o is seen by
 * keyframe obs_cam[o] (camera centre cam_center[3 obs_cam[o]]) through the
 * keypoint whose descriptor is row obs_row[o] of desc; a row may be named by
 * any number of observations.  Descriptors are expected finite.
 *
 * Order.  The reference walks a std::map keyed by pointer, so its order is
 * unspecified; here the order is the caller's.
 *
 * Distances.  D[i][j] is the distance of ba_match_descriptors between rows
 * obs_row[i] and obs_row[j]: (float)sqrt((double)d2) with d2 = max(0,
 * fmaf(-2, dot, nrm_i + nrm_j)) and the fmaf chains in ascending k.  D[i][i]
 * is exactly 0; D[i][j] and D[j][i] are bitwise equal (the chain's products
 * and the sum of the norms commute); two observations naming one row are at
 * distance 0.
 *
 * Row median.  k = max(0, n/2 - 1) in integer division: the reference's
 * curDistances[(n / 2.0) - 1] after truncation (0 for n <= 3, 1 for n = 4 and
 * 5, 31 for n = 64 and 65).  m_i is the k-th smallest value (0-based) of row
 * i, the self-distance included, formed by rank: the value whose key
 * bits(D[i][j]) << 32 | j has exactly k smaller keys in the row.  The value
 * does not depend on how ties are ordered.
 *
 * Choice.
 *   BA_MP_MEDIAN_REFERENCE (default) restates the reference line for line:
 *     t_i = (int32_t)m_i, truncated toward zero (the reference stores the
 *     median in an int; INT32_MAX from 2^31 on), and best is the lowest i with
 *     the smallest t_i (a strict < starting at INT_MAX).  With unit-norm SURF
 *     rows every distance is below 2, every t_i is 0 and the reference keeps
 *     observation 0: that is its behaviour, and the default keeps it, as
 *     behind_rule = 0 does in ba_triangulate.
 *   BA_MP_MEDIAN_FLOAT is what the reference's comment intends: the smallest
 *     key bits(m_i) << 32 | i.  For n = 4 and 5 (k = 1) the median of a row is
 *     its nearest-neighbour distance, so the two mutually nearest rows tie
 *     bitwise and the lower index wins.
 *   median = m_best.  With desc_out, row obs_row[best] is copied bit for bit.
 *
 * Viewing direction (float, round to nearest, no contraction, IEEE division
 * and square root).  For each observation in caller order: v = X - c per
 * component, s = (v0 v0 + v1 v1) + v2 v2, u = s > 0 ? v / sqrt(s) : v
 * (Eigen's normalized()); sum += u per component from 0; view_dir = sum /
 * (float)n.
 *
 * Depth bounds.  With r = ref_obs[p] (the reference keyframe's observation):
 * d = sqrt((w0 w0 + w1 w1) + w2 w2), w = X - c_r (ba_prune's worldDist);
 * max_dist = d * obs_scale[r]; min_dist = max_dist / max_scale.
 *
 * Empty track.  n = 0 gives BA_MP_EMPTY, best = -1 and zeros in the other
 * fields and in the desc_out row.
 *
 * Contract, as ba_match_descriptors: a point's output bits depend only on its
 * own data and the options, not on its place in the batch or on the other
 * points (every float is formed by one thread in a fixed order and every
 * selection is on integer keys, so the route a track length takes does not
 * matter either); two calls give bitwise equal output; the context's current
 * problem is untouched; no collective; the call blocks until the results are
 * on the host.  An empty batch is valid.
 *
 * Errors (the context stays usable; nothing is launched; all validation is on
 * the host):
 *   BA_ERR_INVALID_ARGUMENT  a NULL required array, dim other than 64 / 128,
 *                            negative counts, obs_offset[0] != 0 or a
 *                            decreasing obs_offset (the message names the
 *                            point), a track longer than BA_MP_MAX_TRACK, an
 *                            obs_cam, obs_row or ref_obs out of range (the
 *                            message names the observation or the point), an
 *                            unknown median_rule, a max_scale that is not
 *                            positive and finite, a non-zero reserved field,
 *   BA_ERR_OUT_OF_MEMORY     the staging buffer cannot be allocated. */
#define BA_MP_MAX_TRACK 1024
enum ba_mp_status { BA_MP_OK = 0, BA_MP_EMPTY = 1 };
enum ba_mp_median { BA_MP_MEDIAN_REFERENCE = 0, BA_MP_MEDIAN_FLOAT = 1 };

typedef struct {
  int32_t dim;                   /* 64 or 128 */
  int32_t n_cams, n_pts, n_rows;
  const float*   cam_center;     /* [3*n_cams] getWorldPos() (= getPose().block(0,3,3,1)) */
  const float*   pts;            /* [3*n_pts]  MapPoint::getPosition() */
  const int32_t* obs_offset;     /* [n_pts+1], [0] = 0, non-decreasing: point p owns its track */
  const int32_t* obs_cam;        /* [n_obs] observing keyframe */
  const int32_t* obs_row;        /* [n_obs] row of desc: the observing keypoint's descriptor */
  const float*   obs_scale;      /* [n_obs] (float)pow(1.2, octave); NULL = all 1 (as ba_tri_batch) */
  const int32_t* ref_obs;        /* [n_pts] local index, within the track, of the reference keyframe's
                                    observation; NULL = 0 */
  const float*   desc;           /* [n_rows*dim] row-major */
} ba_map_point_batch;

typedef struct {
  int32_t median_rule;           /* default BA_MP_MEDIAN_REFERENCE */
  int32_t reserved;              /* 0 */
  float   max_scale;             /* default (float)pow(1.2, 7) = 3.5831808f */
  float   reserved_f;            /* 0 */
} ba_map_point_options;

typedef struct {                 /* 32 bytes */
  int32_t status, best;          /* best: local index within the track of the chosen descriptor; -1 if EMPTY */
  float   median;                /* m_best */
  float   view_dir[3];
  float   min_dist, max_dist;
} ba_map_point;

void ba_map_points_defaults(ba_map_point_options* opt);
int ba_map_points_update(ba_ctx* ctx, const ba_map_point_batch* batch, const ba_map_point_options* opt /* NULL = defaults */,
                         ba_map_point* out /* [n_pts] */, float* desc_out /* [n_pts*dim], may be NULL */);
/* Times (ms) of the last successful ba_map_points_update: [0] host
 * preparation, [1] the kernels (device), [2] the whole call.  As
 * ba_match_times otherwise. */
int ba_map_points_times(ba_ctx* ctx, double* ms, int n);
/* Test / inspection entry point, in the role of ba_match_knn: the dense n x n
 * distance matrix and the n row medians of point `point`, exactly as
 * ba_map_points_update forms them.  Same errors (no options are read), plus a
 * point out of range. */
int ba_map_points_distances(ba_ctx* ctx, const ba_map_point_batch* batch, int point, float* D /* [n*n] */, float* m /* [n] */);

/* ---------------------------------------------------------------------------
 * ba_associate: the gates of SfMHelper::searchInNeighbors
 * (SfMHelper.cpp:254-479) per candidate association, as a pure function of a
 * snapshot.  The caller keeps the object graph and the case analysis (which
 * side of a match has a map point); the two middle branches of the reference
 * are one test with the roles swapped, so an item is (camera, keypoint, map
 * point) and a fuse pair is (point, point).
 *
 * Item (item_cam c, keypoint at item_uv with descriptor row item_row, map
 * point item_pt at X).  The gates run in the reference's order
 * (SfMHelper.cpp:272-353); the first that fails gives the status, and fields
 * that were not reached are -1.  Float, round to nearest, no contraction, the
 * operation order of ba_prune:
 *   v = extr_c * [X; 1], cz = v2 / v3; cz <= 0 is BA_AS_BEHIND;
 *   q = K_c * (v0 / v3, v1 / v3, cz) accumulated column by column, px = q0 /
 *     q2, py = q1 / q2; px < 0 || px >= (float)w || py < 0 || py >= (float)h
 *     is BA_AS_BOUNDS;
 *   chi = sqrt(e0 e0 + e1 e1) * invSigma with e = (px, py) - uv and invSigma =
 *     (float)(1.0 / (double)item_scale); chi > chi2 is BA_AS_CHI2 (a norm, as
 *     in ba_prune);
 *   cosine = (w0 n0 + w1 n1) + w2 n2 with w the normalised X - centre_c (as
 *     the viewing direction above) and n = pt_view_dir; cosine < min_cos is
 *     BA_AS_ANGLE (a NaN passes, as in the reference);
 *   world_dist = |X - centre_c|; world_dist > max || world_dist < min of
 *     pt_dist is BA_AS_DEPTH;
 *   dist_matched = the descriptor distance (ba_match_descriptors' formulas)
 *     from desc[item_row] to pt_desc[item_pt].  Not yet observed
 *     (item_cur_row < 0): dist_matched < max_desc_dist gives BA_AS_ADD, else
 *     BA_AS_DESC.  Already observed: dist_current is the distance from
 *     desc[item_cur_row] to pt_desc[item_pt]; dist_matched < dist_current
 *     gives BA_AS_REPLACE, else BA_AS_WORSE.
 * Fuse pair (p, q): cosine = (a0 b0 + a1 b1) + a2 b2 of the two view
 * directions; cosine < fuse_min_cos is BA_FUSE_ANGLE (dist = -1); dist = the
 * distance between the two pt_desc rows; dist < fuse_max_desc_dist gives
 * BA_FUSE_OK, else BA_FUSE_DESC.  Which point survives stays with the caller
 * (getNumObserved).
 *
 * Contract and errors as ba_map_points_update; the message names the item.
 * BA_ERR_INVALID_ARGUMENT: a NULL required array, dim other than 64 / 128,
 * negative counts, an item_cam, item_pt, item_row, item_cur_row (below -1 or
 * beyond n_rows) or fuse_pairs entry out of range, a non-zero reserved. */
enum ba_assoc_status { BA_AS_ADD = 0, BA_AS_REPLACE = 1, BA_AS_BEHIND = 2, BA_AS_BOUNDS = 3, BA_AS_CHI2 = 4,
                       BA_AS_ANGLE = 5, BA_AS_DEPTH = 6, BA_AS_DESC = 7, BA_AS_WORSE = 8 };
enum ba_fuse_status  { BA_FUSE_OK = 0, BA_FUSE_ANGLE = 1, BA_FUSE_DESC = 2 };

typedef struct {
  int32_t dim, n_cams, n_pts, n_rows, n_items, n_fuse;
  const float *extr, *cam_center, *K;   /* as ba_prune_problem */
  const int32_t* image_size;            /* [2*n_cams] width, height */
  const float *pts, *pt_view_dir;       /* [3*n_pts] each */
  const float *pt_dist;                 /* [2*n_pts] min, max (ba_prune's obs_dist, per point) */
  const float *pt_desc;                 /* [n_pts*dim] (desc_out of ba_map_points_update) */
  const float *desc;                    /* [n_rows*dim] keypoint descriptors */
  const int32_t *item_cam, *item_pt;    /* [n_items] */
  const float   *item_uv;               /* [2*n_items] */
  const float   *item_scale;            /* [n_items] pow(1.2, octave); NULL = 1 */
  const int32_t *item_row;              /* [n_items] the matched keypoint's descriptor row */
  const int32_t *item_cur_row;          /* [n_items] row of the keypoint through which item_cam already observes
                                           item_pt, -1 if it does not; NULL = none */
  const int32_t *fuse_pairs;            /* [2*n_fuse] */
} ba_assoc_batch;

typedef struct {
  float chi2, min_cos, max_desc_dist, fuse_min_cos, fuse_max_desc_dist;   /* defaults 5.991f, 0.5f, 0.2f, 0.0f, 0.3f */
  int32_t reserved;                                                       /* 0 */
} ba_assoc_options;

typedef struct { int32_t status; float chi, cosine, world_dist, dist_matched, dist_current; } ba_assoc_result;
typedef struct { int32_t status; float cosine, dist; } ba_fuse_result;

void ba_associate_defaults(ba_assoc_options* opt);
int ba_associate(ba_ctx* ctx, const ba_assoc_batch* batch, const ba_assoc_options* opt /* NULL = defaults */,
                 ba_assoc_result* items /* [n_items] */, ba_fuse_result* fuse /* [n_fuse] */);

/* ba_map_graph: the covisibility lists, the culling votes and the local-BA
 * windows of a batch of query frames, as a stateless function of a
 * point-sorted observation table (the layout of ba_map_point_batch).  It
 * restates Frame::updateCovisibilityGraph / getBestCovisibilityFrames
 * (Frame.cpp:292-386), SfMHelper::cullRedundantKeyframes and the erase rule
 * of cullRecentMapPoints / eraseOutlier (SfMHelper.cpp:974-1111) and the
 * window of LocalBAOptimizerAngles (ba_optimizer.hpp:341-374) on indices.
 * Everything is integers, so the result is exactly the restatement whatever
 * the batching.  The table is expected to hold a (frame, point) pair at most
 * once; it is not validated, and the rules are stated per observation, so
 * duplicates still have a defined result.
 *
 * For a query frame q:
 *   weights   for g != q, W_q[g] = the number of pairs (o, o') with
 *             obs_frame[o] = q, obs_outlier[o] = 0, o' in the same track and
 *             obs_frame[o'] = g.  pt_invalid and the outlier flag of o' are
 *             not tested (Frame.cpp:301-321), so W is not symmetric once
 *             outliers exist.
 *   list L_q  the candidates are the g with W_q[g] > th (strict) and
 *             frame_is_key[g].  No candidate but some W_q[g] > 0: the single
 *             fallback g*, the lowest index among the largest weights, no
 *             keyframe test (Frame.cpp:352-357), status BA_GRAPH_FALLBACK.
 *             Every weight 0: the empty list, BA_GRAPH_ISOLATED (the
 *             reference dereferences a null frame).  Else BA_GRAPH_OK.  The
 *             list is ascending by the key W << 32 | g (the reference's ties
 *             fall in pointer order, here in frame-index order).
 *             degree = |L_q|, max_weight = the largest W_q[g] over all g.
 *   best      the first min(n_best, |L_q|) entries of the list:
 *             BA_GRAPH_WEAKEST_FIRST takes the ascending list (what the
 *             reference does), BA_GRAPH_STRONGEST_FIRST the list by
 *             descending weight, ties in ascending index (what it intends).
 *   vote      n_map = the o with obs_frame[o] = q whose point is not invalid
 *             (no outlier test).  Such an o is redundant when its track is
 *             longer than 3 and at least 3 observations o' of the track have
 *             obs_frame[o'] != q and obs_octave[o'] <= obs_octave[o] + 1.
 *             cull = frame_id[q] is neither 0 nor 1 and
 *             (double)n_map * redundant_fraction < (double)n_redundant
 *             (SfMHelper.cpp:1019-1074; 0.95 is the code's value).
 *   window    (build_windows != 0) local frames: the best frames in list
 *             order, then q.  Local points: the p with pt_invalid[p] = 0 that
 *             have a non-outlier observation by a local frame, ascending.
 *             Fixed frames: the keyframes g, not local, with a non-outlier
 *             observation of a local point, ascending.  Window observations:
 *             the o of a local point with obs_outlier[o] = 0 and a local or
 *             fixed frame, ascending (so sorted by point).  Window cameras:
 *             the local frames, then the fixed frames; a camera's fixed flag
 *             is set when it is a fixed frame or its frame_id is 0.
 *   pt_status (when the array is given) with age = current_frame_id -
 *             frame_id[pt_ref_frame[p]] and n the track length:
 *             BA_GRAPH_PT_INVALID if pt_invalid[p], else BA_GRAPH_PT_ERASE if
 *             age >= 4 && n <= 2, else BA_GRAPH_PT_MATURE if age >= 5, else
 *             BA_GRAPH_PT_RECENT.
 *
 * A query's output depends only on the table, the options and q: not on its
 * place in the batch, the other queries (duplicates are allowed), the column
 * tile or the chunking.  Two calls give bitwise equal output.  The context's
 * current problem is untouched, there is no collective, and the call blocks
 * until the records are on the host.  The variable-length lists stay on the
 * device until the next ba_map_graph or ba_destroy; ba_map_graph_lists copies
 * them out.  An empty batch is valid.
 *
 * Errors: everything is validated on the host before anything is launched, and
 * the message names the point, observation or query.
 *   BA_ERR_INVALID_ARGUMENT  a NULL required array; negative counts;
 *                            obs_offset[0] != 0 or a decreasing obs_offset; an
 *                            obs_frame, pt_ref_frame or query out of range;
 *                            n_best outside 0 .. BA_WINDOW_MAX_CAMS - 1; an
 *                            unknown order; a negative th; a non-finite
 *                            redundant_fraction; a negative debug field; a
 *                            non-zero reserved field; pt_status without
 *                            pt_ref_frame,
 *   BA_ERR_OUT_OF_MEMORY     a buffer cannot be allocated. */
typedef struct {
  int32_t n_frames, n_pts, n_obs, reserved;
  const int32_t *frame_id;       /* [n_frames] Frame::getID() */
  const uint8_t *frame_is_key;   /* [n_frames]; NULL = all 1 */
  const uint8_t *pt_invalid;     /* [n_pts]; NULL = all 0 */
  const int32_t *pt_ref_frame;   /* [n_pts] frame index of the reference keyframe; NULL allowed without pt_status */
  const int32_t *obs_offset;     /* [n_pts + 1]: point p owns observations [obs_offset[p], obs_offset[p+1]) */
  const int32_t *obs_frame;      /* [n_obs] observing frame */
  const int32_t *obs_octave;     /* [n_obs] keypoint octave; NULL = all 0 */
  const uint8_t *obs_outlier;    /* [n_obs] Frame::isOutlier; NULL = all 0 */
} ba_map_table;

enum ba_graph_status { BA_GRAPH_OK = 0, BA_GRAPH_FALLBACK = 1, BA_GRAPH_ISOLATED = 2 };
enum ba_graph_order { BA_GRAPH_WEAKEST_FIRST = 0, BA_GRAPH_STRONGEST_FIRST = 1 };
enum ba_graph_pt_status { BA_GRAPH_PT_RECENT = 0, BA_GRAPH_PT_MATURE = 1, BA_GRAPH_PT_ERASE = 2, BA_GRAPH_PT_INVALID = 3 };

typedef struct {
  int32_t th;                  /* a covisibility edge needs more than th shared points; default 10 */
  int32_t n_best;              /* default 10 */
  int32_t order;               /* ba_graph_order; default BA_GRAPH_WEAKEST_FIRST */
  int32_t build_windows;       /* default 1 */
  int32_t current_frame_id;    /* read for pt_status only; default 0 */
  int32_t debug_tile_frames;   /* column tile of the weight histogram; 0 = automatic */
  int32_t debug_chunk_queries; /* queries per chunk; 0 = from the scratch budget */
  int32_t reserved;            /* 0 */
  double  redundant_fraction;  /* default 0.95 */
} ba_graph_options;

typedef struct {
  int32_t status, degree, max_weight, n_map, n_redundant, cull, n_local, n_fixed, n_win_pts, n_win_obs;
} ba_graph_frame;

/* The variable-length results of the last successful ba_map_graph, query after
 * query in query order; any array may be NULL.  Lengths (sums over the
 * records): nbr_* sum(degree); win_cam* sum(n_local + n_fixed); win_pt
 * sum(n_win_pts); win_obs* sum(n_win_obs).  win_obs is the index into the
 * table; win_obs_cam and win_obs_pt are local to the window (positions in
 * its win_cam and win_pt), the form ba_window_batch wants. */
typedef struct {
  int32_t *nbr_frame, *nbr_weight;
  int32_t *win_cam;
  uint8_t *win_cam_fixed;
  int32_t *win_pt;
  int32_t *win_obs, *win_obs_cam, *win_obs_pt;
} ba_graph_lists;

void ba_map_graph_defaults(ba_graph_options* opt);
int ba_map_graph(ba_ctx* ctx, const ba_map_table* table, const int32_t* query /* [n_query] */, int n_query,
                 const ba_graph_options* opt /* NULL = defaults */, ba_graph_frame* out /* [n_query] */,
                 uint8_t* pt_status /* [n_pts] or NULL */);
/* BA_ERR_INVALID_ARGUMENT before any successful ba_map_graph on the context. */
int ba_map_graph_lists(ba_ctx* ctx, const ba_graph_lists* out);
/* Test / inspection: the raw row W_frame[n_frames] (W[frame] = 0) exactly as
 * ba_map_graph forms it; opt (NULL = defaults) is read for debug_tile_frames. */
int ba_map_graph_weights(ba_ctx* ctx, const ba_map_table* table, int frame, const ba_graph_options* opt, int32_t* W);
/* Times (ms) of the last successful ba_map_graph: [0] host preparation
 * (wall), [1] the kernels (device), [2] the whole call (wall).  Copies
 * min(n, 3) values and returns 3 (0 before the first call). */
int ba_map_graph_times(ba_ctx* ctx, double* ms, int n);

/* ---------------------------------------------------------------------------
 * ba_icp: batched point-to-point ICP of point clouds and its fitness score:
 * the arithmetic behind the reference's reconstruction error
 * (ReconstructionError.cpp:134-190: pcl::IterativeClosestPoint with every
 * default, align, hasConverged, getFitnessScore).  PCL was not available where
 * this was written: the rules below restate PCL 1.12's documented defaults as
 * recalled and are pinned here (csrc/ba_icp.h is the text, the same on the
 * device and in host programs); INTEGRATION.md lists what to verify against a
 * PCL build.  PCL's kd-tree search is exact, so the exact nearest neighbour is
 * what is pinned.
 *
 * Batch.  n_sets clouds in CSR form: set s owns points
 * [set_offset[s], set_offset[s+1]) of xyz (3 floats per point).  Pair i aligns
 * the points of set pair_src[i] (the source) to those of set pair_tgt[i] (the
 * target); a set may appear in any number of pairs and is uploaded once.
 * guess: per pair a float 4x4, row-major, applied to the source first (its
 * first three rows are read; the last is taken as 0 0 0 1); NULL = identity.
 *
 * Per iteration, on cur (float; cur_0 = guess * source):
 *  1. Correspondences.  For a source point p and a target point q (float,
 *     every operation rounded on its own, nothing contracted):
 *       d2 = ((dx*dx + dy*dy) + dz*dz),   dx = p.x - q.x, ...
 *     The neighbour of p is the target index j of smallest key
 *     (bits(d2) << 32 | j): ties go to the lowest index.  p is kept iff
 *     d2 <= max_corr_dist * max_corr_dist (a float product); a point that is
 *     not kept has index -1 and d2 = +inf.
 *  2. Fewer than min_correspondences kept: state NO_CORRESPONDENCES,
 *     converged = 0, the loop stops (iterations is not advanced).
 *  3. Rigid estimate (Umeyama; TransformationEstimationSVD), fp64: sums of
 *     a = cur - c0 and b = target - c0 (c0: the centre of the target's bounding
 *     box) over the kept points in a fixed order; means ma, mb;
 *     H = sum b a^T - n mb ma^T = U diag(s) V^T by one-sided Jacobi with U, V
 *     rotations (the reflection case carries its sign on the smallest singular
 *     value, which is Umeyama's sign matrix); R = U V^T;
 *     c = (s0 + s1 +- s2) / (sum |a|^2 - n |ma|^2) with with_scale, else 1;
 *     t = (c0 + mb) - c R (c0 + ma).  c R and t are rounded to float.  A
 *     non-finite R (the kept source points are collinear) is replaced by the
 *     identity with c = 1.
 *  4. Update.  cur <- (c R) cur + t as ((m0*x + m1*y) + m2*z) + t per row, and
 *     final <- T_k final as a float 4x4 product, terms in ascending k (final
 *     starts as the guess).
 *  5. Convergence (DefaultConvergenceCriteria), in this order, after
 *     iterations += 1:
 *       iterations >= max_iterations                        -> ITERATIONS
 *       (tr(cR) - 1) / 2 >= 1 - transformation_eps and
 *         |t|^2 <= transformation_eps (fp64 of the floats)  -> TRANSFORM
 *       mse = fp64 mean of the kept float d2;
 *       |mse - prev| < mse_abs_eps                          -> ABS_MSE
 *       mse_rel_eps > 0 and |mse - prev| / prev < mse_rel_eps -> REL_MSE
 *     each with converged = 1; otherwise prev = mse (initially DBL_MAX).
 *     mse[k] of iteration k is recorded whichever rule ends the loop.
 *
 * Fitness (getFitnessScore).  For a converged pair, one more correspondence
 * pass on the final cur: the fp64 mean of d2 over the points with
 * d2 <= fitness_max_range, DBL_MAX when there is none.  A pair that did not
 * converge has fitness DBL_MAX (the reference reports its maximum there).
 *
 * Search.  Targets above a size threshold (route AUTO) are searched through a
 * uniform grid over the target's bounding box, built once on the host; the
 * ring walk stops only when every unvisited cell is provably farther than the
 * best key found, so GRID, BRUTE and every cell size give the same bits.
 * cell > 0 overrides the grid's cell size (debug).
 *
 * Contract, as ba_match_descriptors: a pair's output bits depend only on its
 * own data and the options, not on its place in the batch, on the other
 * pairs, on route or on cell; two calls give bitwise equal output; no float
 * atomics; the context's current problem is untouched; no collective; the
 * call blocks until the results are on the host.  An empty batch is valid.
 *
 * Errors (the context stays usable; nothing is launched; all validation is on
 * the host; the message names the culprit):
 *   BA_ERR_INVALID_ARGUMENT  a NULL required array, negative counts, a bad
 *                            set_offset, a pair's set index out of range, a
 *                            source of fewer than 3 points, an empty target,
 *                            a non-finite coordinate (the message names the
 *                            set and the point) or guess, max_iterations < 1
 *                            or > 10000, min_correspondences < 3, a negative
 *                            or NaN max_corr_dist / fitness_max_range / cell,
 *                            a NaN epsilon, with_scale other than 0 / 1, an
 *                            unknown route, reserved != 0,
 *   BA_ERR_OUT_OF_MEMORY     the scratch cannot be allocated. */
#define BA_ICP_ROUTE_AUTO 0
#define BA_ICP_ROUTE_GRID 1
#define BA_ICP_ROUTE_BRUTE 2
/* ba_icp_result.state (PCL's ConvergenceState) */
#define BA_ICP_NOT_CONVERGED 0
#define BA_ICP_ITERATIONS 1
#define BA_ICP_TRANSFORM 2
#define BA_ICP_ABS_MSE 3
#define BA_ICP_REL_MSE 4
#define BA_ICP_NO_CORRESPONDENCES 5

typedef struct {
  int32_t n_sets, n_pairs;
  const int32_t* set_offset;     /* [n_sets+1], [0] = 0, non-decreasing: points of xyz */
  const float*   xyz;            /* [3 * points] */
  const int32_t* pair_src;       /* [n_pairs] set index of the source */
  const int32_t* pair_tgt;       /* [n_pairs] set index of the target */
  const float*   guess;          /* [n_pairs][16] row-major, or NULL = identity */
} ba_icp_batch;

typedef struct {
  int32_t max_iterations;        /* default 10 */
  float   max_corr_dist;         /* default +inf (PCL: sqrt(DBL_MAX), which rejects nothing) */
  double  mse_abs_eps;           /* default 1e-12 */
  double  mse_rel_eps;           /* default 0: <= 0 is off (PCL: euclidean_fitness_epsilon = -DBL_MAX) */
  double  transformation_eps;    /* default 0 */
  int32_t min_correspondences;   /* default 3 */
  int32_t with_scale;            /* default 0 */
  float   fitness_max_range;     /* default +inf; compared with d2 */
  int32_t route;                 /* default BA_ICP_ROUTE_AUTO */
  float   cell;                  /* default 0: the planned cell size; > 0 overrides it (never changes a result bit) */
  int32_t reserved;              /* 0 */
} ba_icp_options;

typedef struct {
  float   final[16];             /* row-major 4x4: the guess times every step */
  int32_t converged, state;
  int32_t iterations, n_corr;    /* n_corr: kept correspondences of the last iteration */
  double  fitness;
} ba_icp_result;

void ba_icp_defaults(ba_icp_options* opt);
/* mse: [n_pairs][max_iterations] (entries past a pair's iterations are 0), or NULL */
int ba_icp(ba_ctx* ctx, const ba_icp_batch* batch, const ba_icp_options* opt /* NULL = defaults */,
           ba_icp_result* out /* [n_pairs] */, double* mse);
/* Times (ms) of the last successful ba_icp: [0] host preparation (wall: the
 * checks, the grids, the source permutations), [1] the kernels (device),
 * [2] the whole call (wall), [3] [1] per enqueued round (max_iterations + 1).
 * As ba_match_times otherwise. */
int ba_icp_times(ba_ctx* ctx, double* ms, int n);
/* Test / inspection entry point, in the role of ba_match_knn: one
 * correspondence pass of pair `pair` on guess * source through the route the
 * options select (opt NULL = defaults; route, cell and max_corr_dist are
 * read): idx[n_src] (-1: not kept) and d2[n_src].  Same errors as ba_icp, plus
 * a pair out of range. */
int ba_icp_nn(ba_ctx* ctx, const ba_icp_batch* batch, int pair, const ba_icp_options* opt, int32_t* idx, float* d2);

/* Test / inspection entry point: the state inside ceres::Solve's
 * SchurComplementSolver (Optimizer.cpp:242, DENSE_SCHUR) for one step.
 * Linearises at the current parameters with iteration-0 Jacobi scaling, then
 * forms the reduced camera system at trust-region radius `radius` with the
 * very kernels a solve's step runs (J-free consumers, compact or 18-double W
 * records, LDS or global camera tables: whatever the problem size selects),
 * without factoring it, and copies out (caller indices; any pointer may be
 * NULL):
 *   Hpp[6*n_pts]  J_p^T J_p per point (xx, xy, xz, yy, yz, zz; unscaled,
 *                 Huber-corrected J; zero for constant points),
 *   gp[3*n_pts]   J_p^T r,
 *   Hcc[21*n_cams] J_c^T J_c (lower triangle, row-major: (a, b), b <= a),
 *   gc[6*n_cams]  J_c^T r (zero for constant / unobserved cameras),
 *   S[n*n]        the reduced system s_c (Hcc - sum W W^T) s_c + D^2 as the
 *                 Cholesky receives it (row-major, lower triangle; upper 0),
 *   rhs[n]        its right-hand side,
 * with n = *n_out = 6 x the observed variable cameras in increasing camera
 * index (Jacobi-scaled columns, as Ceres' DENSE_SCHUR forms them). */
int ba_debug_blocks(ba_ctx* ctx, double radius, double* Hpp, double* gp, double* Hcc, double* gc, double* S,
                    double* rhs, int* n_out);

/* Test / inspection: the dispatch decisions the host has made for the current
 * problem, as of the last ba_solve / ba_debug_blocks (a read-only copy of host
 * state: nothing is built and nothing is launched; before the first solve the
 * structures are not built and their fields are 0).  Writes the first
 * min(n, BA_DEBUG_PLAN_FIELDS) of these int32 values to out, in this order:
 *    0 nvc           observed variable cameras (the reduced system has 6 nvc rows)
 *    1 nblocks       DENSE_SCHUR pair blocks (co-observed camera pairs, (I, I) included)
 *    2 neblocks      lower blocks of S no pair writes, zeroed from a list each step
 *    3 s_memset      ... or the whole of S is cleared by a memset each step
 *    4 dup_diag      a pair block (I, I) exists (a point seen twice by one camera)
 *    5 chol_persist  the factorisation runs as one persistent launch
 *    6 ov_ok         the overlapped form's plan was built (S formed in that launch)
 *    7 wcompact      W as compact 128-byte records
 *    8 jdiag         the diagonal Schur blocks formed without stored J
 *    9 jrfree        the iteration never stores J (0: BA_JR=1)
 *   10 have_dense    the DENSE_SCHUR structures are built
 *   11 have_pcg      the ITERATIVE_SCHUR structures are built
 *   12 npchunks      point-aligned chunks of the PCG point pass (0: a point has
 *                    more than 64 observations, or BA_PCG_SEG=0)
 *   13 pcg_ndup      ITERATIVE_SCHUR duplicate (camera, point) observation pairs
 *   14 pcgc          the PCG point pass reads the 16-value records
 *   15 pacc          the back substitution uses the CG's accumulated point products
 *   16 pcgjf         the PCG point pass forms its records itself (no W)
 * Fields 7-9 and 14-16 are decided per step from the options and the
 * environment: they describe the last step enqueued.
 * Errors: BA_ERR_INVALID_ARGUMENT for a NULL ctx or out or n < 0 (no device
 * needed); BA_ERR_NO_PROBLEM before ba_set_problem. */
#define BA_DEBUG_PLAN_FIELDS 17
int ba_debug_plan(ba_ctx* ctx, int32_t* out, int n);

/* Test / inspection: run the DENSE_SCHUR factorisation + back substitution a
 * solve's step runs (the context's own dispatch: whatever form the order and
 * the BA_CHOL_* knobs select) on a caller-supplied system of the current
 * problem's order n (= *n_out of ba_debug_blocks).
 *   S_in[n*n]  row-major, lower triangle read (upper ignored); rhs_in[n]
 *   L[(n+1)*n] row-major: rows < n the factor as the kernels leave it: the
 *              tiles left of each row's diagonal 64-block.  The diagonal
 *              64-blocks are NOT stored by the kernels (only their inverses
 *              V leave the workgroup that factors them); they and everything
 *              right of them come out as zeros, L_kk = V_k^-1 is the caller's
 *              to rebuild.  Row n = z = L^-1 rhs.  (n % 64 == 0: the rhs row is
 *              a tile row of its own and the kernels keep z's last block in
 *              LDS; the entry forms those 64 values on the host as the back
 *              substitution does, z_K = V_K A_{n,K}^T from the updated rhs
 *              row.)
 *   V[T*64*64] the explicit inverses of the diagonal blocks (T = ceil(n/64)),
 *              lower triangular, identity past a partial last block's order;
 *              the persistent form stores only the 16x16 blocks on and below
 *              the block diagonal of a full 64-block (the rest is never read
 *              and comes out as whatever the buffer held)
 *   y[n]       the solution of S y = rhs
 *   *ok        1, or 0 if the factorisation reported a non-positive pivot
 *              (a normal outcome: the call still returns BA_OK)
 * Any output pointer may be NULL.  The overlapped form, which builds S inside
 * its own launch, cannot take an injected matrix and is never selected here.
 * A hand-off spin bound is handled as in ba_covariance (one redo with the
 * per-step launches, else BA_ERR_DEVICE).  Afterwards the context is as
 * before the call: a ba_solve, ba_debug_blocks or ba_covariance on it is bit
 * for bit what it would have been.
 * Errors: BA_ERR_NO_PROBLEM before ba_set_problem; BA_ERR_INVALID_ARGUMENT
 * for n == 0, a NULL input, a context with a communicator, or a system too
 * large for DENSE_SCHUR. */
int ba_debug_factor(ba_ctx* ctx, const double* S_in, const double* rhs_in, double* L, double* V, double* y,
                    int* ok);

/* Marginal covariances of parameter blocks at the current parameters:
 * ceres::Covariance with its defaults.  The covariance is (J^T J)^-1 with J
 * the Huber-corrected Jacobian ba_linearize returns, taken over the variable
 * blocks in unscaled parameters: no LM damping, no residual-variance factor.
 * With H = J^T J = [[Hcc, Hcp], [Hpc, Hpp]]:
 *   cameras  Sigma_cc = (Hcc - Hcp Hpp^-1 Hpc)^-1; cam_cov block q is the
 *            6x6 Cov(cam_i, cam_j) of pair q = (i, j),
 *   point p  Hpp_p^-1 + Hpp_p^-1 (sum_{a,b in obs(p)} Hpc_a Sigma[c(a), c(b)]
 *            Hcp_b) Hpp_p^-1, 3x3.
 * Every block of a constant camera or constant point is all zeros, as in
 * Ceres.  Camera-point and point-point cross blocks: ba_covariance_ex.
 *
 * The call linearises at the current parameters (with that linearisation's
 * Jacobi scaling), forms and factors the undamped DENSE_SCHUR reduced system,
 * inverts the factor on the device and gathers the requested blocks; it
 * blocks until they are on the host.  It leaves the parameters unchanged, and
 * a later ba_solve on the context is bit for bit what it would have been
 * without the call.  Two calls at the same parameters give bitwise equal
 * output.
 *
 * The caller must remove the gauge: the covariance exists only where J has
 * full column rank.  With only one camera constant a monocular problem keeps
 * its scale freedom (the reduced system's condition number is then ~1e17), so
 * at least two cameras, or a camera and some points, must be constant.  A
 * nearly singular system may still factor; the call then returns large
 * finite values, not an error.
 *
 * Errors (the context stays usable after each):
 *   BA_ERR_NO_PROBLEM        before ba_set_problem,
 *   BA_ERR_INVALID_ARGUMENT  an index out of range; a requested block that
 *                            is variable but has no observation (the message
 *                            names it); a context with a communicator
 *                            (ba_comm_init / ba_comm_init_host); a system too
 *                            large for DENSE_SCHUR,
 *   BA_ERR_SINGULAR          a point block or the reduced system is not
 *                            positive definite, or a requested entry is not
 *                            finite. */
typedef struct {
  int32_t n_cam_pairs, n_points;
  const int32_t* cam_pairs;  /* [2*n_cam_pairs] caller camera indices (i, j), any order, i == j allowed */
  double*        cam_cov;    /* [36*n_cam_pairs] row-major 6x6 Cov(cam_i, cam_j) */
  const int32_t* points;     /* [n_points] caller point indices */
  double*        pt_cov;     /* [9*n_points] row-major 3x3 */
} ba_covariance_request;
int ba_covariance(ba_ctx* ctx, const ba_covariance_request* req);

/* ba_covariance for any pair of parameter blocks, and the leverages of
 * observations, from the same single factorisation and inverse.  `base` is
 * served exactly as by ba_covariance (bitwise the same output).  With
 * Sigma = (J^T J)^-1 over the variable blocks, T_p = Hpp_p^-1 Hpc_p:
 *   cam_pt_cov    Cov(cam i, point p) = -(Sigma_cc T_p^T)[i], 6x3,
 *   pt_pt_cov     Cov(p, q) = T_p Sigma_cc T_q^T + delta_pq Hpp_p^-1, 3x3; for
 *                 p == q bitwise the marginal of `base`; Cov(p, q)^T and
 *                 Cov(q, p) are bitwise equal,
 *   leverage      h_o = J_o Sigma J_o^T, the 2x2 diagonal block of the hat
 *                 matrix J Sigma J^T of observation o (J_o = [Jc | Jp], 2x9;
 *                 a constant block contributes nothing; every duplicate of an
 *                 observation has its own h_o).  h_o is symmetric; with J of
 *                 full column rank the traces of all h_o sum to the number of
 *                 variable parameters.
 * Any block with a constant camera or constant point is all zeros; so is the
 * leverage of an observation whose two blocks are both constant.
 * Contract and errors are ba_covariance's: it linearises at the current
 * parameters, factors and inverts once whatever is requested, leaves the
 * parameters and the context as they were (a later ba_solve, ba_covariance or
 * ba_debug_blocks is bit for bit what it would have been), gives bitwise
 * equal output on a second call, and blocks until the results are on the
 * host.  BA_ERR_INVALID_ARGUMENT also for an observation index out of range;
 * BA_ERR_SINGULAR also for a non-finite requested entry of the new outputs. */
typedef struct {
  ba_covariance_request base;      /* camera pairs and point marginals, exactly as ba_covariance */
  int32_t n_cam_pt, n_pt_pairs;
  const int32_t* cam_pt;           /* [2*n_cam_pt] (camera, point), caller indices */
  double*        cam_pt_cov;       /* [18*n_cam_pt] row-major 6x3 Cov(cam, pt) */
  const int32_t* pt_pairs;         /* [2*n_pt_pairs] (p, q), any order, p == q allowed */
  double*        pt_pt_cov;        /* [9*n_pt_pairs] row-major 3x3 Cov(p, q) */
  int32_t n_lev, reserved;
  const int32_t* lev_obs;          /* [n_lev] caller observation indices; NULL with
                                      n_lev == n_obs: every observation in caller order */
  double*        leverage;         /* [4*n_lev] row-major 2x2 */
} ba_covariance_request_ex;
int ba_covariance_ex(ba_ctx* ctx, const ba_covariance_request_ex* req);

/* Device time (ms, HIP events) of the phases of the last successful
 * ba_covariance or ba_covariance_ex: [0] linearisation + reduced system (and
 * the J records when leverages are requested), [1] factorisation (the
 * launches of a DENSE_SCHUR step's), [2] inverse of the factor and
 * Sigma = L^-T L^-1, [3] all block gathers and the copies to the host.  Copies
 * min(n, 4) values, returns 4 (0 before the first call).  Diagnostic. */
int ba_covariance_times(ba_ctx* ctx, double* ms, int n);

/* ba_covariance's request (camera pairs and point marginals) without the
 * dense factor: the requested blocks come from a few block columns of
 * S_scaled^-1, each solved by preconditioned conjugate gradients on the
 * implicit reduced camera system (the ITERATIVE_SCHUR matvec, several
 * right-hand sides per pass over the per-observation blocks).  Neither S nor
 * its factor is formed, so the call serves problems DENSE_SCHUR refuses.
 * Cross blocks and leverages stay with ba_covariance_ex.
 *
 * Semantics are ba_covariance's: (J^T J)^-1 over the variable blocks at the
 * current parameters, unscaled, undamped; blocks of constant cameras or
 * points are exact zeros; the gauge is the caller's to fix.  For a pair
 * (i, j) of variable cameras the block is read from the six columns of
 * camera j; a variable point needs the columns of all its variable observers.
 * Every column e is solved from x = 0 until |r|_2 <= tolerance (|e|_2 = 1)
 * or max_iterations, in the Jacobi-scaled system.  A block's bits depend only
 * on the problem, the parameters and the options, not on what else is
 * requested; two calls give bitwise equal output.  Cov(i, j) and Cov(j, i)^T
 * come from different columns: they agree to the tolerance, not bitwise.
 *
 * A column that does not converge is not an error: the call returns BA_OK,
 * the outputs are formed from the last iterate and `info` reports it.
 * Errors (the context stays usable after each; a later ba_solve,
 * ba_covariance or ba_debug_blocks is bit for bit what it would have been):
 *   BA_ERR_NO_PROBLEM        before ba_set_problem,
 *   BA_ERR_INVALID_ARGUMENT  ba_covariance's, and: a tolerance that is not
 *                            positive and finite, max_iterations < 1, an
 *                            unknown preconditioner; a context with a
 *                            communicator,
 *   BA_ERR_SINGULAR          a point block or a preconditioner block is not
 *                            positive definite, the CG broke down (p^T S p
 *                            <= 0 or not finite), or a requested entry is not
 *                            finite. */
typedef struct {
  int32_t preconditioner_type;   /* BA_JACOBI | BA_SCHUR_JACOBI (default BA_SCHUR_JACOBI) */
  int32_t max_iterations;        /* per column, default 500 */
  double  tolerance;             /* tau: a column stops when |r|_2 <= tau (|e|_2 = 1), default 1e-10 */
} ba_cov_iter_options;

typedef struct {
  int32_t n_columns;             /* 6 x distinct column cameras solved */
  int32_t n_converged;           /* columns that met tau within max_iterations */
  int32_t max_iterations_used, reserved;
  double  max_residual;          /* max over columns of the TRUE |e - S x|_2, recomputed by one matvec */
  double  ms[4];                 /* linearise+W+preconditioner | CG | residual check + gathers | copies */
} ba_cov_iter_info;

void ba_covariance_iterative_defaults(ba_cov_iter_options* opt);
int  ba_covariance_iterative(ba_ctx* ctx, const ba_covariance_request* req,
                             const ba_cov_iter_options* opt /* NULL = defaults */,
                             ba_cov_iter_info* info /* may be NULL */);

/* Diagnostic: device time (ms, HIP events, one pair per launch pair) of `reps`
 * implicit matvecs after `warmup` untimed ones, on the current problem with
 * ba_covariance_iterative's prologue and W records.  cols = 0: the
 * single-vector matvec of ITERATIVE_SCHUR on the same records; cols = 1, 2, 4:
 * the multi-column matvec with that many column cameras (6 cols columns).
 * ms[reps].  Single rank only; the context stays usable as after
 * ba_covariance_iterative. */
int ba_covariance_iterative_bench(ba_ctx* ctx, int cols, int reps, int warmup, double* ms);

/* Blocks until all device work of the context is done. */
int ba_synchronize(ba_ctx* ctx);

/* Timing hooks for bench.py: one LM iteration = linearise + assemble + Schur
 * + reduced solve (opt->linear_solver; NULL = defaults) + back-substitution +
 * candidate evaluation at a fixed trust-region radius (no accept/reject
 * bookkeeping).  Runs `iters` iterations on the context's stream and returns
 * the device-measured (HIP events) average milliseconds of the whole
 * iteration and of the residual+Jacobian kernel alone, and the mean number
 * of linear-solver iterations per LM iteration (may be NULL).  ms_rj_kernel
 * NULL: no event pair around the kernel (each pair's packets idle the device
 * ~5 us per iteration; bench.py times the kernel in a second pass). */
int ba_bench_iterations(ba_ctx* ctx, const ba_options* opt, int iters, double radius, double* ms_per_iter,
                        double* ms_rj_kernel, double* linear_iters);

/* Host wall time (ms) of each LM iteration of the last ba_bench_iterations
 * call: from one iteration's scalar record reaching the host to the next's
 * (the first from the call's start).  Copies min(n, available) values and
 * returns the number available (bench.py reports their median, BASELINE.md
 * §2, beside the mean over the timed region). */
int ba_bench_iteration_times(ba_ctx* ctx, double* ms, int n);

/* Measured copy bandwidth of the context's device ("also
 * report a measured STREAM-copy figure" beside the 8 TB/s peak): a
 * non-temporal 16-B load / store copy of `bytes` (rounded down to 16 B)
 * between two device buffers, `reps` timed launches after one warm-up, HIP
 * events on the context's stream.  *gbs = 2 * bytes * reps / time (read +
 * write).  Diagnostic; no reference counterpart. */
int ba_stream_copy(ba_ctx* ctx, size_t bytes, int reps, double* gbs);

#ifdef __cplusplus
}
#endif
#endif /* BA_HIP_H_ */
