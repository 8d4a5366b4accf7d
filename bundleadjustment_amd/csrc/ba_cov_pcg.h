// ba_cov_pcg.h — launch interface of the multi-column PCG on the implicit
// reduced camera system (ba_cov_pcg.hip; ba_covariance_iterative).
#pragma once
#include "ba_kernels.h"

namespace bahip {

constexpr int kMcgMaxB = 4;               // column cameras per pass: B in {1, 2, 4}
constexpr int kMcgMaxR = 6 * kMcgMaxB;    // columns per pass
constexpr int kMcgGroup = 32;             // cameras per workgroup of the camera-side kernels

// compact variable-camera index of each slot's column camera (-1: an empty slot)
struct McgPass { int cc[kMcgMaxB]; };

// State record of a pass (doubles): two scalars, then per-column arrays of
// kMcgMaxR entries.  The done / converged / broken flags only ever go from 0
// to 1 within a pass; rho has one slot per iteration parity (the workgroups
// of the launch that writes rho of iteration it + 1 still read that of it).
enum McgSlot {
  MS_ALLDONE = 0,   // every column of the pass is done: the kernels return at once
  MS_BADBLK,        // a preconditioner block was not positive definite (launch_mcg_blocks)
  MS_COL = 4,       // the per-column arrays start here
};
enum McgCol { MC_DONE = 0, MC_CONV, MC_BAD, MC_ITERS, MC_RHO0, MC_RHO1, MC_ALPHA, MC_RR, kMcgCols };
constexpr int kMcgState = MS_COL + kMcgCols * kMcgMaxR;
__host__ __device__ inline int mcg_slot(int arr, int col) { return MS_COL + arr * kMcgMaxR + col; }

// Scratch of the path.  Multi-vectors are camera-major [nvc][6][R], R = 6 B.
struct McgBufs {
  double* X; double* Rv; double* Z; double* Pv; double* Q;
  double* T;      // [G][nvc][6][R] camera-pass slices of one matvec
  double* Vp;     // [np][3][R] point products of one matvec
  double* part;   // [3][groups][R] per-workgroup partials: p.q | r.z | r.r
  double* st;     // [kMcgState]
};

// A_c = s Hcc s (undamped) into W.Adiag and M_c^-1 into W.Minv from W.Sd, as
// k_pcg_setup forms them; st[MS_BADBLK] = 1 for a block that is not PD
void launch_mcg_blocks(const DevProblem& P, const DevWork& W, bool schur_jacobi, double* st, hipStream_t s);
// x = 0, r = e, z = M e, p = z, rho = e.z of the pass's columns; the state record
void launch_mcg_init(const DevProblem& P, const DevWork& W, const McgBufs& b, int B, const McgPass& ps, double tau,
                     hipStream_t s);
// one implicit matvec of the multi-vector `vec` into b.T (point pass into b.Vp,
// camera pass); force: also when every column is done (the residual check)
void launch_mcg_matvec(const DevProblem& P, const DevWork& W, const McgBufs& b, int B, const double* vec, bool force,
                       hipStream_t s);
// mode 0: a full CG iteration from b.T = matvec(p); 1: up to the x update;
// 2: the residual reset from b.T = matvec(x), then the rest of the iteration;
// 3: partials of |e - S x|^2 from b.T = matvec(x) into b.part[2] (nothing else written)
void launch_mcg_update(const DevProblem& P, const DevWork& W, const McgBufs& b, int B, const McgPass& ps, int mode,
                       int it, double tau, int max_it, hipStream_t s);
// camera blocks of the requests ord[lo, hi) (pairs: compact indices, column camera .y in the pass)
void launch_mcg_gather_cam(const DevProblem& P, const DevWork& W, const McgBufs& b, int B, const McgPass& ps,
                           const int2* pairs, const int* ord, int lo, int hi, double* out, hipStream_t s);
// acc[q] (3 x 3) += V_p^(c(b)) W_b over the observations b of pts[q] whose camera is in the pass
void launch_mcg_gather_pt(const DevProblem& P, const DevWork& W, const McgBufs& b, int B, const McgPass& ps,
                          const int* pts, int npts, double* acc, hipStream_t s);
// out[q] = s_p L_p^-T (I + acc[q]) L_p^-1 s_p (zeros for a constant point)
void launch_mcg_pt_finish(const DevProblem& P, const DevWork& W, const int* pts, int npts, const double* acc,
                          double* out, hipStream_t s);

}  // namespace bahip
