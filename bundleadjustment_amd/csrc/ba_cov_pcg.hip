// ba_cov_pcg.hip — covariance blocks without the dense factor
// (ba_covariance_iterative): a few block columns of S_scaled^-1 by
// preconditioned conjugate gradients on the implicit reduced camera system of
// ba_pcg.hip, several right-hand sides per pass over the W records.
//
//   S_scaled X = E_v   (n x 6, E_v the unit columns of column camera v),
//   (S x)_c = A_c x_c - sum_{o in c} W_o v_{p(o)},   v_p = sum_{o in p} W_o^T x_{c(o)}
//
// A pass carries B column cameras (B in {1, 2, 4}), R = 6 B columns.  Multi-
// vectors are camera-major [nvc][6][R]: the six columns of one column camera
// (a "chunk") are 48 contiguous bytes of every row, and everything one camera
// contributes to a matvec is one contiguous 48 R byte run.  Point products are
// [np][3][R].
//
// A column's bits do not depend on its pass.  Every kernel splits its work
// into units that carry one chunk (or one column) and whose lane / thread
// decomposition does not involve B; B only enters strides and the unit count:
//   k_mcg_point   unit = (point, chunk), 16 lanes, the value-pair walk of point_wtx
//   k_mcg_cam     unit = (camera, slice, chunk), one wave, lane-strided
//   camera side   thread = (camera, column); a column's dot products are summed
//                 over fixed groups of kMcgGroup cameras in index order, then
//                 over the groups (lane-strided, wave tree)
// The units of one point / one camera slice sit next to each other in a wave /
// a workgroup, so their W loads are the same addresses in the same
// instruction (point pass) or hit the CU's cache (camera pass): HBM sees each
// W record once per pass whatever B is.  The per-chunk arithmetic is written
// once (mcg_*_acc below, fp contraction off, explicit fma), outside the
// templates, so that every instantiation rounds alike.
//
// No flags, tickets, spin waits, cooperative launches or floating-point
// atomics: every dependency is a launch boundary or a barrier inside one
// workgroup; every loop is bounded by the problem's sizes.
#include <algorithm>
#include <limits>

#include "ba_cov_pcg.h"
#include "ba_cov_point.h"
#include "ba_pcg_blocks.h"
#include "ba_reduce.h"

namespace bahip {

namespace {

__device__ __forceinline__ int mcg_find_slot(const McgPass& ps, int B, int v) {
  int slot = -1;
#pragma unroll
  for (int b = 0; b < kMcgMaxB; ++b)
    if (b < B && ps.cc[b] == v) slot = b;
  return slot;
}

// entry (camera v, row a) of column r = 6 slot + j of E: the unit vector of
// row j of the slot's column camera
__device__ __forceinline__ int mcg_cc(const McgPass& ps, int slot) {   // (selects: no indexed copy of the argument)
  return slot == 0 ? ps.cc[0] : (slot == 1 ? ps.cc[1] : (slot == 2 ? ps.cc[2] : ps.cc[3]));
}
__device__ __forceinline__ double mcg_e(const McgPass& ps, int v, int a, int r) {
  return (mcg_cc(ps, r / 6) == v && a == r % 6) ? 1.0 : 0.0;
}

// one value pair (values 2 f, 2 f + 1 of a W record: row i / 3, column i % 3)
// times the six columns of a chunk of x_c: s[k][j] += W[a][k] x[a][j]
__device__ __forceinline__ void mcg_point_acc(double t0, double t1, int f, const double* __restrict__ xc, int R,
                                              double (&s0)[6], double (&s1)[6], double (&s2)[6]) {
#pragma clang fp contract(off)
  const int i0 = 2 * f, i1 = i0 + 1;
  const double2* x0 = reinterpret_cast<const double2*>(xc + (size_t)(i0 / 3) * R);
  const double2* x1 = reinterpret_cast<const double2*>(xc + (size_t)(i1 / 3) * R);
  const int b0 = i0 % 3, b1 = i1 % 3;
#pragma unroll
  for (int h = 0; h < 3; ++h) {
    const double2 u = x0[h], w = x1[h];
    const double p0[2] = {t0 * u.x, t0 * u.y}, p1[2] = {t1 * w.x, t1 * w.y};
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int j = 2 * h + e;
      s0[j] += b0 == 0 ? p0[e] : (b1 == 0 ? p1[e] : 0.0);
      s1[j] += b0 == 1 ? p0[e] : (b1 == 1 ? p1[e] : 0.0);
      s2[j] += b0 == 2 ? p0[e] : (b1 == 2 ? p1[e] : 0.0);
    }
  }
}

// acc[a][j] += sum_k W[a][k] V[k][j]: one observation's W_o (6 x 3) times the
// chunk's six columns of its point's products (3 x 6)
__device__ __forceinline__ void mcg_cam_acc(const double (&w)[18], const double (&V)[3][6], double (&acc)[36]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int j = 0; j < 6; ++j)
      acc[a * 6 + j] = fma(w[a * 3 + 2], V[2][j], fma(w[a * 3 + 1], V[1][j], fma(w[a * 3], V[0][j], acc[a * 6 + j])));
}

// ---------------------------------------------------------------------------
// A_c = s Hcc s + D^2 and the preconditioner block M_c = A_c (JACOBI) or
// A_c + Sd_c (SCHUR_JACOBI) inverted, as k_pcg_setup forms them (thread per
// camera).  A block that is not positive definite raises st[MS_BADBLK] (a
// plain store of one value: no order among the writers matters).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mcg_blocks(DevProblem P, const double* __restrict__ Sd,
                                                    const double* __restrict__ Hcc,
                                                    const double* __restrict__ scale_c,
                                                    const double* __restrict__ diag_c, double radius, int schur_jacobi,
                                                    double* __restrict__ Adiag, double* __restrict__ Minv,
                                                    double* __restrict__ st) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= P.nvc) return;
  double s[6], D2[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    s[a] = scale_c[(size_t)v * 6 + a];
    const double D = sqrt(diag_c[(size_t)v * 6 + a] / radius);
    D2[a] = D * D;
  }
  double M[21];
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = 0; c <= a; ++c) {
      const int k = tri(a, c);
      double h = Hcc[(size_t)v * 21 + k] * s[a] * s[c];
      if (a == c) h += D2[a];
      Adiag[(size_t)v * 21 + k] = h;
      M[k] = schur_jacobi ? Sd[(size_t)v * 27 + k] + h : h;
    }
  if (!spd6_inverse(M, Minv + (size_t)v * 36)) st[MS_BADBLK] = 1.0;
}

// ---------------------------------------------------------------------------
// start of a pass: x = 0, r = e, z = M e, p = z (thread per (camera, column));
// workgroup 0 writes the state record: rho = e.z = (M_v^-1)_jj
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mcg_init(int nvc, int R, McgPass ps, double tau,
                                                  const double* __restrict__ Minv, double* __restrict__ X,
                                                  double* __restrict__ Rv, double* __restrict__ Z,
                                                  double* __restrict__ Pv, double* __restrict__ st) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < (size_t)nvc * R) {
    const int v = (int)(e / R), r = (int)(e % R);
    double rv[6], zv[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) rv[a] = mcg_e(ps, v, a, r);
    mat6_mul(Minv + (size_t)v * 36, rv, zv);
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const size_t i = ((size_t)v * 6 + a) * R + r;
      X[i] = 0.0; Rv[i] = rv[a]; Z[i] = zv[a]; Pv[i] = zv[a];
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    bool all = true;
    for (int r = 0; r < kMcgMaxR; ++r) {
      const int cc = r < R ? mcg_cc(ps, r / 6) : -1;
      double rho = 0.0;
      if (cc >= 0) {   // the same products as the threads' z and the dot product e.z
        double rv[6], zv[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) rv[a] = a == r % 6 ? 1.0 : 0.0;
        mat6_mul(Minv + (size_t)cc * 36, rv, zv);
#pragma unroll
        for (int a = 0; a < 6; ++a) rho += rv[a] * zv[a];
      }
      const bool conv = cc >= 0 && 1.0 <= tau;                   // |e|_2 = 1 already meets tau: x = 0
      const bool bad = cc >= 0 && !conv && !(rho > 0.0 && isfinite(rho));
      const bool done = cc < 0 || conv || bad;
      st[mcg_slot(MC_DONE, r)] = done ? 1.0 : 0.0;
      st[mcg_slot(MC_CONV, r)] = conv ? 1.0 : 0.0;
      st[mcg_slot(MC_BAD, r)] = bad ? 1.0 : 0.0;
      st[mcg_slot(MC_ITERS, r)] = 0.0;
      st[mcg_slot(MC_RHO0, r)] = rho;
      st[mcg_slot(MC_RHO1, r)] = rho;
      st[mcg_slot(MC_ALPHA, r)] = 0.0;
      st[mcg_slot(MC_RR, r)] = cc >= 0 ? 1.0 : 0.0;
      all = all && done;
    }
    st[MS_ALLDONE] = all ? 1.0 : 0.0;
  }
}

// ---------------------------------------------------------------------------
// matvec, point pass: V_p[:, r] = sum_{o in p} W_o^T X_{c(o)}[:, r].  Unit =
// (point, chunk): kPtLanes lanes walk the value pairs of the point's
// contiguous W records as point_wtx does (whole 256-B segments per wave
// instruction), each against the chunk's six columns of x_c (48 contiguous
// bytes per row).  The B units of a point are adjacent lane groups, so their
// W loads are one request.  Any number of observations per point (the walk is
// a loop); fixed cameras and fixed points carry W_o = 0.
// ---------------------------------------------------------------------------
template <int B>
__global__ __launch_bounds__(256) void k_mcg_point(DevProblem P, const double* __restrict__ Wm,
                                                   const double* __restrict__ xv, double* __restrict__ vp,
                                                   const double* __restrict__ st, int force) {
  if (!force && st[MS_ALLDONE] != 0.0) return;
  constexpr int R = 6 * B;
  constexpr int GPB = 256 / kPtLanes;   // units per workgroup
  const int gl = threadIdx.x & (kPtLanes - 1);
  const long long nunits = (long long)P.np * B;
  for (long long u = (long long)blockIdx.x * GPB + threadIdx.x / kPtLanes; u < nunits;
       u += (long long)gridDim.x * GPB) {
    const int p = (int)(u / B), ch = (int)(u % B);
    const int o0 = P.pt_off[p], o1 = P.pt_off[p + 1];
    const double* base = Wm + (size_t)o0 * 18;
    const int nch = 9 * (o1 - o0);
    double s0[6], s1[6], s2[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) s0[j] = s1[j] = s2[j] = 0.0;
    for (int c = gl; c < nch; c += kPtLanes) {
      double t0, t1;
      w_pair(base, c, t0, t1);
      const int k = c / 9;
      const int vc = max(P.obs_vc[o0 + k], 0);
      mcg_point_acc(t0, t1, c - 9 * k, xv + (size_t)vc * 6 * R + 6 * ch, R, s0, s1, s2);
    }
#pragma unroll
    for (int m = kPtLanes / 2; m > 0; m >>= 1)
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        s0[j] += __shfl_xor(s0[j], m, kPtLanes);
        s1[j] += __shfl_xor(s1[j], m, kPtLanes);
        s2[j] += __shfl_xor(s2[j], m, kPtLanes);
      }
    if (gl < 3) {   // lane k of the group stores row k
      double2* dst = reinterpret_cast<double2*>(vp + ((size_t)p * 3 + gl) * R + 6 * ch);
#pragma unroll
      for (int h = 0; h < 3; ++h) {
        const double a = gl == 0 ? s0[2 * h] : (gl == 1 ? s1[2 * h] : s2[2 * h]);
        const double b = gl == 0 ? s0[2 * h + 1] : (gl == 1 ? s1[2 * h + 1] : s2[2 * h + 1]);
        dst[h] = make_double2(a, b);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// matvec, camera pass: slice g of camera v, chunk ch: sum_{o in slice} W_o
// V_{p(o)}[:, chunk] (6 x 6) by one wave, lane l taking the observations
// l, l + 64, ... of the slice in order, then the wave's shuffle tree.  The
// slices are those of k_pcg_cam (G per camera); the B units of a slice are the
// waves of one workgroup (their W gathers hit the CU's cache).
// ---------------------------------------------------------------------------
template <int B>
__global__ __launch_bounds__(256) void k_mcg_cam(DevProblem P, int G, const double* __restrict__ Wm,
                                                 const double* __restrict__ vp, double* __restrict__ T,
                                                 const double* __restrict__ st, int force) {
  if (!force && st[MS_ALLDONE] != 0.0) return;
  constexpr int R = 6 * B;
  const int lane = threadIdx.x & 63;
  const long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (u >= (long long)P.nvc * G * B) return;   // (uniform in the wave; no barrier below)
  const int ch = (int)(u % B);
  const long long vg = u / B;
  const int g = (int)(vg % G), v = (int)(vg / G);
  const int a0 = P.cam_off[v], a1 = P.cam_off[v + 1];
  const int len = (a1 - a0 + G - 1) / G;
  const int i0 = min(a1, a0 + g * len), i1 = min(a1, i0 + len);
  double acc[36];
#pragma unroll
  for (int k = 0; k < 36; ++k) acc[k] = 0.0;
  for (int i = i0 + lane; i < i1; i += 64) {
    const int2 op = P.cam_op[i];   // fixed points: W_o = 0
    double w[18], V[3][6];
    load_w18(Wm, (size_t)op.x, w);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double2* src = reinterpret_cast<const double2*>(vp + ((size_t)op.y * 3 + k) * R + 6 * ch);
#pragma unroll
      for (int h = 0; h < 3; ++h) { const double2 t = src[h]; V[k][2 * h] = t.x; V[k][2 * h + 1] = t.y; }
    }
    mcg_cam_acc(w, V, acc);
  }
#pragma unroll
  for (int k = 0; k < 36; ++k) acc[k] = wave_sum(acc[k]);
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      double2* dst = reinterpret_cast<double2*>(T + (((size_t)g * P.nvc + v) * 6 + a) * R + 6 * ch);
#pragma unroll
      for (int h = 0; h < 3; ++h) dst[h] = make_double2(acc[a * 6 + 2 * h], acc[a * 6 + 2 * h + 1]);
    }
  }
}

// ---------------------------------------------------------------------------
// camera side.  Workgroup = kMcgGroup cameras x R columns, thread t = (camera
// t / R, column t % R): consecutive threads read consecutive columns of one
// row.  R is a launch argument: one instantiation serves every B.
// ---------------------------------------------------------------------------
// sum of a value over the group's cameras, per column, in camera order; the
// column's total goes to dst[column] (threads < R)
__device__ __forceinline__ void mcg_group_sum(double val, int R, double (*sh)[kMcgMaxR], double* __restrict__ dst) {
  const int t = threadIdx.x;
  sh[t / R][t % R] = val;
  __syncthreads();
  if (t < R) {
    double s = 0.0;
    for (int i = 0; i < kMcgGroup; ++i) s += sh[i][t];
    dst[t] = s;
  }
  __syncthreads();
}
// per-column sums of the ng per-group partials, to every thread through
// tot[column] (wave w takes the columns w, w + waves, ...: lane-strided over
// the groups, then the wave tree: a fixed order for a given ng)
__device__ __forceinline__ void mcg_fold(const double* __restrict__ part, int ng, int R, double* tot) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int r = w; r < R; r += nw) {
    double v = 0.0;
    for (int i = lane; i < ng; i += 64) v += part[(size_t)i * R + r];
    v = wave_sum(v);
    if (lane == 0) tot[r] = v;
  }
  __syncthreads();
}
// (S y)_v for column r from the camera's A block and the G slices of the matvec of y
__device__ __forceinline__ void mcg_schur_row(const double* __restrict__ Adiag, const double* __restrict__ T, int G,
                                              int nvc, int R, int v, int r, const double (&y)[6], double (&out)[6]) {
  sym6_mul(Adiag + (size_t)v * 21, y, out);
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    double t = T[((size_t)v * 6 + a) * R + r];
    for (int g = 1; g < G; ++g) t += T[(((size_t)g * nvc + v) * 6 + a) * R + r];
    out[a] -= t;
  }
}
__device__ __forceinline__ void mcg_load6(const double* __restrict__ p, size_t i0, int R, double (&v)[6]) {
#pragma unroll
  for (int a = 0; a < 6; ++a) v[a] = p[i0 + (size_t)a * R];
}
__device__ __forceinline__ void mcg_store6(double* __restrict__ p, size_t i0, int R, const double (&v)[6]) {
#pragma unroll
  for (int a = 0; a < 6; ++a) p[i0 + (size_t)a * R] = v[a];
}

// q = S p, per-group partials of p.q
__global__ __launch_bounds__(kMcgGroup * kMcgMaxR) void k_mcg_q(int nvc, int R, int G,
                                                                 const double* __restrict__ Adiag,
                                                                 const double* __restrict__ Pv, double* __restrict__ Q,
                                                                 const double* __restrict__ T,
                                                                 double* __restrict__ part,
                                                                 const double* __restrict__ st) {
  if (st[MS_ALLDONE] != 0.0) return;
  __shared__ double sh[kMcgGroup][kMcgMaxR];
  const int t = threadIdx.x, r = t % R, v = blockIdx.x * kMcgGroup + t / R;
  double d = 0.0;
  if (v < nvc) {
    const size_t i0 = (size_t)v * 6 * R + r;
    double pv[6], qv[6];
    mcg_load6(Pv, i0, R, pv);
    mcg_schur_row(Adiag, T, G, nvc, R, v, r, pv, qv);
    mcg_store6(Q, i0, R, qv);
#pragma unroll
    for (int a = 0; a < 6; ++a) d += pv[a] * qv[a];
  }
  mcg_group_sum(d, R, sh, part + (size_t)blockIdx.x * R);
}

// mode 0: alpha = rho / p.q, x += alpha p, r -= alpha q, z = M r, partials of
// r.z and r.r.  mode 1: up to the x update.  mode 2: r = e - S x from the
// matvec of x, z = M r, the partials.  mode 3: the partials of |e - S x|^2
// alone, for every column, nothing else written.  A column that is done is
// never touched; p.q <= 0 or a non-finite step breaks a column (MC_BAD).
__global__ __launch_bounds__(kMcgGroup * kMcgMaxR) void k_mcg_xr(int nvc, int R, int G, McgPass ps, int mode, int it,
                                                                  const double* __restrict__ Adiag,
                                                                  const double* __restrict__ Minv,
                                                                  double* __restrict__ X, double* __restrict__ Rv,
                                                                  double* __restrict__ Z, const double* __restrict__ Pv,
                                                                  const double* __restrict__ Q,
                                                                  const double* __restrict__ T, double* __restrict__ part,
                                                                  double* __restrict__ st) {
  if (mode != 3 && st[MS_ALLDONE] != 0.0) return;
  __shared__ double sh[kMcgGroup][kMcgMaxR];
  __shared__ double tot[kMcgMaxR];
  const int ng = gridDim.x;
  const int t = threadIdx.x, r = t % R, v = blockIdx.x * kMcgGroup + t / R;
  const bool on = v < nvc;
  const size_t i0 = (size_t)(on ? v : 0) * 6 * R + r;
  double* part_rz = part + (size_t)ng * R;
  double* part_rr = part + 2 * (size_t)ng * R;
  if (mode == 3) {
    double d = 0.0;
    if (on) {
      double xv[6], sx[6];
      mcg_load6(X, i0, R, xv);
      mcg_schur_row(Adiag, T, G, nvc, R, v, r, xv, sx);
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        const double rt = mcg_e(ps, v, a, r) - sx[a];
        d += rt * rt;
      }
    }
    mcg_group_sum(d, R, sh, part_rr + (size_t)blockIdx.x * R);
    return;
  }
  // (the lead workgroup may raise MC_BAD of a column in this launch: a
  // workgroup that reads it early skips what it would have skipped anyway)
  bool act = st[mcg_slot(MC_DONE, r)] == 0.0 && st[mcg_slot(MC_BAD, r)] == 0.0;
  double rv[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (mode != 2) {
    mcg_fold(part, ng, R, tot);
    const double pq = tot[r], rho = st[mcg_slot(MC_RHO0 + (it & 1), r)];
    const double alpha = rho / pq;
    const bool broken = !(pq > 0.0) || !isfinite(pq) || !isfinite(alpha);
    if (blockIdx.x == 0 && t < R && act) {   // (t < R: this thread's column is t)
      if (broken) st[mcg_slot(MC_BAD, r)] = 1.0;
      else st[mcg_slot(MC_ALPHA, r)] = alpha;
    }
    act = act && !broken;
    if (act && on) {
      double xv[6], pv[6];
      mcg_load6(X, i0, R, xv);
      mcg_load6(Pv, i0, R, pv);
#pragma unroll
      for (int a = 0; a < 6; ++a) xv[a] = xv[a] + alpha * pv[a];
      mcg_store6(X, i0, R, xv);
    }
    if (mode == 1) return;
    if (act && on) {
      double qv[6];
      mcg_load6(Rv, i0, R, rv);
      mcg_load6(Q, i0, R, qv);
#pragma unroll
      for (int a = 0; a < 6; ++a) rv[a] = rv[a] - alpha * qv[a];
    }
  } else if (act && on) {
    double xv[6], sx[6];
    mcg_load6(X, i0, R, xv);
    mcg_schur_row(Adiag, T, G, nvc, R, v, r, xv, sx);
#pragma unroll
    for (int a = 0; a < 6; ++a) rv[a] = mcg_e(ps, v, a, r) - sx[a];
  }
  double drz = 0.0, drr = 0.0;
  if (act && on) {
    double zv[6];
    mcg_store6(Rv, i0, R, rv);
    mat6_mul(Minv + (size_t)v * 36, rv, zv);
    mcg_store6(Z, i0, R, zv);
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      drz += rv[a] * zv[a];
      drr += rv[a] * rv[a];
    }
  }
  mcg_group_sum(drz, R, sh, part_rz + (size_t)blockIdx.x * R);
  mcg_group_sum(drr, R, sh, part_rr + (size_t)blockIdx.x * R);
}

// end of iteration it: a column stops when |r|_2 <= tau (converged), at
// max_it, or broken (MC_BAD, or r.z not positive and finite); otherwise
// beta = rho' / rho, p = z + beta p.  Every workgroup folds the partials
// itself and reaches the same decisions; workgroup 0 records them (rho' into
// the other parity's slot: workgroups of this launch still read rho).
__global__ __launch_bounds__(kMcgGroup * kMcgMaxR) void k_mcg_p(int nvc, int R, int it, double tau, int max_it,
                                                                 const double* __restrict__ Z, double* __restrict__ Pv,
                                                                 const double* __restrict__ part,
                                                                 double* __restrict__ st) {
  if (st[MS_ALLDONE] != 0.0) return;
  __shared__ double trz[kMcgMaxR], trr[kMcgMaxR];
  __shared__ int sdone[kMcgMaxR];
  const int ng = gridDim.x;
  const int t = threadIdx.x, r = t % R, v = blockIdx.x * kMcgGroup + t / R;
  mcg_fold(part + (size_t)ng * R, ng, R, trz);
  mcg_fold(part + 2 * (size_t)ng * R, ng, R, trr);
  // (MC_DONE may be raised by workgroup 0 in this launch, for a column every
  // workgroup finds done anyway; MC_BAD was written by an earlier launch)
  const bool was_done = st[mcg_slot(MC_DONE, r)] != 0.0;
  const bool bad = st[mcg_slot(MC_BAD, r)] != 0.0;
  const double rho = st[mcg_slot(MC_RHO0 + (it & 1), r)];
  const double rz = trz[r], rr = trr[r];
  const bool conv = !bad && sqrt(rr) <= tau;
  const bool stop = bad || conv || it >= max_it;
  const double beta = rz / rho;
  const bool brk = !stop && (!(rz > 0.0) || !isfinite(rz) || !isfinite(beta));
  const bool done = was_done || stop || brk;
  if (!done && v < nvc) {
    const size_t i0 = (size_t)v * 6 * R + r;
    double zv[6], pv[6];
    mcg_load6(Z, i0, R, zv);
    mcg_load6(Pv, i0, R, pv);
#pragma unroll
    for (int a = 0; a < 6; ++a) pv[a] = zv[a] + beta * pv[a];
    mcg_store6(Pv, i0, R, pv);
  }
  if (blockIdx.x != 0) return;
  if (t < R) {
    if (!was_done) {
      st[mcg_slot(MC_ITERS, r)] = it;
      if (!bad) st[mcg_slot(MC_RR, r)] = rr;
      if (conv) st[mcg_slot(MC_CONV, r)] = 1.0;
      if (brk) st[mcg_slot(MC_BAD, r)] = 1.0;
      if (done) st[mcg_slot(MC_DONE, r)] = 1.0;
      else st[mcg_slot(MC_RHO0 + ((it + 1) & 1), r)] = rz;
    }
    sdone[r] = done ? 1 : 0;
  }
  __syncthreads();
  if (t == 0) {
    bool all = true;
    for (int c = 0; c < R; ++c) all = all && sdone[c] != 0;
    if (all) st[MS_ALLDONE] = 1.0;
  }
}

// ---------------------------------------------------------------------------
// gathers
// ---------------------------------------------------------------------------
// Cov(cam i, cam v) = s_i X[i, columns of v] s_v for the requests ord[lo, hi)
__global__ __launch_bounds__(256) void k_mcg_gather_cam(int R, int B, McgPass ps, const double* __restrict__ X,
                                                        const double* __restrict__ scale_c,
                                                        const int2* __restrict__ pairs, const int* __restrict__ ord,
                                                        int lo, int hi, double* __restrict__ out) {
  const size_t total = (size_t)(hi - lo) * 36;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int q = ord[lo + (int)(e / 36)], t = (int)(e % 36), a = t / 6, j = t % 6;
    const int2 pr = pairs[q];
    const int slot = mcg_find_slot(ps, B, pr.y);
    if (slot < 0 || pr.x < 0) continue;
    out[(size_t)q * 36 + t] = scale_c[(size_t)pr.x * 6 + a] * X[((size_t)pr.x * 6 + a) * R + 6 * slot + j] *
                              scale_c[(size_t)pr.y * 6 + j];
  }
}

// acc[q] += V_p^(c(b)) W_b (3 x 3) for the observations b of point pts[q] by
// the pass's column cameras, b in observation order, one term at a time
// (thread per request): with the passes in increasing column camera the terms
// of a point add up in observation order whatever the batching.  V_p^(v) are
// the columns of v in the point products of the matvec of the final X.
__global__ __launch_bounds__(64) void k_mcg_gather_pt(DevProblem P, int R, int B, McgPass ps,
                                                      const double* __restrict__ Wm, const double* __restrict__ vp,
                                                      const int* __restrict__ pts, int npts, double* __restrict__ acc) {
#pragma clang fp contract(off)
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= npts) return;
  const int p = pts[q];
  if (!P.pt_var[p]) return;
  double t[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) t[k] = acc[(size_t)q * 9 + k];
  for (int o = P.pt_off[p]; o < P.pt_off[p + 1]; ++o) {
    const int slot = mcg_find_slot(ps, B, P.obs_vc[o]);   // (a constant camera: -1, no slot)
    if (slot < 0 || P.obs_vc[o] < 0) continue;
    double w[18];
    load_w18(Wm, (size_t)o, w);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double* V = vp + ((size_t)p * 3 + k) * R + 6 * slot;
#pragma unroll
      for (int l = 0; l < 3; ++l) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) s = fma(V[j], w[j * 3 + l], s);
        t[k * 3 + l] += s;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[(size_t)q * 9 + k] = t[k];
}

// Sigma_pp = s_p L_p^-T (I + acc) L_p^-1 s_p (cov_point_finish); zeros for a constant point
__global__ __launch_bounds__(64) void k_mcg_pt_finish(DevProblem P, const double* __restrict__ scale_p,
                                                      const double* __restrict__ Linv, const int* __restrict__ pts,
                                                      int npts, const double* __restrict__ acc,
                                                      double* __restrict__ out) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= npts) return;
  const int p = pts[q];
  double r[9];
  if (P.pt_var[p]) {
    double t[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) t[k] = acc[(size_t)q * 9 + k];
    CovPt cp;
    cp.load(Linv, scale_p, p, (size_t)P.np);
    cov_point_finish(t, true, cp, cp, r);
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = 0.0;
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) out[(size_t)q * 9 + k] = r[k];
}

int mcg_groups(int nvc) { return (nvc + kMcgGroup - 1) / kMcgGroup; }

}  // namespace

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
void launch_mcg_blocks(const DevProblem& P, const DevWork& W, bool schur_jacobi, double* st, hipStream_t s) {
  if (P.nvc == 0) return;
  hipLaunchKernelGGL(k_mcg_blocks, dim3((P.nvc + 255) / 256), dim3(256), 0, s, P, (const double*)W.Sd,
                     (const double*)W.Hcc, (const double*)W.scale_c, (const double*)W.diag_c,
                     std::numeric_limits<double>::infinity(), schur_jacobi ? 1 : 0, W.Adiag, W.Minv, st);
}

void launch_mcg_init(const DevProblem& P, const DevWork& W, const McgBufs& b, int B, const McgPass& ps, double tau,
                     hipStream_t s) {
  const int R = 6 * B;
  const size_t n = (size_t)P.nvc * R;
  hipLaunchKernelGGL(k_mcg_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, P.nvc, R, ps, tau,
                     (const double*)W.Minv, b.X, b.Rv, b.Z, b.Pv, b.st);
}

void launch_mcg_matvec(const DevProblem& P, const DevWork& W, const McgBufs& b, int B, const double* vec, bool force,
                       hipStream_t s) {
  const int f = force ? 1 : 0;
  const int G = W.pcg_G;
  const long long pu = (long long)P.np * B, cu = (long long)P.nvc * G * B;
  const int gp = (int)std::max<long long>(1, std::min<long long>((pu + 15) / 16, 1 << 16));
  const unsigned gc = (unsigned)((cu + 3) / 4);
#define BA_MCG_MATVEC(B_)                                                                                       \
  do {                                                                                                          \
    if (pu > 0)                                                                                                 \
      hipLaunchKernelGGL(k_mcg_point<B_>, dim3(gp), dim3(256), 0, s, P, (const double*)W.W, vec, b.Vp,          \
                         (const double*)b.st, f);                                                               \
    hipLaunchKernelGGL(k_mcg_cam<B_>, dim3(gc), dim3(256), 0, s, P, G, (const double*)W.W, (const double*)b.Vp, \
                       b.T, (const double*)b.st, f);                                                            \
  } while (0)
  if (B == 1) BA_MCG_MATVEC(1);
  else if (B == 2) BA_MCG_MATVEC(2);
  else BA_MCG_MATVEC(4);
#undef BA_MCG_MATVEC
}

void launch_mcg_update(const DevProblem& P, const DevWork& W, const McgBufs& b, int B, const McgPass& ps, int mode,
                       int it, double tau, int max_it, hipStream_t s) {
  const int R = 6 * B, G = W.pcg_G, ng = mcg_groups(P.nvc);
  const dim3 grid(ng), block(kMcgGroup * R);
  if (mode == 0 || mode == 1)
    hipLaunchKernelGGL(k_mcg_q, grid, block, 0, s, P.nvc, R, G, (const double*)W.Adiag, (const double*)b.Pv, b.Q,
                       (const double*)b.T, b.part, (const double*)b.st);
  hipLaunchKernelGGL(k_mcg_xr, grid, block, 0, s, P.nvc, R, G, ps, mode, it, (const double*)W.Adiag,
                     (const double*)W.Minv, b.X, b.Rv, b.Z, (const double*)b.Pv, (const double*)b.Q,
                     (const double*)b.T, b.part, b.st);
  if (mode == 0 || mode == 2)
    hipLaunchKernelGGL(k_mcg_p, grid, block, 0, s, P.nvc, R, it, tau, max_it, (const double*)b.Z, b.Pv,
                       (const double*)b.part, b.st);
}

void launch_mcg_gather_cam(const DevProblem& P, const DevWork& W, const McgBufs& b, int B, const McgPass& ps,
                           const int2* pairs, const int* ord, int lo, int hi, double* out, hipStream_t s) {
  if (hi <= lo) return;
  hipLaunchKernelGGL(k_mcg_gather_cam, dim3(grid_for(std::min(hi - lo, 1 << 24) * 36)), dim3(256), 0, s, 6 * B, B, ps,
                     (const double*)b.X, (const double*)W.scale_c, pairs, ord, lo, hi, out);
}

void launch_mcg_gather_pt(const DevProblem& P, const DevWork& W, const McgBufs& b, int B, const McgPass& ps,
                          const int* pts, int npts, double* acc, hipStream_t s) {
  if (npts == 0) return;
  hipLaunchKernelGGL(k_mcg_gather_pt, dim3((npts + 63) / 64), dim3(64), 0, s, P, 6 * B, B, ps, (const double*)W.W,
                     (const double*)b.Vp, pts, npts, acc);
}

void launch_mcg_pt_finish(const DevProblem& P, const DevWork& W, const int* pts, int npts, const double* acc,
                          double* out, hipStream_t s) {
  if (npts == 0) return;
  hipLaunchKernelGGL(k_mcg_pt_finish, dim3((npts + 63) / 64), dim3(64), 0, s, P, (const double*)W.scale_p,
                     (const double*)W.Linv, pts, npts, acc, out);
}

}  // namespace bahip
