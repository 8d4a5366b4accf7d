// ba_window.hip — batched small-window bundle adjustment (gfx950, wave64):
// many independent problems with variable cameras AND variable points, the
// whole DENSE_SCHUR Levenberg-Marquardt loop of each problem in ONE launch.
//
// Replaces, per window, the ceres::Problem + ceres::Solve of the reference's
// local BA (LocalBAOptimizerAngles, Optimizer.cpp:500-698) and of its small
// global BAs: at most kWinMaxCams variable cameras, any number of constant
// observers, 10^2-10^4 observations.  At these sizes the general path
// (solve(), ba_solver.hip) is launch and round-trip latency; here a problem
// costs one launch.
//
// One workgroup per problem, grid = number of problems.  NO dependency
// between workgroups: no flags, tickets, spin waits or cooperative launch;
// every hand-off is a workgroup barrier and the loop is bounded by
// max_num_iterations, so the kernel cannot hang whatever is co-resident.
//
// Uniform control flow: every LM decision (valid / accept / reject, each
// termination test, the Cholesky's success) is computed by EVERY thread from
// the same LDS values with the same operations, so all waves take the same
// branches and reach the same barriers.  The helpers below never return early.
//
// Determinism: every reduction has a fixed order that depends on the problem
// alone (the number of working waves is a function of its camera count), no
// floating-point atomics: a problem's result is bitwise independent of its
// place in the batch and of its neighbours.
//
// Per LM iteration (x: current point, x': candidate; two copies of the
// linearisation state, flipped when a step is accepted):
//   elim    thread per point: A = s Hpp s + D^2 = L L^T, L^-1, u = L^-1 s g_p,
//           W = E L^-T per (point, camera) group          -> global scratch
//   schur   wave w walks its points in order and subtracts W_i W_j^T from its
//           PRIVATE packed copy of S in LDS (64 lanes share one point's
//           update: no two lanes touch one entry), rhs row alike
//   fold    copies summed in wave order, + s Hcc s + D^2, + s g_c
//   factor  in-LDS right-looking Cholesky, the rhs as row n (forward
//           substitution folded in); back substitution in wave 0
//   point   thread per point, ONE pass: back substitution of the point,
//           model cost change from J(x), candidate cost at x', and the
//           linearisation at x' (speculative, as k_pose_batch: adopted when
//           the step is accepted)
//   cams    wave per camera: Hcc, g_c at x' from the new records
//   decide  one fixed-order block reduction, then the host loop of solve()
//           restated per thread
// The per-observation arithmetic is lin_obs / project_value (ba_lin.h), the
// functions of the general path.
#include <hip/hip_runtime.h>

#include "ba_kernels.h"
#include "ba_device.h"
#include "ba_lin.h"
#include "../../include/ba_hip.h"

namespace bahip {

constexpr int kWinThreads = 512;
constexpr int kWinWaves = kWinThreads / 64;
// up to this many variable cameras all 8 waves work (8 private copies of S
// fit the LDS), beyond it 4
constexpr int kWinWideCams = 11;
constexpr int kWinRed = 12;   // block-reduction slots (11 used)
enum WinSlot { WS_COST = 0, WS_BAD, WS_GN2, WS_XN2, WS_MNEG, WS_CCOST, WS_CBAD, WS_STEP2, WS_STEP_BAD, WS_ELIM_BAD,
               WS_GMAX, kWinSlots };
static_assert(kWinSlots <= kWinRed, "reduction slots");
static_assert(kWinMaxCams == BA_WINDOW_MAX_CAMS, "camera cap");
static_assert(kWinTbl == kTblRec && kWinVRec == kRecL && kWinJR == kJR, "scratch record sizes");
constexpr int kWinN = 6 * kWinMaxCams;
// fixed LDS: reduction partials, s_c, D_c^2 source, y / delta_c, the pivots,
// the variable cameras at x and x', per-wave slot lists
constexpr size_t kWinFixedDoubles = kWinWaves * kWinRed + 6 * kWinN;
constexpr size_t kWinFixedBytes = kWinFixedDoubles * sizeof(double) + kWinWaves * 2 * kWinMaxCams * sizeof(int);
static_assert(kWinFixedBytes % 16 == 0, "LDS carve alignment");

__host__ __device__ inline int win_waves(int nvc) { return nvc <= kWinWideCams ? kWinWaves : 4; }
__host__ __device__ inline int win_packed(int n) { return n * (n + 1) / 2 + n; }   // lower triangle + rhs row

size_t window_lds_bytes(int nvc) {
  return kWinFixedBytes + sizeof(double) * (size_t)win_waves(nvc) * win_packed(6 * nvc);
}

__device__ inline double wave_sum64(double v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ inline double wave_max64(double v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

__global__ __launch_bounds__(kWinThreads) void k_window_batch(WinArgs A, PoseOpts o) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const WinProb pr = A.prob[blockIdx.x];
  const int nc = pr.nc, np = pr.np, nvc = pr.nvc, n = 6 * nvc;
  const int NW = win_waves(nvc), NT = NW * 64;
  const bool act = wave < NW;           // waves beyond NW only keep the barriers
  const int PS = win_packed(n), rhs0 = n * (n + 1) / 2;

  // ---- LDS carve
  double* red = reinterpret_cast<double*>(smem);   // [kWinWaves][kWinRed]
  double* sc = red + kWinWaves * kWinRed;          // [n] Jacobi scale of the camera columns
  double* dg = sc + kWinN;                         // [n] clamped LM diagonal (before / radius)
  double* yv = dg + kWinN;                         // [n] reduced solution y
  double* Ld = yv + kWinN;                         // [n] Cholesky pivots, then delta_c
  double* xcam = Ld + kWinN;                       // [2][n] variable cameras at x / x'
  int* wl = reinterpret_cast<int*>(xcam + 2 * kWinN);   // [kWinWaves][2][kWinMaxCams] a point's groups: observation, camera
  double* Sw = reinterpret_cast<double*>(smem + kWinFixedBytes);   // [NW][PS]
  double* S0 = Sw;
  double* myS = Sw + (size_t)(act ? wave : 0) * PS;
  int* mywl = wl + wave * 2 * kWinMaxCams;

  // ---- this problem's slices
  const double* cams_in = A.cams_in + 6 * (size_t)pr.cam0;
  const double* pts_in = A.pts_in + 3 * (size_t)pr.pt0;
  const float* Kf = A.K + 9 * (size_t)pr.cam0;
  const float* extr = A.extr + 16 * (size_t)pr.cam0;
  const int* cam_vc = A.cam_vc + pr.cam0;
  const uint8_t* pt_var = A.pt_var + pr.pt0;
  const int* poff = A.pt_off + pr.poff0;
  const int* obs_cam = A.obs_cam + pr.obs0;
  const int* obs_slot = A.obs_slot + pr.obs0;
  const float2* uvs = A.uv + pr.obs0;
  const int* coff = A.cam_off + pr.coff0;
  const int* cobs = A.cam_obs + pr.vobs0;
  double* ptsb[2] = {A.pts + 3 * (size_t)pr.pt0, A.pts + 3 * (A.NP + pr.pt0)};
  double* ctab[2] = {A.ctab + (size_t)kTblRec * pr.cam0, A.ctab + (size_t)kTblRec * (A.NC + pr.cam0)};
  double* vrec = A.vrec + (size_t)kRecL * pr.cam0;
  double* JRb[2] = {A.JR + (size_t)kJR * pr.obs0, A.JR + (size_t)kJR * (A.NO + pr.obs0)};
  double* Hpb[2] = {A.Hp + 9 * (size_t)pr.pt0, A.Hp + 9 * (A.NP + pr.pt0)};
  double* scale_p = A.scale_p + 3 * (size_t)pr.pt0;
  double* prec = A.prec + 9 * (size_t)pr.pt0;
  double* Wb = A.Wb + 18 * (size_t)pr.obs0;
  double* hcb[2] = {A.hc + 27 * (size_t)pr.vc0, A.hc + 27 * (A.NV + pr.vc0)};
  ba_iteration* logp = static_cast<ba_iteration*>(A.log) + (size_t)blockIdx.x * A.log_cap;

  DevProblem P{};
  P.huber_a = A.huber_a;
  P.huber_b = A.huber_a * A.huber_a;

  // ---- setup: parameters into the scratch, the constant cameras' tables
  for (int i = tid; i < 3 * np; i += kWinThreads) { const double v = pts_in[i]; ptsb[0][i] = v; ptsb[1][i] = v; }
  for (int c = tid; c < nc; c += kWinThreads) {
    const int v = cam_vc[c];
    if (v >= 0) {
#pragma unroll
      for (int a = 0; a < 6; ++a) { xcam[6 * v + a] = cams_in[6 * c + a]; xcam[kWinN + 6 * v + a] = cams_in[6 * c + a]; }
    }
  }
  for (int i = tid; i < nc * kTblRec; i += kWinThreads) {
    const int c = i / kTblRec, l = i - c * kTblRec;
    if (cam_vc[c] < 0) {   // PointOnlyReprojectionError: K E(0:3, :), E(3, :) (k_cam_prep's constant-camera record)
      const float* E = extr + 16 * c;
      const float* Kc = Kf + 9 * c;
      double v = 0.0;
      if (l < 12) {
        const int col = l / 3, row = l % 3;
        v = (double)Kc[row] * (double)E[col * 4] + (double)Kc[3 + row] * (double)E[col * 4 + 1] +
            (double)Kc[6 + row] * (double)E[col * 4 + 2];
      } else if (l < 16) {
        v = (double)E[(l - 12) * 4 + 3];
      }
      ctab[0][i] = v;
      ctab[1][i] = v;
    }
  }
  for (int i = tid; i < nc * kRecL; i += kWinThreads) {
    const int c = i / kRecL, e = i - c * kRecL;
    if (cam_vc[c] < 0) {
      double v = 0.0;
      if (e < 16) v = (double)extr[16 * c + e];
      else if (e >= kRecK) v = (double)Kf[9 * c + e - kRecK];
      vrec[i] = v;
    }
  }
  __syncthreads();

  // K-folded tables of the variable cameras at xcam[b] (and, cand: their
  // value-only records for the candidate cost); one wave per camera, every
  // lane evaluates the Rodrigues duals (k_cam_prep)
  auto cam_tables = [&](int b, bool cand) {
    if (act) {
      for (int c = wave; c < nc; c += NW) {
        const int v = cam_vc[c];
        if (v < 0) continue;
        double x[6], Kd[9];
#pragma unroll
        for (int a = 0; a < 6; ++a) x[a] = xcam[b * kWinN + 6 * v + a];
#pragma unroll
        for (int k = 0; k < 9; ++k) Kd[k] = (double)Kf[9 * c + k];
        D3 R[9];
        angle_axis_to_R_d3(x, R);
        double* tb = ctab[b] + (size_t)c * kTblRec;
        if (lane < kLin) tb[lane] = cam_rec_entry(kRecL + lane, x, x + 3, Kd, R, nullptr, true);
        if (lane == kLin) tb[kLin] = 1.0;
        if (lane == kLin + 1) tb[kLin + 1] = 0.0;
        if (cand) {
          double R0[9];
          angle_axis_to_R(x, R0);
          if (lane < kRecL) vrec[(size_t)c * kRecL + lane] = cam_rec_entry(lane, x, x + 3, Kd, nullptr, R0, false);
        }
      }
    }
  };

  // thread-local partials of the next block reduction
  double acc[kWinSlots];
  auto acc_clear = [&]() {
#pragma unroll
    for (int k = 0; k < kWinSlots; ++k) acc[k] = 0.0;
  };
  // fixed-order block reduction: wave butterflies, then the waves' partials
  // in wave order; every thread ends with the same totals.  Two barriers.
  auto reduce = [&](double (&tot)[kWinSlots]) {
#pragma unroll
    for (int k = 0; k < kWinSlots; ++k) {
      const double v = k == WS_GMAX ? wave_max64(acc[k]) : wave_sum64(acc[k]);
      if (lane == 0) red[wave * kWinRed + k] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kWinSlots; ++k) {
      double v = red[k];
      for (int w = 1; w < NW; ++w) v = k == WS_GMAX ? fmax(v, red[w * kWinRed + k]) : v + red[w * kWinRed + k];
      tot[k] = v;
    }
    __syncthreads();
  };

  // One pass over the points (thread per point).  step: back substitution
  // with y (yv; delta_c in Ld), model cost change from JR[cur], candidate cost at
  // x' = pts[nxt]; always: the linearisation at pts[nxt] / ctab[nxt] into
  // JR[nxt], Hp[nxt] and the points' share of cost, gradient and x norms.
  auto point_pass = [&](int cur, int nxt, bool step, bool first) {
    if (act) {
      for (int p = tid; p < np; p += NT) {
        const int a0 = poff[p], a1 = poff[p + 1];
        if (a0 == a1) continue;   // no residual: not part of the problem
        const bool pv = pt_var[p] != 0;
        const double X[3] = {ptsb[cur][3 * p], ptsb[cur][3 * p + 1], ptsb[cur][3 * p + 2]};
        double Xn[3] = {X[0], X[1], X[2]}, dp[3] = {0.0, 0.0, 0.0};
        if (step && pv) {
          const double* q = prec + 9 * (size_t)p;
          double w0 = q[6], w1 = q[7], w2 = q[8];
          for (int ob = a0; ob < a1; ++ob) {
            const int v = obs_slot[ob];
            if (v < 0) continue;
            const double* Wo = Wb + 18 * (size_t)ob;
            const double* y = yv + 6 * v;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
              w0 -= Wo[3 * a] * y[a];
              w1 -= Wo[3 * a + 1] * y[a];
              w2 -= Wo[3 * a + 2] * y[a];
            }
          }
          const double yp[3] = {q[0] * w0 + q[1] * w1 + q[3] * w2, q[2] * w1 + q[4] * w2, q[5] * w2};
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            dp[k] = (-yp[k]) * scale_p[3 * (size_t)p + k];
            Xn[k] = X[k] + dp[k];
            const double e = X[k] - Xn[k];
            acc[WS_STEP2] += e * e;
            if (!isfinite(dp[k])) acc[WS_STEP_BAD] += 1.0;
            ptsb[nxt][3 * p + k] = Xn[k];
          }
        }
        double H[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
        for (int ob = a0; ob < a1; ++ob) {
          const int c = obs_cam[ob], v = cam_vc[c];
          const bool cv = v >= 0;
          const float2 uv = uvs[ob];
          if (step) {
            const double* jr = JRb[cur] + (size_t)kJR * ob;
            double jd0 = 0.0, jd1 = 0.0;
            if (cv) {
              const double* dl = Ld + 6 * v;   // delta_c
#pragma unroll
              for (int a = 0; a < 6; ++a) { jd0 += jr[a] * dl[a]; jd1 += jr[6 + a] * dl[a]; }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) { jd0 += jr[12 + k] * dp[k]; jd1 += jr[15 + k] * dp[k]; }
            acc[WS_MNEG] += jd0 * (jr[18] + jd0 / 2.0) + jd1 * (jr[19] + jd1 / 2.0);
            double rc[2], s;
            project_value(vrec + (size_t)kRecL * c, cv, Xn[0], Xn[1], Xn[2], uv, rc);
            acc[WS_CCOST] += 0.5 * huber(rc[0] * rc[0] + rc[1] * rc[1], P.huber_a, P.huber_b, &s);
            if (!isfinite(rc[0]) || !isfinite(rc[1])) acc[WS_CBAD] += 1.0;
          }
          double out[kJR];
          bool fin;
          const double rho = lin_obs(P, CamLds{ctab[nxt] + (size_t)kTblRec * c, Kf + 9 * c}, cv, pv, Xn[0], Xn[1], Xn[2],
                                     uv, out, fin);
          acc[WS_COST] += 0.5 * rho;
          acc[WS_BAD] += fin ? 0.0 : 1.0;
          double2* dst = reinterpret_cast<double2*>(JRb[nxt] + (size_t)kJR * ob);
#pragma unroll
          for (int k = 0; k < kJR / 2; ++k) dst[k] = make_double2(out[2 * k], out[2 * k + 1]);
          if (pv) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
              const double* j = out + 12 + 3 * r;
              H[0] += j[0] * j[0]; H[1] += j[0] * j[1]; H[2] += j[0] * j[2];
              H[3] += j[1] * j[1]; H[4] += j[1] * j[2]; H[5] += j[2] * j[2];
#pragma unroll
              for (int k = 0; k < 3; ++k) g[k] += j[k] * out[18 + r];
            }
          }
        }
        if (pv) {
          double* hp = Hpb[nxt] + 9 * (size_t)p;
#pragma unroll
          for (int k = 0; k < 6; ++k) hp[k] = H[k];
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            hp[6 + k] = g[k];
            const double d = Xn[k] - (Xn[k] + (-g[k]));
            acc[WS_GMAX] = fmax(acc[WS_GMAX], fabs(d));
            acc[WS_GN2] += d * d;
            acc[WS_XN2] += Xn[k] * Xn[k];
          }
          if (first) {
            scale_p[3 * (size_t)p] = o.jacobi ? 1.0 / (1.0 + sqrt(H[0])) : 1.0;
            scale_p[3 * (size_t)p + 1] = o.jacobi ? 1.0 / (1.0 + sqrt(H[3])) : 1.0;
            scale_p[3 * (size_t)p + 2] = o.jacobi ? 1.0 / (1.0 + sqrt(H[5])) : 1.0;
          }
        }
      }
    }
  };

  // Hcc (lower 21, row-major) and g_c of every variable camera from JR[b]:
  // one wave per camera, lanes over its observations, butterfly totals
  auto cam_pass = [&](int b) {
    if (act) {
      for (int v = wave; v < nvc; v += NW) {
        double h[27];
#pragma unroll
        for (int k = 0; k < 27; ++k) h[k] = 0.0;
        for (int i = coff[v] + lane; i < coff[v + 1]; i += 64) {
          const double* jr = JRb[b] + (size_t)kJR * cobs[i];
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            const double* j = jr + 6 * r;
            int t = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
              for (int c2 = 0; c2 <= a; ++c2) h[t++] += j[a] * j[c2];
#pragma unroll
            for (int a = 0; a < 6; ++a) h[21 + a] += j[a] * jr[18 + r];
          }
        }
#pragma unroll
        for (int k = 0; k < 27; ++k) h[k] = wave_sum64(h[k]);
        if (lane == 0) {
#pragma unroll
          for (int k = 0; k < 27; ++k) hcb[b][27 * (size_t)v + k] = h[k];
        }
      }
    }
  };

  // the cameras' share of the gradient and x norms at buffer b (thread per
  // camera parameter); returns this thread's clamped LM diagonal entry
  auto cam_terms = [&](int b, bool first) -> double {
    double d2 = 0.0;
    if (tid < n) {
      const int v = tid / 6, k = tid - 6 * v;
      const double h = hcb[b][27 * (size_t)v + tri(k, k)], g = hcb[b][27 * (size_t)v + 21 + k];
      if (first) sc[tid] = o.jacobi ? 1.0 / (1.0 + sqrt(h)) : 1.0;
      const double s = sc[tid];
      d2 = fmin(fmax(h * s * s, o.min_diag), o.max_diag);
      const double x = xcam[b * kWinN + tid];
      const double d = x - (x + (-g));
      acc[WS_GMAX] = fmax(acc[WS_GMAX], fabs(d));
      acc[WS_GN2] += d * d;
      acc[WS_XN2] += x * x;
    }
    return d2;
  };

  // ---- iteration 0: linearisation at x
  int cur = 0;
  double tot[kWinSlots];
  acc_clear();
  cam_tables(0, false);
  __syncthreads();
  point_pass(0, 0, false, true);
  __syncthreads();
  cam_pass(0);
  __syncthreads();
  {
    const double d2 = cam_terms(0, true);
    if (tid < n) dg[tid] = d2;
  }
  reduce(tot);

  double x_cost = tot[WS_COST], gmax = tot[WS_GMAX], gnorm = sqrt(tot[WS_GN2]), xnorm = sqrt(tot[WS_XN2]);
  const double initial_cost = x_cost;
  int iteration = 0, nsucc = 0, nunsucc = 0, termination = BA_NO_CONVERGENCE, nlog = 0;
  auto push = [&](int it, int valid, int succ, double cost, double cost_change, double step_norm, double rel,
                  double radius, double mcc) {
    if (tid == 0 && nlog < A.log_cap) {
      ba_iteration r;
      r.iteration = it;
      r.step_is_valid = valid;
      r.step_is_successful = succ;
      r.linear_solver_iterations = it > 0 ? 1 : 0;
      r.cost = cost;
      r.cost_change = cost_change;
      r.gradient_max_norm = gmax;
      r.gradient_norm = gnorm;
      r.step_norm = step_norm;
      r.relative_decrease = rel;
      r.trust_region_radius = radius;
      r.model_cost_change = mcc;
      r.iteration_time_s = 0.0;
      logp[nlog] = r;
    }
    ++nlog;
  };

  if (!(tot[WS_BAD] == 0.0 && isfinite(x_cost))) {
    termination = BA_FAILURE;
  } else {
    double radius = o.r0, decrease = 2.0;
    int consecutive_invalid = 0;
    bool last_success = true;
    push(0, 1, 1, x_cost, 0.0, 0.0, 0.0, radius, 0.0);
    while (true) {
      if (iteration >= o.max_iter) { termination = BA_NO_CONVERGENCE; break; }
      if (last_success && gmax <= o.gtol) { termination = BA_CONVERGENCE; break; }
      if (radius <= o.rmin) { termination = BA_CONVERGENCE; break; }
      ++iteration;
      const int nxt = cur ^ 1;
      acc_clear();

      // ---- elim: point blocks at this radius, W per (point, camera) group
      if (act) {
        for (int e = lane; e < PS; e += 64) myS[e] = 0.0;
        for (int p = tid; p < np; p += NT) {
          if (!pt_var[p]) continue;
          const double* hp = Hpb[cur] + 9 * (size_t)p;
          double s[3], D2[3], gs[3];
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            s[k] = scale_p[3 * (size_t)p + k];
            const double hkk = hp[k == 0 ? 0 : (k == 1 ? 3 : 5)];
            const double D = sqrt(fmin(fmax(hkk * s[k] * s[k], o.min_diag), o.max_diag) / radius);
            D2[k] = D * D;
            gs[k] = hp[6 + k] * s[k];
          }
          const double h00 = hp[0] * s[0] * s[0] + D2[0];
          const double h10 = hp[1] * s[0] * s[1];
          const double h20 = hp[2] * s[0] * s[2];
          const double h11 = hp[3] * s[1] * s[1] + D2[1];
          const double h21 = hp[4] * s[1] * s[2];
          const double h22 = hp[5] * s[2] * s[2] + D2[2];
          bool ok = h00 > 0.0;
          const double l00 = sqrt(h00);
          const double l10 = h10 / l00, l20 = h20 / l00;
          const double d11 = h11 - l10 * l10;
          ok = ok && d11 > 0.0;
          const double l11 = sqrt(d11);
          const double l21 = (h21 - l20 * l10) / l11;
          const double d22 = h22 - l20 * l20 - l21 * l21;
          ok = ok && d22 > 0.0;
          const double l22 = sqrt(d22);
          const double i00 = 1.0 / l00, i11 = 1.0 / l11, i22 = 1.0 / l22;
          const double i10 = -(l10 * i00) * i11;
          const double i21 = -(l21 * i11) * i22;
          const double i20 = -(l20 * i00 + l21 * i10) * i22;
          double* q = prec + 9 * (size_t)p;
          q[0] = i00; q[1] = i10; q[2] = i11; q[3] = i20; q[4] = i21; q[5] = i22;
          q[6] = i00 * gs[0];
          q[7] = i10 * gs[0] + i11 * gs[1];
          q[8] = i20 * gs[0] + i21 * gs[1] + i22 * gs[2];
          acc[WS_ELIM_BAD] += ok ? 0.0 : 1.0;
          // E = (Jc s_c)^T (Jp s_p) summed over the group, W = E L^-T at the group's first observation
          double E[18];
          int first_ob = -1;
          auto flush = [&]() {
            if (first_ob < 0) return;
            double* Wo = Wb + 18 * (size_t)first_ob;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
              Wo[3 * a] = E[3 * a] * i00;
              Wo[3 * a + 1] = E[3 * a] * i10 + E[3 * a + 1] * i11;
              Wo[3 * a + 2] = E[3 * a] * i20 + E[3 * a + 1] * i21 + E[3 * a + 2] * i22;
            }
          };
          for (int ob = poff[p]; ob < poff[p + 1]; ++ob) {
            const int v = cam_vc[obs_cam[ob]];
            if (v < 0) continue;
            if (obs_slot[ob] >= 0) {
              flush();
              first_ob = ob;
#pragma unroll
              for (int k = 0; k < 18; ++k) E[k] = 0.0;
            }
            const double* jr = JRb[cur] + (size_t)kJR * ob;
            const double jp[6] = {jr[12] * s[0], jr[13] * s[1], jr[14] * s[2], jr[15] * s[0], jr[16] * s[1], jr[17] * s[2]};
#pragma unroll
            for (int a = 0; a < 6; ++a) {
              const double c0 = jr[a] * sc[6 * v + a], c1 = jr[6 + a] * sc[6 * v + a];
#pragma unroll
              for (int t = 0; t < 3; ++t) E[3 * a + t] += c0 * jp[t] + c1 * jp[3 + t];
            }
          }
          flush();
        }
      }
      __syncthreads();

      // ---- schur: wave-private S -= W_i W_j^T, rhs -= W_i u
      if (act) {
        const int p0 = (int)((long long)np * wave / NW), p1 = (int)((long long)np * (wave + 1) / NW);
        for (int p = p0; p < p1; ++p) {
          if (!pt_var[p]) continue;   // (wave-uniform)
          const int a0 = poff[p], a1 = poff[p + 1];
          int m = 0;
          for (int base = a0; base < a1; base += 64) {
            const int ob = base + lane;
            const int v = ob < a1 ? obs_slot[ob] : -1;
            const unsigned long long mask = __ballot(v >= 0);
            if (v >= 0) {
              const int pos = m + __popcll(mask & ((1ull << lane) - 1ull));
              if (pos < kWinMaxCams) { mywl[pos] = ob; mywl[kWinMaxCams + pos] = v; }
            }
            m += __popcll(mask);
          }
          m = min(m, kWinMaxCams);   // (distinct variable cameras: never more; a bound for the indices below)
          wave_lds_sync();
          const double* q = prec + 9 * (size_t)p;
          const int T = m * (m + 1) / 2 * 36;
          for (int t = lane; t < T; t += 64) {
            const int pq = t / 36, e = t - 36 * pq;
            int i = 0;
            while ((i + 1) * (i + 2) / 2 <= pq) ++i;
            const int j = pq - i * (i + 1) / 2;
            const int ra = e / 6, rb = e - 6 * ra;
            if (i == j && rb > ra) continue;
            const double* Wi = Wb + 18 * (size_t)mywl[i] + 3 * ra;
            const double* Wj = Wb + 18 * (size_t)mywl[j] + 3 * rb;
            const int I = 6 * mywl[kWinMaxCams + i] + ra, J = 6 * mywl[kWinMaxCams + j] + rb;
            myS[tri(I, J)] -= Wi[0] * Wj[0] + Wi[1] * Wj[1] + Wi[2] * Wj[2];
          }
          for (int t = lane; t < 6 * m; t += 64) {
            const int i = t / 6, ra = t - 6 * i;
            const double* Wi = Wb + 18 * (size_t)mywl[i] + 3 * ra;
            myS[rhs0 + 6 * mywl[kWinMaxCams + i] + ra] -= Wi[0] * q[6] + Wi[1] * q[7] + Wi[2] * q[8];
          }
          wave_lds_sync();
        }
      }
      __syncthreads();

      // ---- fold the copies in wave order, then + s Hcc s + D^2 and + s g_c
      for (int e = tid; e < PS; e += kWinThreads) {
        double v = S0[e];
        for (int w = 1; w < NW; ++w) v += Sw[(size_t)w * PS + e];
        S0[e] = v;
      }
      __syncthreads();
      for (int t = tid; t < 27 * nvc; t += kWinThreads) {
        const int v = t / 27, k = t - 27 * v;
        const double h = hcb[cur][27 * (size_t)v + k];
        if (k < 21) {
          int a2 = 0;
          while ((a2 + 1) * (a2 + 2) / 2 <= k) ++a2;
          const int b2 = k - a2 * (a2 + 1) / 2;
          double add = h * sc[6 * v + a2] * sc[6 * v + b2];
          if (a2 == b2) {
            const double D = sqrt(dg[6 * v + a2] / radius);
            add += D * D;
          }
          S0[tri(6 * v + a2, 6 * v + b2)] += add;
        } else {
          S0[rhs0 + 6 * v + (k - 21)] += h * sc[6 * v + (k - 21)];
        }
      }
      __syncthreads();

      // ---- factor: right-looking Cholesky of the packed lower triangle, the
      // rhs as row n.  Every thread reads the pivot itself: chol_ok is uniform.
      bool chol_ok = true;
      for (int j = 0; j < n; ++j) {
        const double d = S0[tri(j, j)];
        if (!(d > 0.0 && isfinite(d))) chol_ok = false;
        const double lj = sqrt(d);
        if (tid == 0) Ld[j] = lj;
        for (int i = j + 1 + tid; i <= n; i += kWinThreads) S0[tri(i, j)] /= lj;
        __syncthreads();
        for (int i = j + 1 + wave; i <= n; i += kWinWaves) {
          const double lij = S0[tri(i, j)];
          const int kmax = min(i, n - 1);
          for (int k = j + 1 + lane; k <= kmax; k += 64) S0[tri(i, k)] -= lij * S0[tri(k, j)];
        }
        __syncthreads();
      }
      // back substitution L^T y = z (row n) in wave 0
      if (wave == 0) {
        for (int k = n - 1; k >= 0; --k) {
          if (lane == 0) yv[k] = S0[rhs0 + k] / Ld[k];
          wave_lds_sync();
          const double yk = yv[k];
          for (int i = lane; i < k; i += 64) S0[rhs0 + i] -= S0[tri(k, i)] * yk;
          wave_lds_sync();
        }
      }
      __syncthreads();

      // ---- camera step: delta_c = -y s_c (into Ld, the pivots are done), x' = x + delta_c
      if (tid < n) {
        const double dl = (-yv[tid]) * sc[tid];
        const double x = xcam[cur * kWinN + tid], xn = x + dl;
        xcam[nxt * kWinN + tid] = xn;
        const double e = x - xn;
        acc[WS_STEP2] += e * e;
        if (!isfinite(dl)) acc[WS_STEP_BAD] += 1.0;
        Ld[tid] = dl;
      }
      __syncthreads();
      cam_tables(nxt, true);
      __syncthreads();
      point_pass(cur, nxt, true, false);
      __syncthreads();
      cam_pass(nxt);
      __syncthreads();
      const double d2n = cam_terms(nxt, false);
      reduce(tot);

      // ---- decide (solve(), ba_solver.hip): identical in every thread
      const double mcc = -tot[WS_MNEG];
      const bool linear_ok = chol_ok && tot[WS_ELIM_BAD] == 0.0 && tot[WS_STEP_BAD] == 0.0;
      const bool valid = linear_ok && mcc > 0.0;
      if (!valid) {
        if (++consecutive_invalid >= o.max_invalid) { termination = BA_FAILURE; break; }
        radius = radius / decrease;
        decrease *= 2.0;
        last_success = false;
        ++nunsucc;
        push(iteration, 0, 0, x_cost, 0.0, 0.0, 0.0, radius, mcc);
        continue;
      }
      consecutive_invalid = 0;
      const double step_norm = sqrt(tot[WS_STEP2]);
      if (step_norm <= o.ptol * (xnorm + o.ptol)) { termination = BA_CONVERGENCE; break; }
      const double dmax = 1.7976931348623157e308;
      const double cand_cost = (tot[WS_CBAD] > 0.0 || !isfinite(tot[WS_CCOST])) ? dmax : tot[WS_CCOST];
      const double cost_change = x_cost - cand_cost;
      if (fabs(cost_change) <= o.ftol * x_cost) { termination = BA_CONVERGENCE; break; }
      const double rel = cand_cost >= dmax ? -dmax : (x_cost - cand_cost) / mcc;
      if (rel > o.min_rel) {
        cur = nxt;
        if (tid < n) dg[tid] = d2n;
        x_cost = tot[WS_COST];
        if (!(tot[WS_BAD] == 0.0 && isfinite(x_cost))) { termination = BA_FAILURE; break; }
        gmax = tot[WS_GMAX];
        gnorm = sqrt(tot[WS_GN2]);
        xnorm = sqrt(tot[WS_XN2]);
        const double t3 = 2.0 * rel - 1.0;
        radius = fmin(o.rmax, radius / fmax(1.0 / 3.0, 1.0 - t3 * t3 * t3));
        decrease = 2.0;
        last_success = true;
        ++nsucc;
        push(iteration, 1, 1, x_cost, cost_change, step_norm, rel, radius, mcc);
      } else {
        radius = radius / decrease;
        decrease *= 2.0;
        last_success = false;
        ++nunsucc;
        push(iteration, 1, 0, cand_cost, cost_change, step_norm, rel, radius, mcc);
      }
    }
  }
  __syncthreads();

  // ---- results: blocks outside the problem keep the caller's values
  for (int i = tid; i < 6 * nc; i += kWinThreads) {
    const int c = i / 6, v = cam_vc[c];
    A.cams_out[6 * (size_t)pr.cam0 + i] = v >= 0 ? xcam[cur * kWinN + 6 * v + (i - 6 * c)] : cams_in[i];
  }
  for (int i = tid; i < 3 * np; i += kWinThreads) A.pts_out[3 * (size_t)pr.pt0 + i] = ptsb[cur][i];
  if (tid == 0) {
    double* sm = A.summ + 8 * (size_t)blockIdx.x;
    sm[0] = initial_cost;
    sm[1] = x_cost;
    sm[2] = iteration;
    sm[3] = nsucc;
    sm[4] = nunsucc;
    sm[5] = termination;
    sm[6] = min(nlog, A.log_cap);
    sm[7] = 0.0;
  }
}

int launch_window_batch(int nprob, const WinArgs& A, const PoseOpts& o, size_t lds_bytes, hipStream_t s) {
  if (nprob <= 0) return (int)hipSuccess;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_window_batch),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_window_batch, dim3(nprob), dim3(kWinThreads), lds_bytes, s, A, o);
  return (int)hipGetLastError();
}

}  // namespace bahip
