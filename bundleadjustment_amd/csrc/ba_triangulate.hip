// ba_triangulate.hip — batched multi-view triangulation with structure-only
// refinement (gfx950, wave64): SfMHelper::triangulatePoints
// (SfMHelper.cpp:759-878: cv::triangulatePoints + three float acceptance
// tests) for any number of views per point, and the dual of k_pose_batch:
// many points refined independently against constant cameras, the whole
// Levenberg-Marquardt loop of every point in ONE launch.
//
// Prologue (k_tri_cams), thread per camera entry: the value-only record of a
// constant camera (E, K as doubles: project_value's layout) and the K-folded
// table lin_obs reads (K E(0:3, :) col-major, E(3, :)).  K E(0:3, :) is also
// the projection matrix P of the DLT: one table serves both.
//
// Main kernel (k_triangulate): kTriGroup = 8 lanes per point, 8 points per
// wave.  The group size is a compile-time constant, never chosen from the
// batch: lane l of a group takes the point's views l, l + 8, ... and every sum
// is folded by an xor butterfly over the group, so all lanes of a group hold
// the bitwise-identical totals, a point's bits depend on its own observations
// alone, and the LM bookkeeping runs group-uniform in registers.  No LDS, no
// barrier, no dependency between groups: a group that has terminated idles
// until its wave's last group ends.
//   DLT     M = A^T A (4x4, fp64) from the rows u P2 - P0, v P2 - P1 of every
//           view; eigenvector of the smallest eigenvalue by cyclic Jacobi
//           rotations in registers; X = v[0:3] / v[3]
//   LM      solve() (ba_solver.hip) restated per group as k_pose_batch does
//           per wave: per iteration the 3x3 damped solve (the window kernel's
//           elim step: A = s Hpp s + D^2 = L L^T), then ONE pass over the
//           views: model cost change from J(x), candidate cost at x'
//           (project_value), speculative linearisation at x' (lin_obs)
//   accept  the float tests of ba_accept.h on (float)X
#include <hip/hip_runtime.h>

#include "ba_accept.h"
#include "ba_kernels.h"
#include "ba_device.h"
#include "ba_lin.h"
#include "../../include/ba_hip.h"

namespace bahip {

constexpr int kTriThreads = 256;
constexpr int kTriSweeps = 16;            // bound on the Jacobi sweeps (the stopping rule ends them after 4-6)
constexpr double kTriOffTol = 1e-36;      // stop when sum offdiag^2 <= kTriOffTol * sum diag^2
constexpr double kTriRankTol = 1e-12;     // lambda_2 <= kTriRankTol * lambda_max: the rays coincide, no point
static_assert(kTriRec == kRecL + 16 && kTriGroup == 8, "camera record layout");
static_assert(BA_TRI_OK == 0 && BA_TRI_SCALE == 5, "status codes");

__device__ __forceinline__ double grp_sum(double v) {
#pragma unroll
  for (int off = 1; off < kTriGroup; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ int grp_sum(int v) {
#pragma unroll
  for (int off = 1; off < kTriGroup; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// constant camera for lin_obs: the 16 live entries of the K-folded table
struct CamFixed {
  const double* r;
  __device__ void load(double (&t)[kLin]) const {
    const double2* s = reinterpret_cast<const double2*>(r);
#pragma unroll
    for (int k = 0; k < 8; ++k) { const double2 u = s[k]; t[2 * k] = u.x; t[2 * k + 1] = u.y; }
#pragma unroll
    for (int k = 16; k < kLin; ++k) t[k] = 0.0;
  }
  __device__ double K(int) const { return 0.0; }
};

__global__ __launch_bounds__(256) void k_tri_cams(int nc, const float* __restrict__ extr, const float* __restrict__ Kf,
                                                  double* __restrict__ rec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nc * kTriRec) return;
  const int c = i / kTriRec, e = i - c * kTriRec;
  const float* E = extr + 16 * (size_t)c;
  const float* Kc = Kf + 9 * (size_t)c;
  double v = 0.0;
  if (e < 16) {
    v = (double)E[e];
  } else if (e >= kRecK && e < kRecL) {
    v = (double)Kc[e - kRecK];
  } else if (e >= kRecL) {   // PointOnlyReprojectionError: K E(0:3, :), E(3, :) (k_cam_prep's constant-camera record)
    const int l = e - kRecL;
    if (l < 12) {
      const int col = l / 3, row = l % 3;
      v = (double)Kc[row] * (double)E[col * 4] + (double)Kc[3 + row] * (double)E[col * 4 + 1] +
          (double)Kc[6 + row] * (double)E[col * 4 + 2];
    } else {
      v = (double)E[(l - 12) * 4 + 3];
    }
  }
  rec[i] = v;
}

// Cyclic Jacobi on a symmetric 4x4 (full storage), pairs in the order (0,1)
// (0,2) (0,3) (1,2) (1,3) (2,3); V accumulates the rotations (columns =
// eigenvectors).  Stopping rule: before each sweep, stop when the squared
// off-diagonal mass is <= 1e-36 of the squared diagonal mass (or is not a
// number), at most kTriSweeps sweeps.
__device__ inline void jacobi4(double (&S)[4][4], double (&V)[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kTriSweeps; ++sweep) {
    double off2 = 0.0, d2 = 0.0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      d2 += S[p][p] * S[p][p];
#pragma unroll
      for (int q = p + 1; q < 4; ++q) off2 += S[p][q] * S[p][q];
    }
    if (!(off2 > kTriOffTol * d2)) break;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        const double apq = S[p][q];
        if (apq != 0.0) {
          const double theta = (S[q][q] - S[p][p]) / (2.0 * apq);
          const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
          const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (k != p && k != q) {
              const double akp = S[k][p], akq = S[k][q];
              S[k][p] = S[p][k] = c * akp - s * akq;
              S[k][q] = S[q][k] = s * akp + c * akq;
            }
            const double vkp = V[k][p], vkq = V[k][q];
            V[k][p] = c * vkp - s * vkq;
            V[k][q] = s * vkp + c * vkq;
          }
          S[p][p] -= t * apq;
          S[q][q] += t * apq;
          S[p][q] = S[q][p] = 0.0;
        }
      }
  }
}

// Hpp (xx xy xz yy yz zz) and g_p of one observation's point block
__device__ __forceinline__ void tri_acc(const double (&out)[kJR], double (&H)[6], double (&g)[3]) {
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const double* j = out + 12 + 3 * r;
    H[0] += j[0] * j[0]; H[1] += j[0] * j[1]; H[2] += j[0] * j[2];
    H[3] += j[1] * j[1]; H[4] += j[1] * j[2]; H[5] += j[2] * j[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] += j[k] * out[18 + r];
  }
}

__global__ __launch_bounds__(kTriThreads, 2) void k_triangulate(TriArgs A, PoseOpts o) {
  const size_t gid = (size_t)blockIdx.x * (kTriThreads / kTriGroup) + threadIdx.x / kTriGroup;
  const int gl = threadIdx.x & (kTriGroup - 1);
  if (gid >= (size_t)A.n_pts) return;   // (whole groups: a group's lanes always run together)
  const size_t p = gid;
  const int o0 = A.off[p], o1 = A.off[p + 1], nv = o1 - o0;
  double X[3] = {0.0, 0.0, 0.0};
  if (A.init_given) {
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = A.pts_init[3 * p + k];
  }
  int status = BA_TRI_OK;
  double initial_cost = 0.0, x_cost = 0.0;
  int iteration = 0, nsucc = 0, nunsucc = 0, termination = BA_CONVERGENCE;

  if (nv < max(2, A.min_views)) {
    status = BA_TRI_FEW_VIEWS;
  } else {
    // ---- DLT
    if (!A.init_given) {
      double m[10];
#pragma unroll
      for (int k = 0; k < 10; ++k) m[k] = 0.0;
      for (int ob = o0 + gl; ob < o1; ob += kTriGroup) {
        const double* T = A.rec + (size_t)kTriRec * A.obs_cam[ob] + kRecL;
        const float2 uv = A.uv[ob];
        const double u = (double)uv.x, v = (double)uv.y;
        double a[4], b[4];
#pragma unroll
        for (int col = 0; col < 4; ++col) {
          const double P0 = T[3 * col], P1 = T[3 * col + 1], P2 = T[3 * col + 2];
          a[col] = u * P2 - P0;
          b[col] = v * P2 - P1;
        }
        int t = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j <= i; ++j) m[t++] += a[i] * a[j] + b[i] * b[j];
      }
      double S[4][4], V[4][4];
      {
        int t = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j <= i; ++j) { const double s = grp_sum(m[t++]); S[i][j] = s; S[j][i] = s; }
      }
      jacobi4(S, V);
      // smallest eigenvalue (lowest index on a tie), the second smallest, the largest
      int im = 0;
      double l1 = S[0][0];
#pragma unroll
      for (int i = 1; i < 4; ++i) if (S[i][i] < l1) { l1 = S[i][i]; im = i; }
      double l2 = 1.7976931348623157e308, lmax = 0.0, vm[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i != im) l2 = fmin(l2, S[i][i]);
        lmax = fmax(lmax, fabs(S[i][i]));
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) vm[k] = im == 0 ? V[k][0] : (im == 1 ? V[k][1] : (im == 2 ? V[k][2] : V[k][3]));
      const bool rank_ok = l2 > kTriRankTol * lmax;
      const double qnan = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll
      for (int k = 0; k < 3; ++k) X[k] = rank_ok ? vm[k] / vm[3] : qnan;
    }

    // ---- per-point LM: solve() for one variable point, every camera constant
    if (A.refine) {
      DevProblem P{};
      P.huber_a = A.huber_a;
      P.huber_b = A.huber_a * A.huber_a;
      double H[6], g[3], cost = 0.0, bad = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) H[k] = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) g[k] = 0.0;
      for (int ob = o0 + gl; ob < o1; ob += kTriGroup) {
        double out[kJR];
        bool fin;
        const double rho = lin_obs(P, CamFixed{A.rec + (size_t)kTriRec * A.obs_cam[ob] + kRecL}, false, true, X[0],
                                   X[1], X[2], A.uv[ob], out, fin);
        cost += 0.5 * rho;
        bad += fin ? 0.0 : 1.0;
        tri_acc(out, H, g);
      }
#pragma unroll
      for (int k = 0; k < 6; ++k) H[k] = grp_sum(H[k]);
#pragma unroll
      for (int k = 0; k < 3; ++k) g[k] = grp_sum(g[k]);
      cost = grp_sum(cost);
      bad = grp_sum(bad);

      double s[3];
      s[0] = o.jacobi ? 1.0 / (1.0 + sqrt(H[0])) : 1.0;
      s[1] = o.jacobi ? 1.0 / (1.0 + sqrt(H[3])) : 1.0;
      s[2] = o.jacobi ? 1.0 / (1.0 + sqrt(H[5])) : 1.0;
      double gmax = 0.0, xnorm = 0.0;
      auto norms = [&]() {
        double xn2 = 0.0;
        gmax = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double d = X[k] - (X[k] + (-g[k]));
          gmax = fmax(gmax, fabs(d));
          xn2 += X[k] * X[k];
        }
        xnorm = sqrt(xn2);
      };
      norms();
      x_cost = cost;
      initial_cost = cost;
      termination = BA_NO_CONVERGENCE;
      if (!(bad == 0.0 && isfinite(cost))) {
        termination = BA_FAILURE;
      } else {
        double radius = o.r0, decrease = 2.0;
        int consecutive_invalid = 0;
        bool last_success = true;
        while (true) {
          if (iteration >= o.max_iter) { termination = BA_NO_CONVERGENCE; break; }
          if (last_success && gmax <= o.gtol) { termination = BA_CONVERGENCE; break; }
          if (radius <= o.rmin) { termination = BA_CONVERGENCE; break; }
          ++iteration;
          // ---- elim (ba_window.hip): A = s Hpp s + D^2 = L L^T, L^-1, u = L^-1 s g, y = L^-T u
          double D2[3], gs[3];
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const double hkk = H[k == 0 ? 0 : (k == 1 ? 3 : 5)];
            const double D = sqrt(fmin(fmax(hkk * s[k] * s[k], o.min_diag), o.max_diag) / radius);
            D2[k] = D * D;
            gs[k] = g[k] * s[k];
          }
          const double h00 = H[0] * s[0] * s[0] + D2[0];
          const double h10 = H[1] * s[0] * s[1];
          const double h20 = H[2] * s[0] * s[2];
          const double h11 = H[3] * s[1] * s[1] + D2[1];
          const double h21 = H[4] * s[1] * s[2];
          const double h22 = H[5] * s[2] * s[2] + D2[2];
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
          const double w0 = i00 * gs[0];
          const double w1 = i10 * gs[0] + i11 * gs[1];
          const double w2 = i20 * gs[0] + i21 * gs[1] + i22 * gs[2];
          const double yp[3] = {i00 * w0 + i10 * w1 + i20 * w2, i11 * w1 + i21 * w2, i22 * w2};
          double Xn[3], dp[3], step2 = 0.0;
          bool step_bad = false;
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            dp[k] = (-yp[k]) * s[k];
            Xn[k] = X[k] + dp[k];
            const double e = X[k] - Xn[k];
            step2 += e * e;
            if (!isfinite(dp[k])) step_bad = true;
          }
          // ---- one pass: model cost change (J at x), candidate cost, linearisation at x'
          double mneg = 0.0, ccost = 0.0, cbad = 0.0, H2[6], g2[3], cost2 = 0.0, bad2 = 0.0;
#pragma unroll
          for (int k = 0; k < 6; ++k) H2[k] = 0.0;
#pragma unroll
          for (int k = 0; k < 3; ++k) g2[k] = 0.0;
          for (int ob = o0 + gl; ob < o1; ob += kTriGroup) {
            const double* cr = A.rec + (size_t)kTriRec * A.obs_cam[ob];
            const float2 uv = A.uv[ob];
            double out[kJR];
            bool fin;
            lin_obs(P, CamFixed{cr + kRecL}, false, true, X[0], X[1], X[2], uv, out, fin);
            double jd0 = 0.0, jd1 = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) { jd0 += out[12 + k] * dp[k]; jd1 += out[15 + k] * dp[k]; }
            mneg += jd0 * (out[18] + jd0 / 2.0) + jd1 * (out[19] + jd1 / 2.0);
            double rc[2], sc;
            project_value(cr, false, Xn[0], Xn[1], Xn[2], uv, rc);
            ccost += 0.5 * huber(rc[0] * rc[0] + rc[1] * rc[1], P.huber_a, P.huber_b, &sc);
            if (!isfinite(rc[0]) || !isfinite(rc[1])) cbad += 1.0;
            const double rho2 = lin_obs(P, CamFixed{cr + kRecL}, false, true, Xn[0], Xn[1], Xn[2], uv, out, fin);
            cost2 += 0.5 * rho2;
            bad2 += fin ? 0.0 : 1.0;
            tri_acc(out, H2, g2);
          }
          mneg = grp_sum(mneg);
          ccost = grp_sum(ccost);
          cbad = grp_sum(cbad);
          // ---- decide (solve(), ba_solver.hip): identical in every lane of the group
          const double mcc = -mneg;
          const bool valid = ok && !step_bad && mcc > 0.0;
          if (!valid) {
            if (++consecutive_invalid >= o.max_invalid) { termination = BA_FAILURE; break; }
            radius = radius / decrease;
            decrease *= 2.0;
            last_success = false;
            ++nunsucc;
            continue;
          }
          consecutive_invalid = 0;
          if (sqrt(step2) <= o.ptol * (xnorm + o.ptol)) { termination = BA_CONVERGENCE; break; }
          const double dmax = 1.7976931348623157e308;
          const double cand_cost = (cbad > 0.0 || !isfinite(ccost)) ? dmax : ccost;
          const double cost_change = x_cost - cand_cost;
          if (fabs(cost_change) <= o.ftol * x_cost) { termination = BA_CONVERGENCE; break; }
          const double rel = cand_cost >= dmax ? -dmax : (x_cost - cand_cost) / mcc;
          if (rel > o.min_rel) {
#pragma unroll
            for (int k = 0; k < 6; ++k) H[k] = grp_sum(H2[k]);
#pragma unroll
            for (int k = 0; k < 3; ++k) { g[k] = grp_sum(g2[k]); X[k] = Xn[k]; }
            x_cost = grp_sum(cost2);
            bad = grp_sum(bad2);
            if (!(bad == 0.0 && isfinite(x_cost))) { termination = BA_FAILURE; break; }
            norms();
            const double t3 = 2.0 * rel - 1.0;
            radius = fmin(o.rmax, radius / fmax(1.0 / 3.0, 1.0 - t3 * t3 * t3));
            decrease = 2.0;
            last_success = true;
            ++nsucc;
          } else {
            radius = radius / decrease;
            decrease *= 2.0;
            last_success = false;
            ++nunsucc;
          }
        }
      }
    }

    // ---- acceptance tests (SfMHelper.cpp:804-858) on the float-rounded point
    const float x0 = (float)X[0], x1 = (float)X[1], x2 = (float)X[2];
    if (!(isfinite(x0) && isfinite(x1) && isfinite(x2)) || termination == BA_FAILURE) {
      status = BA_TRI_DEGENERATE;
    } else {
      const bool chk_scale = (A.checks & BA_TRI_CHECK_SCALE) != 0;
      int nbehind = 0, nchi = 0, nscale = 0;
      float d0 = 1.0f, s0 = 1.0f;
      if (chk_scale) {   // view 0: the point's first observation in caller order
        d0 = acc_world_dist(A.center + 3 * (size_t)A.obs_cam[o0], x0, x1, x2);
        s0 = A.scale ? A.scale[o0] : 1.0f;
      }
      for (int ob = o0 + gl; ob < o1; ob += kTriGroup) {
        const int c = A.obs_cam[ob];
        float v[4];
        acc_cam_h(A.extr + 16 * (size_t)c, x0, x1, x2, v);
        const float cz = acc_hdiv(v[2], v[3]);
        if (cz <= 0.0f) ++nbehind;                                        // :806-813
        const float sj = A.scale ? A.scale[ob] : 1.0f;
        if (A.checks & BA_TRI_CHECK_CHI2) {                               // :815-838
          const float cx = acc_hdiv(v[0], v[3]), cy = acc_hdiv(v[1], v[3]);
          const float inv_sigma = (float)(1.0 / (double)sj);
          const float2 uv = A.uv[ob];
          if (acc_chi(A.K + 9 * (size_t)c, cx, cy, cz, uv.x, uv.y, inv_sigma) > kAccChiThresh) ++nchi;
        }
        if (chk_scale && ob != o0) {                                      // :840-858
          const float dj = acc_world_dist(A.center + 3 * (size_t)c, x0, x1, x2);
          const float ros = __fdiv_rn(sj, s0), rwd = __fdiv_rn(d0, dj);
          if (d0 == 0.0f || dj == 0.0f || __fmul_rn(rwd, 1.5f) < ros || rwd > __fmul_rn(ros, 1.5f)) ++nscale;
        }
      }
      nbehind = grp_sum(nbehind);
      nchi = grp_sum(nchi);
      nscale = grp_sum(nscale);
      const bool behind = A.behind_any ? nbehind > 0 : nbehind == nv;
      if ((A.checks & BA_TRI_CHECK_CHEIRALITY) && behind) status = BA_TRI_BEHIND;
      else if (nchi > 0) status = BA_TRI_CHI2;
      else if (nscale > 0) status = BA_TRI_SCALE;
    }
  }

  if (gl < 3) A.pts_out[3 * p + gl] = gl == 0 ? X[0] : (gl == 1 ? X[1] : X[2]);
  if (gl == 0) {
    A.status[p] = (uint8_t)status;
    double* sm = A.summ + 6 * p;
    sm[0] = initial_cost;
    sm[1] = x_cost;
    sm[2] = iteration;
    sm[3] = nsucc;
    sm[4] = nunsucc;
    sm[5] = termination;
  }
}

void launch_triangulate(const TriArgs& A, const PoseOpts& o, hipStream_t s) {
  if (A.n_pts <= 0) return;
  if (A.n_cams > 0) {
    const long long ne = (long long)A.n_cams * kTriRec;
    hipLaunchKernelGGL(k_tri_cams, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, s, A.n_cams, A.extr, A.K, A.rec);
  }
  const int per = kTriThreads / kTriGroup;
  hipLaunchKernelGGL(k_triangulate, dim3((unsigned)(((long long)A.n_pts + per - 1) / per)), dim3(kTriThreads), 0, s, A,
                     o);
}

}  // namespace bahip
