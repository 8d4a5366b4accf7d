// ba_lin.h — the per-observation linearisation shared by the general LM
// kernels (ba_kernels.hip), the batched small-window solver (ba_window.hip)
// and the batched triangulation (ba_triangulate.hip): camera record entries,
// the value-only projection, the K-folded camera table accessor and lin_obs.
// Device code only.
#pragma once
#include "ba_device.h"
#include "ba_kernels.h"

namespace bahip {

__device__ inline double cam_rec_entry(int e, const double* w, const double* t, const double* Kd, const D3* R,
                                       const double* R0, bool deriv) {
  if (e < 9) return deriv ? R[e].a : R0[e];
  if (e < 36) { const int k = (e - 9) / 9, i = (e - 9) % 9; return deriv ? R[i].d[k] : 0.0; }
  if (e < 39) return t[e - 36];
  if (e < 48) return Kd[e - 39];
  if (!deriv) return 0.0;
  const int l = e - kRecL;
  if (l < 36) {   // K M, M = R or dR/dw_k, col-major
    const int m = l / 9, idx = l % 9, col = idx / 3, row = idx % 3;
    double M0, M1, M2;
    if (m == 0) { M0 = R[col * 3].a; M1 = R[col * 3 + 1].a; M2 = R[col * 3 + 2].a; }
    else { M0 = R[col * 3].d[m - 1]; M1 = R[col * 3 + 1].d[m - 1]; M2 = R[col * 3 + 2].d[m - 1]; }
    return Kd[row] * M0 + Kd[3 + row] * M1 + Kd[6 + row] * M2;
  }
  if (l < 39) { const int row = l - 36; return Kd[row] * t[0] + Kd[3 + row] * t[1] + Kd[6 + row] * t[2]; }
  return 0.0;
}

// Project one observation; value only.  Returns residual (u,v) in r.
__device__ inline void project_value(const double* __restrict__ cr, bool cvar, double X0, double X1, double X2,
                                     float2 uv, double r[2]) {
  double p[3];
  if (cvar) {
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = cr[kRecR + i] * X0 + cr[kRecR + 3 + i] * X1 + cr[kRecR + 6 + i] * X2 + cr[kRecT + i];
  } else {
    double ph[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ph[i] = X0 * cr[i] + X1 * cr[4 + i] + X2 * cr[8 + i] + cr[12 + i];
    p[0] = ph[0] / ph[3]; p[1] = ph[1] / ph[3]; p[2] = ph[2] / ph[3];
  }
  const double* Kc = cr + kRecK;
  double q[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) q[i] = p[0] * Kc[i] + p[1] * Kc[3 + i] + p[2] * Kc[6 + i];
  r[0] = q[0] / q[2] - (double)uv.x;
  r[1] = q[1] / q[2] - (double)uv.y;
}

// ---------------------------------------------------------------------------
// Per-observation Jacobian/residual record (AoS, 20 doubles = 160 B):
//   [0..5]  Jc row 0   [6..11] Jc row 1   [12..14] Jp row 0   [15..17] Jp row 1
//   [18] r0  [19] r1          (Huber-corrected)
// One record per observation in (point, camera) order: the per-point and
// per-observation passes stream it, the per-camera passes gather whole
// records (1-2 cache lines each instead of 14 scattered SoA lines).
// ---------------------------------------------------------------------------
constexpr int kJR = 20;

// ---------------------------------------------------------------------------
// linearisation: one thread per observation (sorted by point)
// ---------------------------------------------------------------------------
// Camera access for the linearisation: the K-folded table (kRecL, 40
// doubles, read as 20 16-B loads) and K (float-valued) from the block's LDS
// copy of the camera table.
// LDS row: lin table (40) + variable flag (slot 40) + pad; stride 42 doubles
// keeps rows 16-B aligned and spreads random cameras over the 16 bank
// groups of ds_read_b128
constexpr int kTblRec = kLin + 2;
struct CamLds {
  const double* r;
  const float* k;
  __device__ bool var() const { return r[kLin] != 0.0; }
  __device__ void load(double (&t)[kLin]) const {
    const double2* s = reinterpret_cast<const double2*>(r);
#pragma unroll
    for (int k = 0; k < kLin / 2; ++k) { const double2 u = s[k]; t[2 * k] = u.x; t[2 * k + 1] = u.y; }
  }
  __device__ double K(int i) const { return (double)k[i]; }
};
// camera row as an indexable value: a register copy
struct RowRegs {
  double t[kLin];
  __device__ double operator[](int i) const { return t[i]; }
};
template <class Cam>
__device__ inline RowRegs cam_row(const Cam& cr) { RowRegs R; cr.load(R.t); return R; }

// r, J (Huber-corrected) of one observation into out[20]; returns rho.
// AngleReprojectionError (Optimizer.h:54-76) / PointOnlyReprojectionError
// (Optimizer.h:96-107) with the chain rule of their Jets:
//   q = K (R X + t),  dq/dw_k = K dR_k X,  dq/dt = K,  dq/dX = K R
//   fixed: q = K E(0:3) [X;1] / w,  w = E(3) [X;1],  dq/dX = (K E - q e3) / w
//   r = q01 / q2 - uv,  dr/d* = (dq01 - r' dq2) / q2,  Huber corrector sqrt(rho')
template <class Cam>
__device__ inline double lin_obs(const DevProblem& P, const Cam& cr, bool cvar, bool pvar, double X0, double X1,
                                 double X2, float2 uv, double (&out)[kJR], bool& fin, double* prf = nullptr) {
  const auto T = cam_row(cr);
  double q[3], iw = 1.0;
  if (cvar) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
      q[i] = T[kLinKR + i] * X0 + T[kLinKR + 3 + i] * X1 + T[kLinKR + 6 + i] * X2 + T[kLinKt + i];
  } else {
    const double wv = T[kLinE3] * X0 + T[kLinE3 + 1] * X1 + T[kLinE3 + 2] * X2 + T[kLinE3 + 3];
    iw = 1.0 / wv;
#pragma unroll
    for (int i = 0; i < 3; ++i)
      q[i] = (T[kLinKE + i] * X0 + T[kLinKE + 3 + i] * X1 + T[kLinKE + 6 + i] * X2 + T[kLinKE + 9 + i]) * iw;
  }
  const double iq = 1.0 / q[2];
  const double pr0 = q[0] * iq, pr1 = q[1] * iq;
  const double r0 = pr0 - (double)uv.x, r1 = pr1 - (double)uv.y;
  double scale;
  const double rho = huber(r0 * r0 + r1 * r1, P.huber_a, P.huber_b, &scale);
  const double f = iq * scale;
  fin = isfinite(r0) && isfinite(r1) && isfinite(f);
  if (prf) { prf[0] = pr0; prf[1] = pr1; prf[2] = f; }   // (k_obs_w_rc's compact records)
  if (cvar) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int b = kLinKdR + 9 * k;
      const double d0 = T[b] * X0 + T[b + 3] * X1 + T[b + 6] * X2;
      const double d1 = T[b + 1] * X0 + T[b + 4] * X1 + T[b + 7] * X2;
      const double d2 = T[b + 2] * X0 + T[b + 5] * X1 + T[b + 8] * X2;
      out[k] = (d0 - pr0 * d2) * f;
      out[6 + k] = (d1 - pr1 * d2) * f;
      const double k2 = cr.K(3 * k + 2);
      out[3 + k] = (cr.K(3 * k) - pr0 * k2) * f;
      out[9 + k] = (cr.K(3 * k + 1) - pr1 * k2) * f;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k) out[k] = 0.0;
  }
  if (pvar) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double d0, d1, d2;
      if (cvar) {
        d0 = T[kLinKR + 3 * k]; d1 = T[kLinKR + 3 * k + 1]; d2 = T[kLinKR + 3 * k + 2];
      } else {
        const double e = T[kLinE3 + k];
        d0 = (T[kLinKE + 3 * k] - q[0] * e) * iw;
        d1 = (T[kLinKE + 3 * k + 1] - q[1] * e) * iw;
        d2 = (T[kLinKE + 3 * k + 2] - q[2] * e) * iw;
      }
      out[12 + k] = (d0 - pr0 * d2) * f;
      out[15 + k] = (d1 - pr1 * d2) * f;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 6; ++k) out[12 + k] = 0.0;
  }
  out[18] = r0 * scale;
  out[19] = r1 * scale;
#pragma unroll
  for (int k = 0; k < 18; ++k) fin = fin && isfinite(out[k]);
  return rho;
}

// LDS hand-off between the lanes of one wave: DS operations of a wave
// execute in order, so a compiler barrier is enough (a wavefront-scope
// fence made the waitcnt pass drain vmcnt before every LDS read)
__device__ inline void wave_lds_sync() {
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
}

__device__ inline int tri(int a, int b) { return a * (a + 1) / 2 + b; }  // a >= b

}  // namespace bahip
