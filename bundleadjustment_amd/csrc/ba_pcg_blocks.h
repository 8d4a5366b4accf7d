// ba_pcg_blocks.h — the 6 x 6 camera-block arithmetic of the implicit reduced
// camera system, shared by the single-vector CG (ba_pcg.hip) and the
// multi-column CG of the iterative covariance (ba_cov_pcg.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace bahip {

// lower-triangle index of (a, b), a >= b
__device__ inline int tri(int a, int b) { return a * (a + 1) / 2 + b; }

// y = A x for a symmetric 6x6 block stored as its lower 21 entries
__device__ inline void sym6_mul(const double* __restrict__ A, const double (&x)[6], double (&y)[6]) {
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    double v = 0.0;
#pragma unroll
    for (int b = 0; b < 6; ++b) v += A[a >= b ? tri(a, b) : tri(b, a)] * x[b];
    y[a] = v;
  }
}

// Inverse of an SPD 6x6 block (lower 21) by LLT + two triangular solves
// against I (Eigen selfadjointView().llt().solve(Identity), as Ceres'
// BlockRandomAccessDiagonalMatrix::Invert).  Returns false if not PD.
__device__ inline bool spd6_inverse(const double (&M)[21], double* __restrict__ out /*36, row-major*/) {
  double L[21];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = M[tri(j, j)];
#pragma unroll
    for (int t = 0; t < j; ++t) d -= L[tri(j, t)] * L[tri(j, t)];
    ok = ok && d > 0.0;
    d = sqrt(d);
    L[tri(j, j)] = d;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = M[tri(i, j)];
#pragma unroll
      for (int t = 0; t < j; ++t) v -= L[tri(i, t)] * L[tri(j, t)];
      L[tri(i, j)] = v / d;
    }
  }
#pragma unroll
  for (int col = 0; col < 6; ++col) {
    double z[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double v = i == col ? 1.0 : 0.0;
#pragma unroll
      for (int t = 0; t < i; ++t) v -= L[tri(i, t)] * z[t];
      z[i] = v / L[tri(i, i)];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
      double v = z[i];
#pragma unroll
      for (int t = i + 1; t < 6; ++t) v -= L[tri(t, i)] * z[t];
      z[i] = v / L[tri(i, i)];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) out[i * 6 + col] = z[i];
  }
  return ok;
}

__device__ inline void mat6_mul(const double* __restrict__ M, const double (&x)[6], double (&y)[6]) {
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    double v = 0.0;
#pragma unroll
    for (int b = 0; b < 6; ++b) v += M[a * 6 + b] * x[b];
    y[a] = v;
  }
}

}  // namespace bahip
