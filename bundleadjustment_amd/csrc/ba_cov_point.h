// ba_cov_point.h — the 3 x 3 point-block finish of the covariance gathers,
// shared by the dense route (ba_cov.hip) and the iterative one
// (ba_cov_pcg.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace bahip {

// L_p^-1 (lower) and s_p of a variable point
struct CovPt {
  double li[3][3], s[3];
  __device__ __forceinline__ void load(const double* __restrict__ Linv, const double* __restrict__ scale_p, int p,
                                       size_t np) {
    li[0][0] = Linv[p]; li[0][1] = 0.0; li[0][2] = 0.0;
    li[1][0] = Linv[np + p]; li[1][1] = Linv[2 * np + p]; li[1][2] = 0.0;
    li[2][0] = Linv[3 * np + p]; li[2][1] = Linv[4 * np + p]; li[2][2] = Linv[5 * np + p];
    s[0] = scale_p[p]; s[1] = scale_p[np + p]; s[2] = scale_p[2 * np + p];
  }
};

// dst (3 x 3, row-major) = s_p Lp^-T (eye I + t) Lq^-1 s_q: Cov(p, q) from the
// sum of cov_pair_sum (eye = 1 for p == q: the point's marginal)
__device__ __forceinline__ void cov_point_finish(const double (&t)[9], bool eye, const CovPt& cp, const CovPt& cq,
                                                 double (&dst)[9]) {
  double M[3][3], ML[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) M[r][c] = (eye && r == c ? 1.0 : 0.0) + t[r * 3 + c];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double x = 0.0;
#pragma unroll
      for (int l = c; l < 3; ++l) x += M[r][l] * cq.li[l][c];
      ML[r][c] = x;
    }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double x = 0.0;
#pragma unroll
      for (int l = r; l < 3; ++l) x += cp.li[l][r] * ML[l][c];
      dst[r * 3 + c] = cp.s[r] * x * cq.s[c];
    }
}

}  // namespace bahip
