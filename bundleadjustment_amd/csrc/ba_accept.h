// ba_accept.h — the float acceptance arithmetic shared by k_prune
// (pruneCorrespondences, Optimizer.cpp:6-79) and k_triangulate
// (SfMHelper::triangulatePoints, SfMHelper.cpp:804-858).  The result bits are
// observable output, so the arithmetic is pinned: round-to-nearest intrinsics
// (no contraction into FMAs), IEEE division and square root, matrix-vector
// products accumulated column by column, norms as sqrt((x*x + y*y) + z*z).
// Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace bahip {

// v = extr * [X; 1] (col-major 4x4); camspacePos = v.hnormalized() is taken
// by the caller entry by entry (acc_hdiv)
__device__ __forceinline__ void acc_cam_h(const float* __restrict__ e, float x0, float x1, float x2, float (&v)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
    v[i] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(e[i], x0), __fmul_rn(e[4 + i], x1)), __fmul_rn(e[8 + i], x2)),
                     e[12 + i]);
}
__device__ __forceinline__ float acc_hdiv(float a, float w) { return __fdiv_rn(a, w); }

// |X - centre|
__device__ __forceinline__ float acc_world_dist(const float* __restrict__ ctr, float x0, float x1, float x2) {
  const float d0 = __fsub_rn(x0, ctr[0]), d1 = __fsub_rn(x1, ctr[1]), d2 = __fsub_rn(x2, ctr[2]);
  return __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2)));
}

// |(K * c).hnormalized() - uv| * invSigma: a norm, not a squared norm
__device__ __forceinline__ float acc_chi(const float* __restrict__ k, float cx, float cy, float cz, float u, float v,
                                         float inv_sigma) {
  float q[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    q[i] = __fadd_rn(__fadd_rn(__fmul_rn(k[i], cx), __fmul_rn(k[3 + i], cy)), __fmul_rn(k[6 + i], cz));
  const float e0 = __fsub_rn(__fdiv_rn(q[0], q[2]), u);
  const float e1 = __fsub_rn(__fdiv_rn(q[1], q[2]), v);
  const float nrm = __fsqrt_rn(__fadd_rn(__fmul_rn(e0, e0), __fmul_rn(e1, e1)));
  return __fmul_rn(nrm, inv_sigma);
}

constexpr float kAccChiThresh = 5.991f;   // float chiThresh = 5.991

}  // namespace bahip
