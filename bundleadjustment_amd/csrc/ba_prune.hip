// ba_prune.hip — pruneCorrespondences (Optimizer.cpp:6-79) as a per-pair
// device kernel.  The reference runs it on the host in float after every
// outer BA round; the result bits are observable output, so the arithmetic
// is pinned: round-to-nearest intrinsics (no contraction into FMAs), IEEE
// division and square root, and the operation order documented for ba_prune
// in include/ba_hip.h.  The arithmetic lives in ba_accept.h, shared with
// k_triangulate.
#include "ba_accept.h"
#include "ba_kernels.h"

namespace bahip {

__global__ __launch_bounds__(256) void k_prune(int n, const float* __restrict__ extr,
                                               const float* __restrict__ center, const float* __restrict__ K,
                                               const int* __restrict__ obs_cam, const float* __restrict__ X,
                                               const float* __restrict__ uv, const float* __restrict__ inv_sigma,
                                               const float* __restrict__ dist, uint8_t* __restrict__ out) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n) return;
  const int c = obs_cam[o];
  const float* e = extr + 16 * c;
  const float x0 = X[3 * o], x1 = X[3 * o + 1], x2 = X[3 * o + 2];
  // camspacePos = (extr * X.homogeneous()).hnormalized()      (Optimizer.cpp:33)
  float v[4];
  acc_cam_h(e, x0, x1, x2, v);
  const float cz = acc_hdiv(v[2], v[3]);
  if (cz <= 0.0f) { out[o] = 1; return; }                        // :36-41
  const float cx = acc_hdiv(v[0], v[3]), cy = acc_hdiv(v[1], v[3]);
  // worldDist = |X - frame->getWorldPos()|                       :44-51
  const float wd = acc_world_dist(center + 3 * c, x0, x1, x2);
  if (wd > dist[2 * o + 1] || wd < dist[2 * o]) { out[o] = 2; return; }
  // projPos = (intr * camspacePos).hnormalized(); |projPos - kp| * invSigma > 5.991   :53-64
  const float chi = acc_chi(K + 9 * c, cx, cy, cz, uv[2 * o], uv[2 * o + 1], inv_sigma[o]);
  out[o] = chi > kAccChiThresh ? 3 : 0;
}

void launch_prune(int n, const float* extr, const float* center, const float* K, const int* obs_cam, const float* X,
                  const float* uv, const float* inv_sigma, const float* dist, uint8_t* out, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_prune, dim3((n + 255) / 256), dim3(256), 0, s, n, extr, center, K, obs_cam, X, uv, inv_sigma,
                     dist, out);
}

}  // namespace bahip
