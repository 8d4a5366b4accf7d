// ba_pnp.hip — batched robust absolute pose (gfx950, wave64): P3P RANSAC with
// the whole hypothesis budget scored in parallel, then the pose LM of
// k_pose_batch on the consensus set.  SfMHelper::estimatePoseUsingPnP
// (SfMHelper.cpp:16-104) wanted cv::solvePnPRansac here.
//
//   k_pnp_score    grid (problem, ceil(H / (64 / G))), one wave per 64 / G
//                  hypotheses, G = 1 or 8 lanes per hypothesis (PnpArgs::G:
//                  8 when the batch alone would leave the chip idle).  Every
//                  lane of a hypothesis draws its sample and solves its P3P
//                  (ba_p3p.h: up to four poses in four register slots), then
//                  counts the inliers of every slot against its share (every
//                  G-th) of the problem's observations, which the wave stages
//                  through LDS in tiles of 32-byte records: lanes of one share
//                  read one address (a broadcast), the G shares 256
//                  contiguous bytes, so there is no bank conflict.  Counts
//                  are integers in registers, summed over the G lanes by
//                  shuffles: the vote does not depend on G.  The wave's
//                  argmax of (count, -h, -slot) is a max-butterfly on one
//                  packed 64-bit key; the winning lane writes one record per
//                  wave.
//   k_pnp_select   one wave per problem: the max over the wave records, the
//                  winner as angle-axis (cam_ransac), the consensus predicate
//                  at cam_ransac through Rodrigues, the per-problem count and
//                  the result record.
//   k_pnp_scan     one wave: exclusive scan of the counts, the dense offsets
//                  launch_pose_batch expects.
//   k_pnp_compact  one wave per problem: the consensus observations in caller
//                  order (ballot + prefix) at the dense offsets.
//   launch_pose_batch on the compacted arrays, unchanged.
//   k_pnp_mask     one wave per problem: REFINE_FAILED handling, the predicate
//                  at cams_out, n_inliers.
// Every value a problem writes depends on its own data alone; there is no
// atomic and no floating-point reduction, so the output is bitwise
// reproducible and independent of the batch.
#include <hip/hip_runtime.h>

#include "ba_kernels.h"
#include "ba_device.h"
#include "ba_p3p.h"
#include "../../include/ba_hip.h"

namespace bahip {

constexpr int kPnpTile = 128;      // observations per LDS tile (4 KiB)
struct PnpPt { double X[3]; float u, v; };
static_assert(sizeof(PnpPt) == 32, "LDS record");
static_assert(kPnpRec >= 13, "wave record: key, R, t");
static_assert(BA_PNP_OK == 0 && BA_PNP_REFINE_FAILED == 3, "status codes");

// The inlier predicate: p = R X + t, q = K p accumulated as k_pose_batch
// accumulates its candidate residual (R row-major here, K col-major)
__device__ __forceinline__ bool pnp_inlier(const double (&R)[9], const double (&t)[3], const double (&Kd)[9], double X0,
                                           double X1, double X2, double u, double v, double thr2) {
  double p[3], q[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) p[i] = R[3 * i] * X0 + R[3 * i + 1] * X1 + R[3 * i + 2] * X2 + t[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) q[i] = p[0] * Kd[i] + p[1] * Kd[3 + i] + p[2] * Kd[6 + i];
  const double r0 = q[0] / q[2] - u, r1 = q[1] / q[2] - v;
  return q[2] > 0.0 && r0 * r0 + r1 * r1 <= thr2;
}

// row-major R of the angle-axis part of cam (the library's Rodrigues)
__device__ __forceinline__ void pnp_cam_R(const double (&cam)[6], double (&R)[9]) {
  double Rc[9];
  angle_axis_to_R(cam, Rc);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) R[3 * r + c] = Rc[3 * c + r];
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long k) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long other = __shfl_xor(k, off, 64);
    k = other > k ? other : k;
  }
  return k;
}
__device__ __forceinline__ int wave_max_i32(int k) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) k = max(k, __shfl_xor(k, off, 64));
  return k;
}

// DBG: ba_pnp_hypotheses, hypotheses [D.h0, D.h0 + D.n) of problem D.problem
template <bool DBG>
__global__ __launch_bounds__(64) void k_pnp_score(PnpArgs A, PnpDebug D) {
  __shared__ PnpPt tile[kPnpTile];
  const int lane = threadIdx.x;
  const int prob = DBG ? D.problem : (int)blockIdx.x;
  const int G = DBG ? 1 : A.G, hpw = 64 / G, sub = lane & (G - 1);   // lanes per hypothesis, hypotheses per wave
  const int idx = (int)blockIdx.y * hpw + lane / G;
  const int h = DBG ? D.h0 + idx : idx;
  const bool live = DBG ? idx < D.n : h < A.H;
  const int nw = (A.H + hpw - 1) / hpw;
  double* rec = DBG ? nullptr : A.rec + ((size_t)prob * nw + blockIdx.y) * kPnpRec;
  const int o0 = A.off[prob], n = A.off[prob + 1] - o0;
  if (!DBG && n < A.n_min) {   // FEW_POINTS (the whole wave)
    if (lane == 0) rec[0] = 0.0;
    return;
  }
  double Kd[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) Kd[k] = (double)A.K[9 * (size_t)prob + k];

  // ---- the lane's hypothesis: up to four poses in slots
  double R[4][9], t[4][3];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
#pragma unroll
    for (int e = 0; e < 9; ++e) R[s][e] = 0.0;
#pragma unroll
    for (int e = 0; e < 3; ++e) t[s][e] = 0.0;
  }
  int smp[3] = {-1, -1, -1}, mask = 0;
  if (live) {
    if (A.use_prior && h == 0) {
      double cam[6];
#pragma unroll
      for (int a = 0; a < 6; ++a) cam[a] = A.prior[6 * (size_t)prob + a];
      pnp_cam_R(cam, R[0]);
#pragma unroll
      for (int e = 0; e < 3; ++e) t[0][e] = cam[3 + e];
      mask = 1;
    } else if (n >= 3) {
      pnp_sample(A.seed, (uint32_t)h, n, smp);
      double Ki[9], X[3][3], f[3][3];
      p3p_inv3(Kd, Ki);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const size_t ob = (size_t)o0 + smp[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) X[i][k] = A.X[3 * ob + k];
        const float2 uv = A.uv[ob];
        p3p_bearing(Ki, (double)uv.x, (double)uv.y, f[i]);
      }
      mask = p3p_solve(X, f, R, t);
    }
  }

  // ---- score every slot against the problem's observations
  int cnt[4] = {0, 0, 0, 0};
  for (int base = 0; base < n; base += kPnpTile) {
    const int m = min(kPnpTile, n - base);
    __syncthreads();
    for (int k = lane; k < m; k += 64) {
      const size_t ob = (size_t)o0 + base + k;
      PnpPt pt;
      pt.X[0] = A.X[3 * ob]; pt.X[1] = A.X[3 * ob + 1]; pt.X[2] = A.X[3 * ob + 2];
      const float2 uv = A.uv[ob];
      pt.u = uv.x; pt.v = uv.y;
      tile[k] = pt;
    }
    __syncthreads();
    for (int k = sub; k < m; k += G) {
      const PnpPt pt = tile[k];
      const double u = (double)pt.u, v = (double)pt.v;
#pragma unroll
      for (int s = 0; s < 4; ++s)
        cnt[s] += (((mask >> s) & 1) && pnp_inlier(R[s], t[s], Kd, pt.X[0], pt.X[1], pt.X[2], u, v, A.thr2)) ? 1 : 0;
    }
  }

  for (int off = 1; off < G; off <<= 1) {
#pragma unroll
    for (int s = 0; s < 4; ++s) cnt[s] += __shfl_xor(cnt[s], off, 64);
  }

  if (DBG) {
    if (live) {
      int j = 0;
#pragma unroll
      for (int k = 0; k < 3; ++k) D.sample[3 * idx + k] = smp[k];
#pragma unroll
      for (int s = 0; s < 4; ++s)
        if ((mask >> s) & 1) {
          double* o = D.Rt + 48 * (size_t)idx + 12 * j;
#pragma unroll
          for (int e = 0; e < 9; ++e) o[e] = R[s][e];
#pragma unroll
          for (int e = 0; e < 3; ++e) o[9 + e] = t[s][e];
          D.count[4 * idx + j] = cnt[s];
          ++j;
        }
      D.n_sol[idx] = j;
      for (; j < 4; ++j) {
        double* o = D.Rt + 48 * (size_t)idx + 12 * j;
        for (int e = 0; e < 12; ++e) o[e] = 0.0;
        D.count[4 * idx + j] = 0;
      }
    }
    return;
  }

  // ---- the lane's best slot (ties: the lower slot), the wave's best lane (ties: the lower h)
  int bs = -1, bc = -1;
#pragma unroll
  for (int s = 0; s < 4; ++s)
    if (((mask >> s) & 1) && cnt[s] > bc) { bc = cnt[s]; bs = s; }
  const unsigned long long key =
      bs >= 0 ? ((unsigned long long)(unsigned)bc << 32) | (unsigned long long)(0x7fffffffu - (unsigned)(4 * h + bs)) : 0ull;
  const unsigned long long kmax = wave_max_u64(key);
  if (kmax == 0ull) {
    if (lane == 0) rec[0] = 0.0;
  } else if (key == kmax && sub == 0) {   // one lane: a nonzero key names its (h, slot)
    rec[0] = __longlong_as_double((long long)kmax);
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (bs == s) {
#pragma unroll
        for (int e = 0; e < 9; ++e) rec[1 + e] = R[s][e];
#pragma unroll
        for (int e = 0; e < 3; ++e) rec[10 + e] = t[s][e];
      }
  }
}

__global__ __launch_bounds__(64) void k_pnp_select(PnpArgs A) {
  const int prob = blockIdx.x, lane = threadIdx.x;
  const int o0 = A.off[prob], n = A.off[prob + 1] - o0;
  const int hpw = 64 / A.G, nw = (A.H + hpw - 1) / hpw;
  int status = BA_PNP_OK, best_h = -1;
  double cam[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) cam[a] = A.use_prior ? A.prior[6 * (size_t)prob + a] : 0.0;
  if (n < A.n_min) {
    status = BA_PNP_FEW_POINTS;
  } else {
    const double* rec = A.rec + (size_t)prob * nw * kPnpRec;
    unsigned long long key = 0ull;
    int wi = -1;
    for (int w = lane; w < nw; w += 64) {
      const unsigned long long k = (unsigned long long)__double_as_longlong(rec[(size_t)w * kPnpRec]);
      if (k > key) { key = k; wi = w; }
    }
    const unsigned long long kmax = wave_max_u64(key);
    const int wsel = wave_max_i32(key == kmax && kmax != 0ull ? wi : -1);
    if (kmax == 0ull || (int)(kmax >> 32) < A.inl_min) {
      status = BA_PNP_NO_MODEL;
    } else {
      best_h = (int)((0x7fffffffu - (unsigned)(kmax & 0xffffffffull)) >> 2);
      if (!(A.use_prior && best_h == 0)) {   // (the prior wins as itself: cam already holds its bits)
        const double* w = rec + (size_t)wsel * kPnpRec;
        double R[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] = w[1 + e];
        p3p_rotation_to_angle_axis(R, cam);
#pragma unroll
        for (int e = 0; e < 3; ++e) cam[3 + e] = w[10 + e];
      }
    }
  }
  // ---- the consensus set: the predicate at cam_ransac through Rodrigues
  int total = 0;
  if (status == BA_PNP_OK) {
    double Kd[9], R[9];
    const double t[3] = {cam[3], cam[4], cam[5]};
#pragma unroll
    for (int k = 0; k < 9; ++k) Kd[k] = (double)A.K[9 * (size_t)prob + k];
    pnp_cam_R(cam, R);
    for (int base = 0; base < n; base += 64) {
      const int ob = base + lane;
      bool in = false;
      if (ob < n) {
        const size_t g = (size_t)o0 + ob;
        const float2 uv = A.uv[g];
        in = pnp_inlier(R, t, Kd, A.X[3 * g], A.X[3 * g + 1], A.X[3 * g + 2], (double)uv.x, (double)uv.y, A.thr2);
        A.cmask[g] = in ? 1 : 0;
      }
      total += __popcll(__ballot(in));
    }
  } else {
    for (int ob = lane; ob < n; ob += 64) A.cmask[(size_t)o0 + ob] = 0;
  }
  if (lane < 6) A.cam_ransac[6 * (size_t)prob + lane] = cam[lane];
  if (lane == 0) {
    A.cnt[prob] = total;
    int* r = A.res + 4 * (size_t)prob;
    r[0] = status; r[1] = 0; r[2] = total; r[3] = best_h;
  }
}

__global__ __launch_bounds__(64) void k_pnp_scan(int n, const int* __restrict__ cnt, int* __restrict__ coff) {
  const int lane = threadIdx.x;
  int carry = 0;
  if (lane == 0) coff[0] = 0;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    int v = i < n ? cnt[i] : 0;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int up = __shfl_up(v, off, 64);
      if (lane >= off) v += up;
    }
    if (i < n) coff[i + 1] = carry + v;
    carry += __shfl(v, 63, 64);
  }
}

__global__ __launch_bounds__(64) void k_pnp_compact(PnpArgs A) {
  const int prob = blockIdx.x, lane = threadIdx.x;
  const int o0 = A.off[prob], n = A.off[prob + 1] - o0;
  size_t dst = (size_t)A.coff[prob];
  for (int base = 0; base < n; base += 64) {
    const int ob = base + lane;
    const size_t g = (size_t)o0 + ob;
    const bool in = ob < n && A.cmask[g] != 0;
    const unsigned long long m = __ballot(in);
    if (in) {
      const size_t d = dst + __popcll(m & ((1ull << lane) - 1ull));
      A.Xc[3 * d] = A.X[3 * g]; A.Xc[3 * d + 1] = A.X[3 * g + 1]; A.Xc[3 * d + 2] = A.X[3 * g + 2];
      A.uvc[d] = A.uv[g];
    }
    dst += __popcll(m);
  }
}

__global__ __launch_bounds__(64) void k_pnp_mask(PnpArgs A) {
  const int prob = blockIdx.x, lane = threadIdx.x;
  const int o0 = A.off[prob], n = A.off[prob + 1] - o0;
  int* r = A.res + 4 * (size_t)prob;
  int status = r[0];
  double* sm = A.summ + 8 * (size_t)prob;
  const bool model = status == BA_PNP_OK;
  bool from_lm = model && A.refine;
  if (from_lm && (int)sm[5] == BA_FAILURE) { status = BA_PNP_REFINE_FAILED; from_lm = false; }
  double cam[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) cam[a] = from_lm ? A.cams_out[6 * (size_t)prob + a] : A.cam_ransac[6 * (size_t)prob + a];
  __syncthreads();   // every lane has read cams_out
  if (!from_lm && lane < 6) A.cams_out[6 * (size_t)prob + lane] = cam[lane];
  if (!model && lane < 8) sm[lane] = 0.0;
  int total = 0;
  if (model) {
    double Kd[9], R[9];
    const double t[3] = {cam[3], cam[4], cam[5]};
#pragma unroll
    for (int k = 0; k < 9; ++k) Kd[k] = (double)A.K[9 * (size_t)prob + k];
    pnp_cam_R(cam, R);
    for (int base = 0; base < n; base += 64) {
      const int ob = base + lane;
      bool in = false;
      if (ob < n) {
        const size_t g = (size_t)o0 + ob;
        const float2 uv = A.uv[g];
        in = pnp_inlier(R, t, Kd, A.X[3 * g], A.X[3 * g + 1], A.X[3 * g + 2], (double)uv.x, (double)uv.y, A.thr2);
        A.inlier[g] = in ? 1 : 0;
      }
      total += __popcll(__ballot(in));
    }
  } else {
    for (int ob = lane; ob < n; ob += 64) A.inlier[(size_t)o0 + ob] = 0;
  }
  if (lane == 0) { r[0] = status; r[1] = total; }
}

void launch_pnp(const PnpArgs& A, const PoseOpts& o, hipStream_t s) {
  if (A.n_prob <= 0) return;
  const int hpw = 64 / A.G, nw = (A.H + hpw - 1) / hpw;
  hipLaunchKernelGGL(k_pnp_score<false>, dim3(A.n_prob, nw), dim3(64), 0, s, A, PnpDebug{});
  hipLaunchKernelGGL(k_pnp_select, dim3(A.n_prob), dim3(64), 0, s, A);
  if (A.refine) {
    hipLaunchKernelGGL(k_pnp_scan, dim3(1), dim3(64), 0, s, A.n_prob, A.cnt, A.coff);
    hipLaunchKernelGGL(k_pnp_compact, dim3(A.n_prob), dim3(64), 0, s, A);
    launch_pose_batch(A.n_prob, A.coff, A.cam_ransac, A.K, A.Xc, A.uvc, A.huber_a, o, A.cams_out, A.summ, s);
  }
  hipLaunchKernelGGL(k_pnp_mask, dim3(A.n_prob), dim3(64), 0, s, A);
}

void launch_pnp_hypotheses(const PnpArgs& A, const PnpDebug& D, hipStream_t s) {
  if (D.n <= 0) return;
  hipLaunchKernelGGL(k_pnp_score<true>, dim3(1, (D.n + 63) / 64), dim3(64), 0, s, A, D);
}

}  // namespace bahip
