// ba_two_view.hip — batched two-view relative pose (gfx950, wave64): E and H
// RANSAC with the whole hypothesis budget scored in parallel, the model
// choice of SfMHelper::recoverPose (SfMHelper.cpp:498-742), the decomposition
// and the positive-depth vote.
//
//   k_tv_solve    grid (pair, ceil(H / 64)), one lane per hypothesis: the
//                 sampler and both minimal solvers (ba_two_view.h); writes E
//                 and H (18 doubles) and their validity per hypothesis.  The
//                 72-double system lives here, not in the scoring kernel.
//   k_tv_score    grid (pair, ceil(H / (64 / G))), one wave per 64 / G
//                 hypotheses, G = 1 or 8 lanes per hypothesis (TvArgs::G, the
//                 pnp_group rule).  A lane holds F = K2^-T E K1^-1, H and H^-1
//                 in registers and counts the inliers of both models over its
//                 share (every G-th) of the pair's matches, which the wave
//                 stages through LDS in tiles of 16-byte records.  Counts are
//                 integers, summed over the G lanes by shuffles; the wave's
//                 argmax per model is a max-butterfly on the packed key
//                 count << 32 | (2^31 - 1 - h); one record of two keys per wave.
//   k_tv_select   one wave per pair: the winners, the essential projection,
//                 the final masks and scores (fixed-order sums), the model
//                 choice, the candidates, the depth vote (ballot counts), the
//                 result record and the inlier mask.
// Five-point mode (TvArgs::e5, BA_TV_E_FIVE_POINT) replaces the E half of the
// first two stages and leaves the H half to the kernels above, instantiated
// without their E work (E8 = false):
//   k_tv_solve5   grid (pair, ceil(H / 64)), one lane per hypothesis.  The
//                 10x20 system does not fit a lane's registers, and its
//                 elimination indexes rows at run time; so the lane's system,
//                 basis, derivative table and breakpoints live in its column
//                 of an LDS array (236 doubles x 64 lanes = 118 KiB, one wave
//                 per CU) and tv_solve_e5 (ba_two_view.h) is the very text a
//                 host program runs.  Writes up to ten E per hypothesis into
//                 slot s * H + h (solution-major) and their number.
//   k_tv_score5   grid (pair, ceil(10 H / (64 / G5))): k_tv_score's E half
//                 over the 10 H slots.  Solutions of high index are rare, so
//                 in the solution-major order whole waves hold no live slot
//                 and leave before the match loop.  Key: count << 32 |
//                 (2^27 - 1 - h) << 4 | (15 - s): the larger count, then the
//                 lower h, then the lower solution.
// Every value a pair writes depends on its own data alone; there is no atomic
// and no floating-point reduction whose order depends on the launch.
#include <hip/hip_runtime.h>

#include "ba_kernels.h"
#include "ba_two_view.h"
#include "../../include/ba_hip.h"

namespace bahip {

constexpr int kTvTile = 256;   // matches per LDS tile (4 KiB)
static_assert(BA_TV_OK == 0 && BA_TV_NO_POSE == 3 && BA_TV_ESSENTIAL == 1 && BA_TV_HOMOGRAPHY == 2, "codes");
static_assert(kTvRes >= 38, "result record");

__device__ __forceinline__ unsigned long long tv_wave_max(unsigned long long k) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long other = __shfl_xor(k, off, 64);
    k = other > k ? other : k;
  }
  return k;
}
// fixed-order sum that every lane receives (a + b == b + a bitwise)
__device__ __forceinline__ double tv_wave_allsum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ void tv_load_K(const float* K, double (&Kd)[9]) {
#pragma unroll
  for (int k = 0; k < 9; ++k) Kd[k] = (double)K[k];
}

// D.n > 0: ba_two_view_hypotheses, hypotheses [D.h0, D.h0 + D.n) of pair D.pair into slots 0 .. D.n-1
// E8 = false (five-point mode): the eight-point E is not formed (zeros, invalid)
template <bool E8>
__global__ __launch_bounds__(64) void k_tv_solve(TvArgs A, TvDebug D) {
  const bool dbg = D.n > 0;
  const int pair = dbg ? D.pair : (int)blockIdx.x;
  const int idx = (int)blockIdx.y * 64 + (int)threadIdx.x;
  const int h = D.h0 + idx;
  if (idx >= (dbg ? D.n : A.H)) return;
  const int o0 = A.off[pair], n = A.off[pair + 1] - o0;
  if (n < A.n_min) return;   // FEW_POINTS: nothing reads the models (n_min >= 8)
  const size_t slot = dbg ? (size_t)idx : (size_t)pair * A.H + h;
  double K1[9], K2[9], Ki1[9], Ki2[9];
  tv_load_K(A.K1 + 9 * (size_t)pair, K1);
  tv_load_K(A.K2 + 9 * (size_t)pair, K2);
  p3p_inv3(K1, Ki1);
  p3p_inv3(K2, Ki2);
  int smp[8];
  tv_sample(A.seed, (uint32_t)h, n, smp);
  double p1[8][2], p2[8][2], q1[4][2], q2[4][2];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float4 m = A.m[(size_t)o0 + smp[i]];
    tv_bearing(Ki1, (double)m.x, (double)m.y, p1[i]);
    tv_bearing(Ki2, (double)m.z, (double)m.w, p2[i]);
    if (i < 4) { q1[i][0] = (double)m.x; q1[i][1] = (double)m.y; q2[i][0] = (double)m.z; q2[i][1] = (double)m.w; }
  }
  double E[9], Hm[9];
  bool ve = false;
  if (E8) ve = tv_solve_e(p1, p2, E);
  const bool vh = tv_solve_h(q1, q2, Hm);
  double* o = A.models + 18 * slot;
#pragma unroll
  for (int e = 0; e < 9; ++e) { o[e] = ve ? E[e] : 0.0; o[9 + e] = vh ? Hm[e] : 0.0; }
  A.valid[2 * slot] = ve ? 1 : 0;
  A.valid[2 * slot + 1] = vh ? 1 : 0;
  if (dbg) {
#pragma unroll
    for (int i = 0; i < 8; ++i) D.sample[8 * (size_t)idx + i] = smp[i];
  }
}

template <bool DBG, bool E8>
__global__ __launch_bounds__(64) void k_tv_score(TvArgs A, TvDebug D) {
  __shared__ float4 tile[kTvTile];
  const int lane = threadIdx.x;
  const int pair = DBG ? D.pair : (int)blockIdx.x;
  const int G = DBG ? 1 : A.G, hpw = 64 / G, sub = lane & (G - 1);
  const int idx = (int)blockIdx.y * hpw + lane / G;
  const int h = DBG ? D.h0 + idx : idx;
  const bool live = idx < (DBG ? D.n : A.H);
  const int nw = (A.H + hpw - 1) / hpw;
  unsigned long long* rec = DBG ? nullptr : A.rec + 2 * ((size_t)pair * nw + blockIdx.y);
  const int o0 = A.off[pair], n = A.off[pair + 1] - o0;
  if (n < A.n_min) {   // FEW_POINTS (the whole wave)
    if (!DBG && lane < 2) rec[lane] = 0ull;
    return;
  }
  // ---- the lane's two models
  double F[9], Hm[9], Hi[9];
  bool ve = false, vh = false;
#pragma unroll
  for (int e = 0; e < 9; ++e) { F[e] = 0.0; Hm[e] = 0.0; Hi[e] = 0.0; }
  if (live) {
    const size_t slot = DBG ? (size_t)idx : (size_t)pair * A.H + h;
    const double* mdl = A.models + 18 * slot;
    ve = E8 && A.valid[2 * slot] != 0;
    vh = A.valid[2 * slot + 1] != 0;
    double K1[9], K2[9], Ki1[9], Ki2[9], E[9];
    tv_load_K(A.K1 + 9 * (size_t)pair, K1);
    tv_load_K(A.K2 + 9 * (size_t)pair, K2);
    p3p_inv3(K1, Ki1);
    p3p_inv3(K2, Ki2);
#pragma unroll
    for (int e = 0; e < 9; ++e) { E[e] = mdl[e]; Hm[e] = mdl[9 + e]; }
    if (E8) tv_fundamental(E, Ki1, Ki2, F);
    if (vh) tv_inv3(Hm, Hi);
  }
  // ---- count both models over the pair's matches
  int ce = 0, ch = 0;
  for (int base = 0; base < n; base += kTvTile) {
    const int m = min(kTvTile, n - base);
    __syncthreads();
    for (int k = lane; k < m; k += 64) tile[k] = A.m[(size_t)o0 + base + k];
    __syncthreads();
    for (int k = sub; k < m; k += G) {
      const float4 r = tile[k];
      const double u1 = (double)r.x, v1 = (double)r.y, u2 = (double)r.z, v2 = (double)r.w;
      if (E8) {
        double d1, d2;
        tv_e_dist2(F, u1, v1, u2, v2, &d1, &d2);
        ce += (d1 <= A.thr2 && d2 <= A.thr2) ? 1 : 0;
      }
      const double e2 = tv_h_err2(Hm, u1, v1, u2, v2), e1 = tv_h_err2(Hi, u2, v2, u1, v1);
      ch += (e1 <= A.thr2 && e2 <= A.thr2) ? 1 : 0;
    }
  }
  for (int off = 1; off < G; off <<= 1) {
    ce += __shfl_xor(ce, off, 64);
    ch += __shfl_xor(ch, off, 64);
  }
  if (!ve) ce = 0;   // an invalid model scores 0
  if (!vh) ch = 0;
  if (DBG) {
    if (live) { D.count[2 * (size_t)idx] = ce; D.count[2 * (size_t)idx + 1] = ch; }
    return;
  }
  // ---- the wave's best hypothesis per model (ties: the lower h); key 0: no valid model
  const unsigned long long hk = (unsigned long long)(0x7fffffffu - (unsigned)h);
  const unsigned long long ke = live && ve ? ((unsigned long long)(unsigned)ce << 32) | hk : 0ull;
  const unsigned long long kh = live && vh ? ((unsigned long long)(unsigned)ch << 32) | hk : 0ull;
  const unsigned long long me = tv_wave_max(ke), mh = tv_wave_max(kh);
  if (lane == 0) { rec[0] = me; rec[1] = mh; }
}

// ---------------------------------------------------------------------------
// five-point mode
// ---------------------------------------------------------------------------
constexpr unsigned kTv5HKey = 0x07ffffffu;   // h < 2^16

// D.n > 0: ba_two_view_hypotheses_e5 (models5 / nsol5 hold D.n hypotheses)
__global__ __launch_bounds__(64) void k_tv_solve5(TvArgs A, TvDebug D) {
  __shared__ double S[kTv5Store * 64];   // element i of lane l at S[64 i + l]
  const bool dbg = D.n > 0;
  const int pair = dbg ? D.pair : (int)blockIdx.x;
  const int idx = (int)blockIdx.y * 64 + (int)threadIdx.x;
  const int h = D.h0 + idx;
  const int Hn = dbg ? D.n : A.H;
  if (idx >= Hn) return;
  const int o0 = A.off[pair], n = A.off[pair + 1] - o0;
  if (n < A.n_min) return;   // FEW_POINTS: nothing reads the solutions
  double K1[9], K2[9], Ki1[9], Ki2[9];
  tv_load_K(A.K1 + 9 * (size_t)pair, K1);
  tv_load_K(A.K2 + 9 * (size_t)pair, K2);
  p3p_inv3(K1, Ki1);
  p3p_inv3(K2, Ki2);
  int smp[8];
  tv_sample(A.seed, (uint32_t)h, n, smp);
  double b1[5][2], b2[5][2];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const float4 m = A.m[(size_t)o0 + smp[i]];
    tv_bearing(Ki1, (double)m.x, (double)m.y, b1[i]);
    tv_bearing(Ki2, (double)m.z, (double)m.w, b2[i]);
  }
  const size_t base = dbg ? 0 : (size_t)pair * A.H;
  double* out = A.models5 + 9 * (10 * base + (size_t)idx);
  A.nsol5[base + idx] = tv_solve_e5(b1, b2, S + threadIdx.x, 64, out, 9 * (size_t)Hn);
  if (dbg) {
#pragma unroll
    for (int i = 0; i < 8; ++i) D.sample[8 * (size_t)idx + i] = smp[i];
  }
}

template <bool DBG>
__global__ __launch_bounds__(64) void k_tv_score5(TvArgs A, TvDebug D) {
  __shared__ float4 tile[kTvTile];
  const int lane = threadIdx.x;
  const int pair = DBG ? D.pair : (int)blockIdx.x;
  const int G = DBG ? 1 : A.G5, hpw = 64 / G, sub = lane & (G - 1);
  const int Hn = DBG ? D.n : A.H;
  const int q = (int)blockIdx.y * hpw + lane / G;   // slot s * Hn + i
  const bool inr = q < 10 * Hn;
  const int sol = inr ? q / Hn : 0, idx = inr ? q - sol * Hn : 0;
  const int h = DBG ? D.h0 + idx : idx;
  const int nw = (10 * A.H + hpw - 1) / hpw;
  unsigned long long* rec = DBG ? nullptr : A.rec5 + ((size_t)pair * nw + blockIdx.y);
  const int o0 = A.off[pair], n = A.off[pair + 1] - o0;
  const size_t base = DBG ? 0 : (size_t)pair * A.H;
  const bool live = n >= A.n_min && inr && sol < A.nsol5[base + idx];
  if (__ballot(live) == 0ull) {   // FEW_POINTS, or no solution in any of the wave's slots
    if (!DBG && lane == 0) rec[0] = 0ull;
    if (DBG && inr) D.count5[10 * (size_t)idx + sol] = 0;
    return;
  }
  double F[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) F[e] = 0.0;
  if (live) {
    const double* mdl = A.models5 + 9 * (10 * base + (size_t)q);
    double K1[9], K2[9], Ki1[9], Ki2[9], E[9];
    tv_load_K(A.K1 + 9 * (size_t)pair, K1);
    tv_load_K(A.K2 + 9 * (size_t)pair, K2);
    p3p_inv3(K1, Ki1);
    p3p_inv3(K2, Ki2);
#pragma unroll
    for (int e = 0; e < 9; ++e) E[e] = mdl[e];
    tv_fundamental(E, Ki1, Ki2, F);
  }
  int ce = 0;
  for (int b0 = 0; b0 < n; b0 += kTvTile) {
    const int m = min(kTvTile, n - b0);
    __syncthreads();
    for (int k = lane; k < m; k += 64) tile[k] = A.m[(size_t)o0 + b0 + k];
    __syncthreads();
    for (int k = sub; k < m; k += G) {
      const float4 r = tile[k];
      double d1, d2;
      tv_e_dist2(F, (double)r.x, (double)r.y, (double)r.z, (double)r.w, &d1, &d2);
      ce += (d1 <= A.thr2 && d2 <= A.thr2) ? 1 : 0;
    }
  }
  for (int off = 1; off < G; off <<= 1) ce += __shfl_xor(ce, off, 64);
  if (!live) ce = 0;
  if (DBG) {
    if (inr) D.count5[10 * (size_t)idx + sol] = ce;
    return;
  }
  // ties: the lower h, then the lower solution; key 0: no solution
  const unsigned long long lo = ((unsigned long long)(kTv5HKey - (unsigned)h) << 4) | (unsigned long long)(15 - sol);
  const unsigned long long me = tv_wave_max(live ? ((unsigned long long)(unsigned)ce << 32) | lo : 0ull);
  if (lane == 0) rec[0] = me;
}

__global__ __launch_bounds__(64) void k_tv_select(TvArgs A) {
  const int pair = blockIdx.x, lane = threadIdx.x;
  const int o0 = A.off[pair], n = A.off[pair + 1] - o0;
  const int hpw = 64 / A.G, nw = (A.H + hpw - 1) / hpw;
  double* res = A.res + (size_t)kTvRes * pair;
  uint8_t* inl = A.inlier + o0;
  int status = BA_TV_OK;
  unsigned long long ke = 0ull, kh = 0ull;
  if (n < A.n_min) {
    status = BA_TV_FEW_POINTS;
  } else {
    const unsigned long long* rec = A.rec + 2 * (size_t)pair * nw;
    for (int w = lane; w < nw; w += 64) {
      const unsigned long long a = rec[2 * (size_t)w], b = rec[2 * (size_t)w + 1];
      ke = a > ke ? a : ke;
      kh = b > kh ? b : kh;
    }
    if (A.e5) {   // the E key comes from the five-point slots
      const int hpw5 = 64 / A.G5, nw5 = (10 * A.H + hpw5 - 1) / hpw5;
      const unsigned long long* rec5 = A.rec5 + (size_t)pair * nw5;
      ke = 0ull;
      for (int w = lane; w < nw5; w += 64) {
        const unsigned long long a = rec5[w];
        ke = a > ke ? a : ke;
      }
    }
    ke = tv_wave_max(ke);
    kh = tv_wave_max(kh);
  }
  const int votes_e = (int)(ke >> 32), votes_h = (int)(kh >> 32);
  const int sol_e = A.e5 && ke ? 15 - (int)(ke & 15ull) : 0;
  const int he = A.e5 ? (ke ? (int)(kTv5HKey - (unsigned)((ke & 0xffffffffull) >> 4)) : -1)
                      : ke ? (int)(0x7fffffffu - (unsigned)(ke & 0xffffffffull)) : -1;
  const int hh = kh ? (int)(0x7fffffffu - (unsigned)(kh & 0xffffffffull)) : -1;
  bool avail_e = ke != 0ull && votes_e >= A.inl_min, avail_h = kh != 0ull && votes_h >= A.inl_min;

  // ---- the winners (every lane computes the same): projected E, F, H, H^-1
  double K1[9], K2[9], Ki1[9], Ki2[9];
  double Ep[9], F[9], Hm[9], Hi[9], U[3][3], V[3][3];
#pragma unroll
  for (int e = 0; e < 9; ++e) { Ep[e] = 0.0; F[e] = 0.0; Hm[e] = 0.0; Hi[e] = 0.0; }
  if (status == BA_TV_OK) {
    tv_load_K(A.K1 + 9 * (size_t)pair, K1);
    tv_load_K(A.K2 + 9 * (size_t)pair, K2);
    p3p_inv3(K1, Ki1);
    p3p_inv3(K2, Ki2);
    if (avail_e) {
      const double* mdl = A.e5 ? A.models5 + 9 * ((10 * (size_t)pair + sol_e) * A.H + he) : A.models + 18 * ((size_t)pair * A.H + he);
      double E[9];
#pragma unroll
      for (int e = 0; e < 9; ++e) E[e] = mdl[e];
      avail_e = tv_project_e(E, Ep, U, V);
      tv_fundamental(Ep, Ki1, Ki2, F);
    }
    if (avail_h) {
      const double* mdl = A.models + 18 * ((size_t)pair * A.H + hh) + 9;
#pragma unroll
      for (int e = 0; e < 9; ++e) Hm[e] = mdl[e];
      tv_inv3(Hm, Hi);
    }
  }

  // ---- final masks (bit 0: E, bit 1: H, parked in `inlier`) and scores
  double se = 0.0, sh = 0.0;
  int ne = 0, nh = 0;
  for (int base = 0; base < n; base += 64) {
    const int k = base + lane;
    bool ie = false, ih = false;
    if (k < n && status == BA_TV_OK) {
      const float4 r = A.m[(size_t)o0 + k];
      const double u1 = (double)r.x, v1 = (double)r.y, u2 = (double)r.z, v2 = (double)r.w;
      if (avail_e) {
        double d1, d2;
        tv_e_dist2(F, u1, v1, u2, v2, &d1, &d2);
        ie = d1 <= A.thr2 && d2 <= A.thr2 && d1 <= kTvChi1 && d2 <= kTvChi1;
        if (ie) se += (kTvChi2 - d1) + (kTvChi2 - d2);
      }
      if (avail_h) {
        const double e2 = tv_h_err2(Hm, u1, v1, u2, v2), e1 = tv_h_err2(Hi, u2, v2, u1, v1);
        ih = e1 <= A.thr2 && e2 <= A.thr2 && e1 <= kTvChi2 && e2 <= kTvChi2;
        if (ih) sh += (kTvChi2 - e1) + (kTvChi2 - e2);
      }
    }
    if (k < n) inl[k] = (uint8_t)((ie ? 1 : 0) | (ih ? 2 : 0));
    ne += __popcll(__ballot(ie));
    nh += __popcll(__ballot(ih));
  }
  se = tv_wave_allsum(se);
  sh = tv_wave_allsum(sh);

  // ---- the model
  int model = 0;
  if (status == BA_TV_OK) {
    model = A.model != BA_TV_AUTO ? A.model : ((double)(float)(sh / (sh + se)) > A.h_ratio ? BA_TV_HOMOGRAPHY : BA_TV_ESSENTIAL);
    if (!(model == BA_TV_ESSENTIAL ? avail_e : avail_h)) { status = BA_TV_NO_MODEL; model = 0; }
  }

  // ---- candidates and the depth vote
  int best = -1, n_good = 0, n_second = 0;
  double best_nz = 0.0;
  double R[9], t[3], nrm[3] = {0.0, 0.0, 0.0};
  TvHDecomp HD;
  if (status == BA_TV_OK) {
    int ncand = 4;
    if (model == BA_TV_HOMOGRAPHY) {
      double Am[9], M[9];
      // A = K2^-1 H K1 (K col-major)
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) M[3 * k + j] = Hm[3 * k] * K1[3 * j] + Hm[3 * k + 1] * K1[3 * j + 1] + Hm[3 * k + 2] * K1[3 * j + 2];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Am[3 * i + j] = Ki2[i] * M[j] + Ki2[3 + i] * M[3 + j] + Ki2[6 + i] * M[6 + j];
      ncand = tv_h_decompose(Am, &HD) ? 8 : 0;
    }
    const int bit = model == BA_TV_HOMOGRAPHY ? 2 : 1;
    for (int c = 0; c < ncand; ++c) {
      if (model == BA_TV_HOMOGRAPHY) tv_h_candidate(&HD, c, R, t, nrm);
      else tv_e_candidate(U, V, c, R, t);
      bool fin = true;
#pragma unroll
      for (int e = 0; e < 9; ++e) fin = fin && fabs(R[e]) < HUGE_VAL;
      int cnt = 0;
      for (int base = 0; base < n; base += 64) {
        const int k = base + lane;
        bool good = false;
        if (k < n && fin && (inl[k] & bit)) {
          const float4 r = A.m[(size_t)o0 + k];
          double b1[2], b2[2];
          tv_bearing(Ki1, (double)r.x, (double)r.y, b1);
          tv_bearing(Ki2, (double)r.z, (double)r.w, b2);
          good = tv_depth_good(R, t, b1, b2);
        }
        cnt += __popcll(__ballot(good));
      }
      const double nz = fabs(nrm[2]);
      if (best < 0 || cnt > n_good || (cnt == n_good && nz > best_nz)) {
        if (best >= 0) n_second = n_good;
        best = c; n_good = cnt; best_nz = nz;
      } else if (cnt > n_second) {
        n_second = cnt;
      }
    }
    if (best < 0 || n_good < A.good_min) status = BA_TV_NO_POSE;
  }

  // ---- the pose, the mask, the record
  double cam[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  nrm[0] = nrm[1] = nrm[2] = 0.0;
  if (status == BA_TV_OK) {
    if (model == BA_TV_HOMOGRAPHY) tv_h_candidate(&HD, best, R, t, nrm);
    else tv_e_candidate(U, V, best, R, t);
    p3p_rotation_to_angle_axis(R, cam);
    cam[3] = t[0]; cam[4] = t[1]; cam[5] = t[2];
  }
  const int bit = model == BA_TV_HOMOGRAPHY ? 2 : 1;
  for (int k = lane; k < n; k += 64) inl[k] = (status == BA_TV_OK && (inl[k] & bit)) ? 1 : 0;
  if (lane == 0) {
    const bool ok = status == BA_TV_OK, rep = ok || status == BA_TV_NO_POSE;   // NO_POSE keeps its diagnostics
    res[0] = status; res[1] = rep ? model : 0;
    res[2] = ok ? (model == BA_TV_HOMOGRAPHY ? nh : ne) : 0;
    res[3] = rep ? n_good : 0; res[4] = rep ? n_second : 0;
    res[5] = ok && avail_e ? he : -1; res[6] = ok && avail_h ? hh : -1;   // (an unavailable model: -1, zeros, its vote)
    res[7] = rep ? votes_e : 0; res[8] = rep ? votes_h : 0;
    res[9] = rep ? se : 0.0; res[10] = rep ? sh : 0.0;
#pragma unroll
    for (int e = 0; e < 9; ++e) { res[11 + e] = rep ? Ep[e] : 0.0; res[20 + e] = rep ? Hm[e] : 0.0; }
#pragma unroll
    for (int e = 0; e < 6; ++e) res[29 + e] = cam[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) res[35 + e] = nrm[e];
    res[38] = ok && avail_e ? sol_e : 0;
  }
}

void launch_two_view(const TvArgs& A, hipStream_t s) {
  if (A.n_pair <= 0) return;
  const int hpw = 64 / A.G, nw = (A.H + hpw - 1) / hpw;
  if (A.e5) {
    const int hpw5 = 64 / A.G5, nw5 = (10 * A.H + hpw5 - 1) / hpw5;
    hipLaunchKernelGGL(k_tv_solve<false>, dim3(A.n_pair, (A.H + 63) / 64), dim3(64), 0, s, A, TvDebug{});
    hipLaunchKernelGGL(k_tv_solve5, dim3(A.n_pair, (A.H + 63) / 64), dim3(64), 0, s, A, TvDebug{});
    hipLaunchKernelGGL((k_tv_score<false, false>), dim3(A.n_pair, nw), dim3(64), 0, s, A, TvDebug{});
    hipLaunchKernelGGL(k_tv_score5<false>, dim3(A.n_pair, nw5), dim3(64), 0, s, A, TvDebug{});
  } else {
    hipLaunchKernelGGL(k_tv_solve<true>, dim3(A.n_pair, (A.H + 63) / 64), dim3(64), 0, s, A, TvDebug{});
    hipLaunchKernelGGL((k_tv_score<false, true>), dim3(A.n_pair, nw), dim3(64), 0, s, A, TvDebug{});
  }
  hipLaunchKernelGGL(k_tv_select, dim3(A.n_pair), dim3(64), 0, s, A);
}

void launch_two_view_hypotheses(const TvArgs& A, const TvDebug& D, hipStream_t s) {
  if (D.n <= 0) return;
  hipLaunchKernelGGL(k_tv_solve<true>, dim3(1, (D.n + 63) / 64), dim3(64), 0, s, A, D);
  hipLaunchKernelGGL((k_tv_score<true, true>), dim3(1, (D.n + 63) / 64), dim3(64), 0, s, A, D);
}

void launch_two_view_hypotheses_e5(const TvArgs& A, const TvDebug& D, hipStream_t s) {
  if (D.n <= 0) return;
  hipLaunchKernelGGL(k_tv_solve5, dim3(1, (D.n + 63) / 64), dim3(64), 0, s, A, D);
  hipLaunchKernelGGL(k_tv_score5<true>, dim3(1, (10 * D.n + 63) / 64), dim3(64), 0, s, A, D);
}

}  // namespace bahip
