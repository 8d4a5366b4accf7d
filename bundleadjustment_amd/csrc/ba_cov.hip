// ba_cov.hip — covariances from the dense Schur factor (ba_covariance,
// ba_covariance_ex): what ceres::Covariance gives with its defaults, blocks of
// (J^T J)^-1 for any pair of cameras and points, and the leverages
// J_o (J^T J)^-1 J_o^T of observations.
//
// Input is the state a DENSE_SCHUR factorisation of the undamped reduced
// system leaves behind (ba_chol.hip): the off-diagonal 64 x 64 tiles L_ij of
// the Cholesky factor in W.Lf, and the inverses V_k = L_kk^-1 of its diagonal
// tiles in W.Vbuf.  With X = L^-1 (lower block triangular):
//   X_kk = V_k,   X_ik = -V_i sum_{j=k}^{i-1} L_ij X_jk   (i > k)
//   Sigma_scaled = S_scaled^-1 = X^T X
// X is kept transposed, U = X^T = L^-T (upper block triangular, row-major):
// block row k of U is block column k of X, so a column's chain writes and
// re-reads one contiguous band, and both products take their operands as
// plain row-major tiles (sum_c A[a][c] B[b][c], the form of mfma_xyT_64):
//   U_ki   = -(sum_j U_kj L_ij^T) V_i^T
//   Sig_IJ = sum_{k >= I} U_Ik U_Jk^T     (I >= J)
// Every dependency is inside one workgroup (a block column's chain) or a
// launch boundary; every sum runs in a fixed order (j, k increasing; the MFMA
// contraction order of ba_chol.h), so the output is reproducible bit for bit.
//
// Buffers: U overwrites W.S (the working matrix the factorisation has
// consumed), Sigma_scaled overwrites the lower block triangle of W.Lf once U
// is complete.  The caller zeroes W.S afterwards (its state before the first
// step); W.Lf is rewritten by every factorisation.
#include "ba_chol.h"
#include "ba_reduce.h"
#include "ba_schur.h"
#include "ba_cov_point.h"

namespace bahip {

// Block column k of X = L^-1, as block row k of U, by one workgroup.
__global__ __launch_bounds__(256) void k_cov_linv(const double* __restrict__ Lf, const double* __restrict__ Vbuf,
                                                  double* U, int ld, int n) {
  __shared__ double S0[CB][LDP];
  __shared__ double S1[CB][LDP];
  const int T = (n + CB - 1) / CB;
  const int k = blockIdx.x;   // (the longest chains are dispatched first)
  const int kc = k * CB, kb = min(CB, n - kc);
  const size_t lds = (size_t)ld;
  // U_kk = V_k^T (V_k lower triangular; what the factorisation left above its
  // diagonal is not defined)
  {
    const double* Vk = Vbuf + (size_t)k * CB * CB;
    for (int e = ctid(); e < CB * CB; e += 256) {
      const int b = e / CB, a = e % CB;
      if (b < kb && a < kb) U[(size_t)(kc + b) * lds + kc + a] = b <= a ? Vk[(size_t)a * CB + b] : 0.0;
    }
  }
  __syncthreads();
  for (int i = k + 1; i < T; ++i) {
    const int ic = i * CB;
    // G[b][a] = sum_{j=k}^{i-1} sum_c U_kj[b][c] L_ij[a][c]   (= (L X)_ik^T)
    d4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[a][b] = d4{0.0, 0.0, 0.0, 0.0};
    TileRegs tu = tile_fetch(U, lds, kc, kc, n, n);
    TileRegs tl = tile_fetch(Lf, lds, ic, kc, n, n);   // (rows < n: the rhs row of Lf is not part of L)
    for (int j = k; j < i; ++j) {
      tile_put(S0, tu);
      tile_put(S1, tl);
      __syncthreads();
      if (j + 1 < i) {   // the next pair of tiles arrives under this pair's MFMAs
        tu = tile_fetch(U, lds, kc, (j + 1) * CB, n, n);
        tl = tile_fetch(Lf, lds, ic, (j + 1) * CB, n, n);
      }
      mfma_xyT_64_add(S0, S1, acc);
      __syncthreads();
    }
    const TileRegs tv = tile_fetch<true>(Vbuf + (size_t)i * CB * CB, CB, 0, 0, CB, CB);
    acc_to_lds(S0, acc, 0);
    tile_put(S1, tv);
    __syncthreads();
    // U_ki[b][a] = -sum_c G[b][c] V_i[a][c]
    mfma_xyT_64(S0, S1, acc);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          int rr, cc;
          acc_pos(a, b, g, &rr, &cc);
          if (rr < kb && ic + cc < n) U[(size_t)(kc + rr) * lds + ic + cc] = -acc[a][b][g];
        }
    // the next round of this chain reads U_ki (same workgroup: the barrier
    // orders the stores before the loads) and reuses S0, S1
    __syncthreads();
  }
}

// Sigma_scaled tile (I, J), I >= J: sum over k >= I, increasing, of U_Ik U_Jk^T.
__global__ __launch_bounds__(256) void k_cov_xtx(const double* __restrict__ U, double* __restrict__ Sg, int ld, int n) {
  const int I = blockIdx.y, J = blockIdx.x;
  if (J > I) return;
  __shared__ double S0[CB][LDP];
  __shared__ double S1[CB][LDP];
  const int T = (n + CB - 1) / CB;
  const size_t lds = (size_t)ld;
  const int r0 = I * CB, c0 = J * CB;
  d4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = d4{0.0, 0.0, 0.0, 0.0};
  TileRegs ta = tile_fetch(U, lds, r0, r0, n, n);
  TileRegs tb = tile_fetch(U, lds, c0, r0, n, n);
  for (int k = I; k < T; ++k) {
    tile_put(S0, ta);
    tile_put(S1, tb);
    __syncthreads();
    if (k + 1 < T) {
      ta = tile_fetch(U, lds, r0, (k + 1) * CB, n, n);
      tb = tile_fetch(U, lds, c0, (k + 1) * CB, n, n);
    }
    mfma_xyT_64_add(S0, S1, acc);
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        int rr, cc;
        acc_pos(a, b, g, &rr, &cc);
        if (r0 + rr < n && c0 + cc < n) Sg[(size_t)(r0 + rr) * lds + c0 + cc] = acc[a][b][g];
      }
}

// entry (r, c) of the symmetric Sigma_scaled, stored in its lower block tiles
__device__ __forceinline__ double cov_sym(const double* __restrict__ Sg, size_t ld, int r, int c) {
  return r >= c ? Sg[(size_t)r * ld + c] : Sg[(size_t)c * ld + r];
}

// Requested camera blocks: Cov(cam_i, cam_j) = s_i Sigma_scaled[i, j] s_j
// (6 x 6, row-major).  pairs: compact variable-camera indices, or -1 for a
// constant camera (an all-zero block, as in Ceres).
__global__ __launch_bounds__(256) void k_cov_cam_blocks(const double* __restrict__ Sg, int ld,
                                                        const double* __restrict__ scale_c,
                                                        const int2* __restrict__ pairs, int npairs,
                                                        double* __restrict__ out) {
  const size_t total = (size_t)npairs * 36;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const int q = (int)(e / 36), t = (int)(e % 36), i = t / 6, j = t % 6;
    const int2 p = pairs[q];
    double v = 0.0;
    if (p.x >= 0 && p.y >= 0) {
      const int r = 6 * p.x + i, c = 6 * p.y + j;
      v = scale_c[r] * cov_sym(Sg, (size_t)ld, r, c) * scale_c[c];
    }
    out[e] = v;
  }
}

// W_o = E_o L_p^-T (6 x 3, scaled columns) of sorted observation o by
// variable camera v, from either record form of the step (step_w_storage)
__device__ __forceinline__ void cov_load_w(const DevProblem& P, const double* __restrict__ Wrec, bool compact,
                                           const double* __restrict__ scale_c, int o, int v, double (&w)[18]) {
  if (!compact) {
    load_w18(Wrec, (size_t)o, w);
    return;
  }
  const WcRaw r = wc_fetch(Wrec, o);
  WcCam m;
  m.load(P, scale_c, v);
  double c0[6], c1[6];
  wc_rows(r, m, c0, c1);
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int k = 0; k < 3; ++k) w[a * 3 + k] = c0[a] * r.r[9 + k] + c1[a] * r.r[12 + k];
}

// t = sum_{a in obs(p), b in obs(q)} W_a^T Sigma_scaled[c(a), c(b)] W_b (3 x 3,
// row-major) by one wave; the sum is in lane 0.  Lane l takes the pairs (a, b)
// with index l, l + 64, ... of obs(p) x obs(q) (increasing), then a fixed
// reduction over the wave.  Observations by constant cameras have no camera
// block and are skipped.
__device__ __forceinline__ void cov_pair_sum(const DevProblem& P, const double* __restrict__ Sg,
                                             const double* __restrict__ Wrec, int compact,
                                             const double* __restrict__ scale_c, int p, int q, int lane,
                                             double (&t)[9]) {
  const size_t ld = (size_t)P.ld;
  const int o0 = P.pt_off[p], m = P.pt_off[p + 1] - o0;
  const int q0 = P.pt_off[q], mq = P.pt_off[q + 1] - q0;
#pragma unroll
  for (int k = 0; k < 9; ++k) t[k] = 0.0;
  for (int e = lane; e < m * mq; e += 64) {
    const int a = e / mq, b = e - a * mq;
    const int va = P.obs_vc[o0 + a], vb = P.obs_vc[q0 + b];
    if (va < 0 || vb < 0) continue;   // an observation by a constant camera: no camera block
    double wa[18], wb[18];
    cov_load_w(P, Wrec, compact != 0, scale_c, o0 + a, va, wa);
    cov_load_w(P, Wrec, compact != 0, scale_c, q0 + b, vb, wb);
    // Y = Sigma[va, vb] W_b (6 x 3), then t += W_a^T Y
    double y[18];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const double g = cov_sym(Sg, ld, 6 * va + i, 6 * vb + j);
        s0 += g * wb[j * 3];
        s1 += g * wb[j * 3 + 1];
        s2 += g * wb[j * 3 + 2];
      }
      y[i * 3] = s0; y[i * 3 + 1] = s1; y[i * 3 + 2] = s2;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) s += wa[i * 3 + r] * y[i * 3 + c];
        t[r * 3 + c] += s;
      }
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) t[k] = wave_sum(t[k]);
}

// Requested points, one per wave.  In scaled columns, with L_p the point's
// 3 x 3 factor and W_a = E_a L_p^-T the records of its observations by
// variable cameras,
//   Sigma_pp = L_p^-T (I + sum_{a, b} W_a^T Sigma_scaled[c(a), c(b)] W_b) L_p^-1
// and the result is s_p Sigma_pp s_p (cov_pair_sum, cov_point_finish).  A
// constant point gives zeros.
__global__ __launch_bounds__(256) void k_cov_points(DevProblem P, const double* __restrict__ Sg,
                                                    const double* __restrict__ Wrec, int compact,
                                                    const double* __restrict__ scale_c,
                                                    const double* __restrict__ scale_p,
                                                    const double* __restrict__ Linv, const int* __restrict__ pts,
                                                    int npts, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wv = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), nwv = (int)((gridDim.x * blockDim.x) >> 6);
  for (int q = wv; q < npts; q += nwv) {
    const int p = pts[q];
    double* dst = out + 9 * (size_t)q;
    if (!P.pt_var[p]) {   // (uniform in the wave)
      if (lane < 9) dst[lane] = 0.0;
      continue;
    }
    double t[9];
    cov_pair_sum(P, Sg, Wrec, compact, scale_c, p, p, lane, t);
    if (lane == 0) {
      CovPt cp;
      cp.load(Linv, scale_p, p, (size_t)P.np);
      double r[9];
      cov_point_finish(t, true, cp, cp, r);
#pragma unroll
      for (int k = 0; k < 9; ++k) dst[k] = r[k];
    }
  }
}

// Requested point pairs, one per wave: Cov(p, q) = s_p L_p^-T (delta_pq I +
// sum_{a in obs(p), b in obs(q)} W_a^T Sigma_scaled[c(a), c(b)] W_b) L_q^-1 s_q.
// The block is formed for (min, max) and stored transposed for p > q, so
// Cov(p, q)^T and Cov(q, p) are the same bits; p == q is k_cov_points' sum and
// finish, bit for bit.  A constant point gives zeros.
__global__ __launch_bounds__(256) void k_cov_pt_pairs(DevProblem P, const double* __restrict__ Sg,
                                                      const double* __restrict__ Wrec, int compact,
                                                      const double* __restrict__ scale_c,
                                                      const double* __restrict__ scale_p,
                                                      const double* __restrict__ Linv, const int2* __restrict__ pq,
                                                      int npairs, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wv = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), nwv = (int)((gridDim.x * blockDim.x) >> 6);
  for (int x = wv; x < npairs; x += nwv) {
    const int2 r = pq[x];
    const int p = min(r.x, r.y), q = max(r.x, r.y);
    double* dst = out + 9 * (size_t)x;
    if (!P.pt_var[p] || !P.pt_var[q]) {   // (uniform in the wave)
      if (lane < 9) dst[lane] = 0.0;
      continue;
    }
    double t[9];
    cov_pair_sum(P, Sg, Wrec, compact, scale_c, p, q, lane, t);
    if (lane == 0) {
      CovPt cp, cq;
      cp.load(Linv, scale_p, p, (size_t)P.np);
      cq.load(Linv, scale_p, q, (size_t)P.np);
      double v[9];
      cov_point_finish(t, p == q, cp, cq, v);
      const bool tr = r.x > r.y;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) dst[i * 3 + j] = tr ? v[j * 3 + i] : v[i * 3 + j];
    }
  }
}

// Requested (camera, point) cross blocks, one per wave:
//   Cov(cam v, p) = s_v (-(sum_{a in obs(p)} Sigma_scaled[v, c(a)] W_a) L_p^-1) s_p   (6 x 3)
// cp: {compact variable-camera index or -1 (constant camera), point}.  Lane l
// takes row l & 7 (< 6) of the terms a = l >> 3, (l >> 3) + 8, ... in
// increasing order, then a fixed xor reduction over the eight lanes of a row;
// the row's lane applies L_p^-1, the scales and the sign.  A constant camera
// or point gives zeros.
__global__ __launch_bounds__(256) void k_cov_cam_pt(DevProblem P, const double* __restrict__ Sg,
                                                    const double* __restrict__ Wrec, int compact,
                                                    const double* __restrict__ scale_c,
                                                    const double* __restrict__ scale_p,
                                                    const double* __restrict__ Linv, const int2* __restrict__ cp,
                                                    int nreq, double* __restrict__ out) {
  const int lane = threadIdx.x & 63, row = lane & 7, a0 = lane >> 3;
  const int wv = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), nwv = (int)((gridDim.x * blockDim.x) >> 6);
  const size_t ld = (size_t)P.ld;
  for (int x = wv; x < nreq; x += nwv) {
    const int v = cp[x].x, p = cp[x].y;
    double* dst = out + 18 * (size_t)x;
    if (v < 0 || !P.pt_var[p]) {   // (uniform in the wave)
      if (lane < 18) dst[lane] = 0.0;
      continue;
    }
    const int o0 = P.pt_off[p], m = P.pt_off[p + 1] - o0;
    double y0 = 0.0, y1 = 0.0, y2 = 0.0;
    if (row < 6)
      for (int a = a0; a < m; a += 8) {
        const int va = P.obs_vc[o0 + a];
        if (va < 0) continue;
        double w[18];
        cov_load_w(P, Wrec, compact != 0, scale_c, o0 + a, va, w);
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          const double g = cov_sym(Sg, ld, 6 * v + row, 6 * va + j);
          y0 += g * w[j * 3];
          y1 += g * w[j * 3 + 1];
          y2 += g * w[j * 3 + 2];
        }
      }
#pragma unroll
    for (int off = 8; off < 64; off <<= 1) {
      y0 += __shfl_xor(y0, off, 64);
      y1 += __shfl_xor(y1, off, 64);
      y2 += __shfl_xor(y2, off, 64);
    }
    if (lane < 6) {
      CovPt c;
      c.load(Linv, scale_p, p, (size_t)P.np);
      const double y[3] = {y0, y1, y2};
      const double sc = scale_c[(size_t)v * 6 + row];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        double s = 0.0;
#pragma unroll
        for (int l = k; l < 3; ++l) s += y[l] * c.li[l][k];
        dst[row * 3 + k] = sc * -s * c.s[k];
      }
    }
  }
}

// Leverages h_o = J_o Sigma J_o^T (2 x 2) of every observation of the listed
// points, one point per workgroup of one wave.  With J_o = [Jc | Jp] of the
// JR records (JA doubles per camera half), jc = Jc s_c, jp = Jp s_p and
//   Y_a = sum_b Sigma_scaled[c(a), c(b)] W_b   (6 x 3, b over obs(p)),
//   h_a = jc Sigma_scaled[c(a), c(a)] jc^T - (X + X^T) + Jp Sigma_pp Jp^T,
//   X = jc Y_a L_p^-1 jp^T,   Sigma_pp = s_p L_p^-T (I + sum_a W_a^T Y_a) L_p^-1 s_p.
// Lane l takes row l & 7 (< 6) of observation 8 g + (l >> 3) in round g.  The
// W_b are staged in LDS 64 at a time (once per point up to 64 observations,
// else once per round and chunk) and every lane sums its row of Y_a over b in
// increasing order, so neither the number of observations of a point nor
// duplicates are bounded; a lane's row of W_a comes from the staged chunk.  A round's products are reduced over the eight
// lanes of an observation (xor 1, 2, 4) and, for sum_a W_a^T Y_a, over the
// wave; the rounds add up in increasing order.  The first pass stores the
// terms that need no Sigma_pp into hbuf [hoff[x] + a][4] (hoff: the running
// count of observations of the listed points); the second
// pass (same lane, so program order) adds Jp Sigma_pp Jp^T.  A constant
// camera or point contributes nothing.
constexpr int kLevLd = 19;   // LDS row stride of a staged W record
__global__ __launch_bounds__(64) void k_cov_leverage(DevProblem P, const double* __restrict__ Sg,
                                                     const double* __restrict__ Wrec, int compact,
                                                     const double* __restrict__ scale_c,
                                                     const double* __restrict__ scale_p,
                                                     const double* __restrict__ Linv, const double* __restrict__ JR,
                                                     int JA, const int* __restrict__ pts,
                                                     const int* __restrict__ hoff, int npts, double* hbuf) {
  __shared__ double Wst[64 * kLevLd];
  __shared__ int vst[64];
  const int lane = threadIdx.x, row = lane & 7, al = lane >> 3;
  const size_t ld = (size_t)P.ld;
  const double* JB = JR + (size_t)JA * P.no;
  for (int x = blockIdx.x; x < npts; x += gridDim.x) {
    const int p = pts[x];
    const bool pvar = P.pt_var[p] != 0;
    const int o0 = P.pt_off[p], m = P.pt_off[p + 1] - o0;
    double* hp = hbuf + 4 * (size_t)hoff[x];   // this point's observations, in sorted order
    CovPt c;
    double jps[3] = {1.0, 1.0, 1.0};
    if (pvar) {
      c.load(Linv, scale_p, p, (size_t)P.np);
      jps[0] = c.s[0]; jps[1] = c.s[1]; jps[2] = c.s[2];
    }
    double t[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) t[k] = 0.0;
    // W_b, b in [b0, b0 + nb), into LDS (between two barriers)
    auto stage = [&](int b0, int nb) {
      __syncthreads();   // (the last chunk's readers are done)
      if (lane < nb) {
        const int vb = P.obs_vc[o0 + b0 + lane];
        vst[lane] = vb;
        if (vb >= 0) {
          double w[18];
          cov_load_w(P, Wrec, compact != 0, scale_c, o0 + b0 + lane, vb, w);
#pragma unroll
          for (int k = 0; k < 18; ++k) Wst[lane * kLevLd + k] = w[k];
        }
      }
      __syncthreads();
    };
    const bool one = m <= 64;   // a single chunk: staged once for all rounds
    if (pvar && one) stage(0, m);
    for (int a8 = 0; a8 < m; a8 += 8) {
      const int a = a8 + al;
      const int va = (a < m && row < 6) ? P.obs_vc[o0 + a] : -1;
      double y[3] = {0.0, 0.0, 0.0}, wr[3] = {0.0, 0.0, 0.0};
      if (pvar)
        for (int b0 = 0; b0 < m; b0 += 64) {
          const int nb = min(64, m - b0);
          if (!one) stage(b0, nb);
          if (va < 0) continue;
          if (a8 >= b0 && a8 < b0 + 64) {   // (a round lies inside one chunk) row `row` of W_a
#pragma unroll
            for (int k = 0; k < 3; ++k) wr[k] = Wst[(a - b0) * kLevLd + row * 3 + k];
          }
          for (int b = 0; b < nb; ++b) {
            const int vb = vst[b];
            if (vb < 0) continue;
            const double* w = &Wst[b * kLevLd];
#pragma unroll
            for (int j = 0; j < 6; ++j) {
              const double g = cov_sym(Sg, ld, 6 * va + row, 6 * vb + j);
              y[0] += g * w[j * 3];
              y[1] += g * w[j * 3 + 1];
              y[2] += g * w[j * 3 + 2];
            }
          }
        }
      // this lane's terms: row `row` of W_a and of jc; 4 + 6 + 9 products
      double cc[4] = {0.0, 0.0, 0.0, 0.0}, gy[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, tt[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) tt[k] = 0.0;
      if (va >= 0) {
        const double* ja = JR + (size_t)(o0 + a) * JA;
        double jc[2][6];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int j = 0; j < 6; ++j) jc[r][j] = ja[r * 6 + j] * scale_c[(size_t)va * 6 + j];
        double z0 = 0.0, z1 = 0.0, j0 = 0.0, j1 = 0.0;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          const double g = cov_sym(Sg, ld, 6 * va + row, 6 * va + j);
          z0 += g * jc[0][j];
          z1 += g * jc[1][j];
          if (j == row) { j0 = jc[0][j]; j1 = jc[1][j]; }
        }
        cc[0] = j0 * z0; cc[1] = j0 * z1; cc[2] = j1 * z0; cc[3] = j1 * z1;
        if (pvar) {
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            gy[k] = j0 * y[k];
            gy[3 + k] = j1 * y[k];
#pragma unroll
            for (int l = 0; l < 3; ++l) tt[k * 3 + l] = wr[k] * y[l];
          }
        }
      }
#pragma unroll
      for (int off = 1; off < 8; off <<= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) cc[k] += __shfl_xor(cc[k], off, 64);
#pragma unroll
        for (int k = 0; k < 6; ++k) gy[k] += __shfl_xor(gy[k], off, 64);
      }
      if (pvar) {
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          double s = tt[k];
#pragma unroll
          for (int off = 1; off < 64; off <<= 1) s += __shfl_xor(s, off, 64);
          t[k] += s;
        }
      }
      if (row == 0 && a < m) {
        double h00 = cc[0], h01 = 0.5 * (cc[1] + cc[2]), h11 = cc[3];
        if (pvar) {
          // X = (jc Y_a) L_p^-1 jp^T
          const double* jb = JB + (size_t)(o0 + a) * 8;
          double gl[2][3], X[2][2];
#pragma unroll
          for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              double s = 0.0;
#pragma unroll
              for (int l = k; l < 3; ++l) s += gy[r * 3 + l] * c.li[l][k];
              gl[r][k] = s;
            }
#pragma unroll
          for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
              double s = 0.0;
#pragma unroll
              for (int k = 0; k < 3; ++k) s += gl[r][k] * (jb[q * 3 + k] * jps[k]);
              X[r][q] = s;
            }
          h00 -= X[0][0] + X[0][0];
          h01 -= X[0][1] + X[1][0];
          h11 -= X[1][1] + X[1][1];
        }
        double* h = hp + 4 * (size_t)a;
        h[0] = h00; h[1] = h01; h[2] = h01; h[3] = h11;
      }
    }
    if (!pvar) continue;
    double spp[9];
    cov_point_finish(t, true, c, c, spp);   // (every lane holds the same t)
    for (int a8 = 0; a8 < m; a8 += 8) {
      const int a = a8 + al;
      if (row != 0 || a >= m) continue;
      const double* jb = JB + (size_t)(o0 + a) * 8;
      double js[2][3];
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          double s = 0.0;
#pragma unroll
          for (int l = 0; l < 3; ++l) s += jb[r * 3 + l] * spp[l * 3 + k];
          js[r][k] = s;
        }
      double q[2][2];
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          double s = 0.0;
#pragma unroll
          for (int k = 0; k < 3; ++k) s += js[r][k] * jb[u * 3 + k];
          q[r][u] = s;
        }
      double* h = hp + 4 * (size_t)a;
      const double h01 = h[1] + 0.5 * (q[0][1] + q[1][0]);
      h[0] += q[0][0]; h[1] = h01; h[2] = h01; h[3] += q[1][1];
    }
  }
}

// out[x] = hbuf[idx[x]] (2 x 2): the request's order, repeats included
__global__ __launch_bounds__(256) void k_cov_lev_gather(const double* __restrict__ hbuf, const int* __restrict__ idx,
                                                        int n, double* __restrict__ out) {
  const size_t total = 4 * (size_t)n;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x)
    out[e] = hbuf[4 * (size_t)idx[e >> 2] + (e & 3)];
}

// U = L^-T into W.S, then Sigma_scaled into the lower block tiles of W.Lf
void launch_cov_inverse(const DevProblem& P, const DevWork& W, hipStream_t s) {
  const int n = P.n;
  if (n == 0) return;
  const int T = (n + CB - 1) / CB;
  hipLaunchKernelGGL(k_cov_linv, dim3(T), dim3(256), 0, s, (const double*)W.Lf, (const double*)W.Vbuf, W.S, P.ld, n);
  hipLaunchKernelGGL(k_cov_xtx, dim3(T, T), dim3(256), 0, s, (const double*)W.S, W.Lf, P.ld, n);
}

void launch_cov_cam_blocks(const DevProblem& P, const DevWork& W, const int2* pairs, int npairs, double* out,
                           hipStream_t s) {
  if (npairs == 0) return;
  hipLaunchKernelGGL(k_cov_cam_blocks, dim3(grid_for(std::min(npairs, 1 << 24) * 36)), dim3(256), 0, s,
                     (const double*)W.Lf, P.ld, (const double*)W.scale_c, pairs, npairs, out);
}

void launch_cov_points(const DevProblem& P, const DevWork& W, const int* pts, int npts, double* out, hipStream_t s) {
  if (npts == 0) return;
  const int grid = std::min(kMaxBlocks, (npts + 3) / 4);   // 4 waves per workgroup, one point per wave and round
  hipLaunchKernelGGL(k_cov_points, dim3(grid), dim3(256), 0, s, P, (const double*)W.Lf, (const double*)W.W,
                     W.wcompact ? 1 : 0, (const double*)W.scale_c, (const double*)W.scale_p, (const double*)W.Linv, pts,
                     npts, out);
}

void launch_cov_pt_pairs(const DevProblem& P, const DevWork& W, const int2* pq, int npairs, double* out,
                         hipStream_t s) {
  if (npairs == 0) return;
  const int grid = std::min(kMaxBlocks, (npairs + 3) / 4);
  hipLaunchKernelGGL(k_cov_pt_pairs, dim3(grid), dim3(256), 0, s, P, (const double*)W.Lf, (const double*)W.W,
                     W.wcompact ? 1 : 0, (const double*)W.scale_c, (const double*)W.scale_p, (const double*)W.Linv, pq,
                     npairs, out);
}

void launch_cov_cam_pt(const DevProblem& P, const DevWork& W, const int2* cp, int nreq, double* out, hipStream_t s) {
  if (nreq == 0) return;
  const int grid = std::min(kMaxBlocks, (nreq + 3) / 4);
  hipLaunchKernelGGL(k_cov_cam_pt, dim3(grid), dim3(256), 0, s, P, (const double*)W.Lf, (const double*)W.W,
                     W.wcompact ? 1 : 0, (const double*)W.scale_c, (const double*)W.scale_p, (const double*)W.Linv, cp,
                     nreq, out);
}

void launch_cov_leverage(const DevProblem& P, const DevWork& W, const int* pts, const int* hoff, int npts,
                         double* hbuf, const int* idx, int nlev, double* out, hipStream_t s) {
  if (nlev == 0) return;
  if (npts > 0)
    hipLaunchKernelGGL(k_cov_leverage, dim3(std::min(npts, 1 << 20)), dim3(64), 0, s, P, (const double*)W.Lf,
                       (const double*)W.W, W.wcompact ? 1 : 0, (const double*)W.scale_c, (const double*)W.scale_p,
                       (const double*)W.Linv, (const double*)W.JR, jr_ja_host(P.nc), pts, hoff, npts, hbuf);
  hipLaunchKernelGGL(k_cov_lev_gather, dim3(grid_for(std::min(nlev, 1 << 24) * 4)), dim3(256), 0, s,
                     (const double*)hbuf, idx, nlev, out);
}

}  // namespace bahip
