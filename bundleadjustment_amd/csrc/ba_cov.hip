// ba_cov.hip — marginal covariances from the dense Schur factor
// (ba_covariance): what ceres::Covariance gives with its defaults, (J^T J)^-1
// restricted to camera x camera and point x point blocks.
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

// Requested points, one per wave.  In scaled columns, with L_p the point's
// 3 x 3 factor and W_a = E_a L_p^-T the records of its observations by
// variable cameras,
//   Sigma_pp = L_p^-T (I + sum_{a, b} W_a^T Sigma_scaled[c(a), c(b)] W_b) L_p^-1
// and the result is s_p Sigma_pp s_p.  Lane l takes the pairs (a, b) with
// index l, l + 64, ... of the point's observation list squared (increasing),
// then a fixed xor reduction over the wave.  A constant point gives zeros.
__global__ __launch_bounds__(256) void k_cov_points(DevProblem P, const double* __restrict__ Sg,
                                                    const double* __restrict__ Wrec, int compact,
                                                    const double* __restrict__ scale_c,
                                                    const double* __restrict__ scale_p,
                                                    const double* __restrict__ Linv, const int* __restrict__ pts,
                                                    int npts, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wv = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), nwv = (int)((gridDim.x * blockDim.x) >> 6);
  const size_t ld = (size_t)P.ld, np = (size_t)P.np;
  for (int q = wv; q < npts; q += nwv) {
    const int p = pts[q];
    double* dst = out + 9 * (size_t)q;
    if (!P.pt_var[p]) {   // (uniform in the wave)
      if (lane < 9) dst[lane] = 0.0;
      continue;
    }
    const int o0 = P.pt_off[p], m = P.pt_off[p + 1] - o0;
    double t[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) t[k] = 0.0;
    for (int e = lane; e < m * m; e += 64) {
      const int a = e / m, b = e - a * m;
      const int va = P.obs_vc[o0 + a], vb = P.obs_vc[o0 + b];
      if (va < 0 || vb < 0) continue;   // an observation by a constant camera: no camera block
      double wa[18], wb[18];
      cov_load_w(P, Wrec, compact != 0, scale_c, o0 + a, va, wa);
      cov_load_w(P, Wrec, compact != 0, scale_c, o0 + b, vb, wb);
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
    if (lane == 0) {
      // M = I + t; R = Li^T M Li with Li = L_p^-1 (lower); out = s R s
      const double li[3][3] = {{Linv[p], 0.0, 0.0},
                               {Linv[np + p], Linv[2 * np + p], 0.0},
                               {Linv[3 * np + p], Linv[4 * np + p], Linv[5 * np + p]}};
      const double s[3] = {scale_p[p], scale_p[np + p], scale_p[2 * np + p]};
      double M[3][3], ML[3][3];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) M[r][c] = (r == c ? 1.0 : 0.0) + t[r * 3 + c];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          double x = 0.0;
#pragma unroll
          for (int l = c; l < 3; ++l) x += M[r][l] * li[l][c];
          ML[r][c] = x;
        }
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          double x = 0.0;
#pragma unroll
          for (int l = r; l < 3; ++l) x += li[l][r] * ML[l][c];
          dst[r * 3 + c] = s[r] * x * s[c];
        }
    }
  }
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

}  // namespace bahip
