// ba_icp.hip — the kernels of ba_icp (include/ba_hip.h; the rules are
// ba_icp.h's, shared with the host).  One round of the loop is four launches
// on one stream, enqueued max_iterations times with no host sync, then once
// more for the fitness:
//
//   k_icp_nn_grid   one lane per source point of a GRID pair, in the cell
//                   order of the plan's permutation: applies the last step as
//                   it loads cur and stores it back, then walks the target's
//                   grid ring by ring (icp_grid_nn).  A lane whose walk passes
//                   the ring limit appends its point to the pair's list.
//   k_icp_nn_brute  target tiles in LDS, every lane sweeps them: whole BRUTE
//                   pairs, and the listed points of GRID pairs.
//   k_icp_partials  per block of 256 points the kIcpSums fp64 sums (fixed
//                   order: shuffle tree, then the waves in index order).
//   k_icp_step      per pair: the block partials in index order (one lane per
//                   quantity), then one lane runs icp_step: the SVD, the
//                   update of final, the convergence rules.
//
// Every kernel reads its pair's state first and returns when the pair has
// left the loop (round < max_iterations: state != NOT_CONVERGED; the fitness
// round: not converged).  The only atomic is the integer count of the list,
// and each listed point writes its own result, so the order does not matter.
#include <hip/hip_runtime.h>

#include "ba_icp.h"
#include "ba_kernels.h"
#include "ba_reduce.h"

namespace bahip {

static_assert(sizeof(IcpPt) == 16 && sizeof(IcpGrid) == 48 && sizeof(IcpPair) == 32, "tables");
static_assert(kIcpThreads == 256 && kIcpTile % kIcpThreads == 0, "launch shape");

// does pair's state let this round run?
__device__ __forceinline__ bool icp_live(const IcpArgs& A, const IcpState& S, int round) {
  return round >= A.rules.max_iter ? S.converged != 0 : S.state == BA_ICP_NOT_CONVERGED;
}

// cur of point i of the pair, with the pending step applied and stored back
__device__ __forceinline__ void icp_load_cur(const IcpArgs& A, const IcpState& S, size_t slot, int round, float& x, float& y,
                                             float& z) {
  float* c = A.cur + 3 * slot;
  x = c[0]; y = c[1]; z = c[2];
  if (S.apply_at == round) {
    icp_apply(S.M, S.t, x, y, z);
    c[0] = x; c[1] = y; c[2] = z;
  }
}

__global__ __launch_bounds__(kIcpThreads) void k_icp_nn_grid(IcpArgs A, int round, float gate) {
  const IcpPair P = A.pair[blockIdx.y];
  if (P.route != BA_ICP_ROUTE_GRID) return;
  IcpState& S = A.st[blockIdx.y];
  if (!icp_live(A, S, round)) return;
  const int t = (int)(blockIdx.x * kIcpThreads + threadIdx.x);
  if (t >= P.ns) return;
  const int i = A.perm[P.soff + t];
  const size_t slot = (size_t)P.soff + i;
  float x, y, z;
  icp_load_cur(A, S, slot, round, x, y, z);
  const IcpGrid G = A.grid[P.grid];
  uint64_t best;
  if (icp_grid_nn(G, A.cell_start + G.cell0, A.sorted + P.t0, x, y, z, gate, A.max_ring, best)) {
    icp_record(best, gate, A.idx[slot], A.d2[slot]);
  } else {
    A.flag[P.soff + atomicAdd(&S.n_flag, 1)] = i;
  }
}

__global__ __launch_bounds__(kIcpThreads) void k_icp_nn_brute(IcpArgs A, int round, float gate) {
  __shared__ IcpPt tile[kIcpTile];
  const IcpPair P = A.pair[blockIdx.y];
  IcpState& S = A.st[blockIdx.y];
  if (!icp_live(A, S, round)) return;
  const bool whole = P.route == BA_ICP_ROUTE_BRUTE;
  const int nq = whole ? P.ns : S.n_flag;
  if ((int)(blockIdx.x * kIcpThreads) >= nq) return;   // the whole block
  const int t = (int)(blockIdx.x * kIcpThreads + threadIdx.x);
  const bool active = t < nq;
  size_t slot = 0;
  float x = 0.0f, y = 0.0f, z = 0.0f;
  if (active) {
    slot = (size_t)P.soff + (whole ? t : A.flag[P.soff + t]);
    if (whole) icp_load_cur(A, S, slot, round, x, y, z);
    else { x = A.cur[3 * slot]; y = A.cur[3 * slot + 1]; z = A.cur[3 * slot + 2]; }   // k_icp_nn_grid stored it
  }
  const IcpPt* tgt = A.sorted + P.t0;
  uint64_t best = kMatchNone;
  for (int base = 0; base < P.nt; base += kIcpTile) {
    const int m = min(kIcpTile, P.nt - base);
    __syncthreads();
    for (int e = threadIdx.x; e < m; e += kIcpThreads) tile[e] = tgt[base + e];
    __syncthreads();
    if (active) icp_scan(tile, 0, m, x, y, z, best);
  }
  if (active) icp_record(best, gate, A.idx[slot], A.d2[slot]);
}

__global__ __launch_bounds__(kIcpThreads) void k_icp_partials(IcpArgs A, int round) {
  __shared__ double lds[kIcpSums * 16];
  const IcpPair P = A.pair[blockIdx.y];
  if ((int)(blockIdx.x * kIcpThreads) >= P.ns) return;
  if (!icp_live(A, A.st[blockIdx.y], round)) return;
  const int i = (int)(blockIdx.x * kIcpThreads + threadIdx.x);
  double v[kIcpSums];
#pragma unroll
  for (int k = 0; k < kIcpSums; ++k) v[k] = 0.0;
  const size_t slot = (size_t)P.soff + i;
  const int j = i < P.ns ? A.idx[slot] : -1;
  if (j >= 0) {
    const float* c0 = A.grid[P.grid].c0;
    const float* q = A.xyz + 3 * ((size_t)P.t0 + j);
    const float* c = A.cur + 3 * slot;
    double a[3], b[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) { a[r] = (double)c[r] - (double)c0[r]; b[r] = (double)q[r] - (double)c0[r]; }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      v[r] = a[r]; v[3 + r] = b[r];
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) v[6 + 3 * r + cc] = b[r] * a[cc];
    }
    v[15] = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
    v[16] = (double)A.d2[slot];
    v[17] = 1.0;
  }
  double out[kIcpSums];
  block_sum<kIcpSums>(v, lds, out);
  if (threadIdx.x == 0) {
    double* dst = A.part + (size_t)kIcpSums * (P.boff + blockIdx.x);
#pragma unroll
    for (int k = 0; k < kIcpSums; ++k) dst[k] = out[k];
  }
}

__global__ __launch_bounds__(64) void k_icp_step(IcpArgs A, int round) {
  __shared__ double s[kIcpSums];
  const int p = blockIdx.x;
  const IcpPair P = A.pair[p];
  IcpState& S = A.st[p];
  if (!icp_live(A, S, round)) return;
  const int nb = (P.ns + kIcpThreads - 1) / kIcpThreads;
  if (threadIdx.x < kIcpSums) {
    const double* src = A.part + (size_t)kIcpSums * P.boff + threadIdx.x;
    double acc = 0.0;
    for (int b = 0; b < nb; ++b) acc += src[(size_t)kIcpSums * b];
    s[threadIdx.x] = acc;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  S.n_flag = 0;
  if (round >= A.rules.max_iter) {
    S.fitness = s[17] > 0.0 ? s[16] / s[17] : DBL_MAX;
    return;
  }
  IcpState T = S;
  const int it0 = T.iterations;
  const double mse = icp_step(T, s, A.grid[P.grid].c0, A.rules, round);
  if (T.iterations > it0) A.mse[(size_t)p * A.rules.max_iter + it0] = mse;
  S = T;
}

void launch_icp_round(const IcpArgs& A, int round, bool nn_only, hipStream_t s) {
  if (A.n_pair <= 0 || A.max_ns <= 0) return;
  const dim3 g((A.max_ns + kIcpThreads - 1) / kIcpThreads, A.n_pair);
  const float gate = round >= A.rules.max_iter ? A.fit_range : A.max_d2;
  k_icp_nn_grid<<<g, kIcpThreads, 0, s>>>(A, round, gate);
  k_icp_nn_brute<<<g, kIcpThreads, 0, s>>>(A, round, gate);
  if (nn_only) return;
  k_icp_partials<<<g, kIcpThreads, 0, s>>>(A, round);
  k_icp_step<<<A.n_pair, 64, 0, s>>>(A, round);
}

}  // namespace bahip
