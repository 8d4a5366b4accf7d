// ba_icp.h — the pinned rules of ba_icp (include/ba_hip.h), written once for
// the device (ba_icp.hip) and for host programs (host/ba_batch_pack.hpp's
// plan, tests/cpp/icp_host.cpp): plain C++ behind __host__ __device__.
//
// Distance and order.  d2 = ((dx*dx + dy*dy) + dz*dz) in float with
// ba_map_points.h's primitives (every operation rounded on its own).  d2 >= 0,
// so the key bits(d2) << 32 | j orders by distance, then by target index; the
// nearest neighbour is the key minimum over the target, whatever the order in
// which the target is walked.
//
// Grid.  A target set is binned into n[0] x n[1] x n[2] cubic cells of edge h
// over its bounding box, cell (i, j, k) at (k n[1] + j) n[0] + i, so an x-run
// of cells is one contiguous run of the cell-sorted points.  A coordinate's
// cell is icp_cell: floor((x - mn) / h) in double, clamped to the grid; the
// same function bins the target (icp_plan) and places a query.
//
// Exactness of the ring walk (icp_grid_nn).  After the rings 0 .. r around the
// query's clamped cell q, every unvisited target point lies in a cell whose
// index differs from q's by more than r on some axis.  On an axis where cells
// below q - r exist, such a point has x < mn + (q - r) h up to the rounding of
// icp_cell, so it is at least px - (mn + (q - r) h) away; likewise above
// q + r.  B is the smallest of these up to six face distances, formed in
// double.  Roundings: icp_cell's quotient and the face are off by a few
// 2^-53 relative; the float d2 of a point at true distance D is at least
// D^2 (1 - 5 * 2^-24) (one rounding per difference, product and sum), unless
// it underflows.  The walk therefore stops only when
//   best_d2 < Bs^2,  Bs = B - kIcpMargin (|B| + h),  Bs^2 > kIcpTiny,
// which leaves a relative margin of 2e-6 against 3e-7 and keeps underflow out:
// every unvisited point then has a strictly larger d2 and so a larger key.
// The same bound against the gate: when gate < Bs^2 no unvisited point can be
// kept, and the best visited key decides.  If no face is left the whole grid
// was visited.  A query whose walk passes max_ring is not answered here: the
// caller sweeps the whole target for it.
#pragma once
#include <float.h>

#include "ba_map_points.h"
#include "ba_two_view.h"

#define BA_ICP_HD BA_MATCH_HD

namespace bahip {

constexpr double kIcpMargin = 1e-6, kIcpTiny = 1e-30;
// Rings before a query goes to the sweep.  Reasoned, not measured: a ring of an empty region costs two
// cell_start loads per row of cells, (2r + 1)^2 rows, against a sweep of the whole target.
constexpr int kIcpMaxRing = 12;
constexpr int kIcpThreads = 256;
constexpr int kIcpTile = 1024;            // target points per LDS tile of the sweep (16 KiB)
constexpr int kIcpCellPts = 8;            // points per cell the plan aims at
constexpr int kIcpMaxCells = 1 << 22;     // cell cap of one grid (16 MiB of cell_start)
// AUTO sweeps targets up to this size.  Measured: for one pair
// of 2k source points the kernels of the two routes cross near 512 target
// points, but a GRID pair costs the host about 0.09 ms of grid and permutation
// build, so 256 pairs of 2k x 2k take 31.0 ms under GRID against 10.7 ms under
// the sweep; the threshold stays where such batches keep the sweep.
constexpr int kIcpBruteMax = 2048;
constexpr int kIcpSums = 18;              // sum a (3), sum b (3), sum b a^T (9), sum |a|^2, sum d2, count

struct IcpPt { float x, y, z; int32_t j; };   // a target point in cell order with its index in the set

struct IcpGrid {
  float mn[3], h;      // the box's low corner, the cell edge
  int32_t n[3];        // cells per axis
  int32_t cell0;       // first entry of this grid's cell_start run (n[0] n[1] n[2] + 1 entries, set-local point ranks)
  float c0[3];         // centre of the bounding box
  int32_t pad;
};

// One pair as the kernels read it
struct IcpPair {
  int32_t s0, ns;      // the source set: first point in xyz, points
  int32_t t0, nt;      // the target set (also its run of the cell-sorted points)
  int32_t grid;        // the target's grid
  int32_t route;       // BA_ICP_ROUTE_GRID or BA_ICP_ROUTE_BRUTE
  int32_t soff;        // first slot of the per-pair arrays (sum of ns of the pairs before)
  int32_t boff;        // first block partial (sum of the blocks of the pairs before)
};

// The loop state of one pair (device; downloaded at the end)
struct IcpState {
  float fin[16];       // final, row-major
  float M[9], t[3];    // the last step, row-major (c R and t)
  int32_t state, converged, iterations, n_corr;
  int32_t apply_at;    // the round whose correspondence pass applies (M, t) as it loads cur; -1: none
  int32_t n_flag;      // queries of this round left to the sweep
  double prev, fitness;
};

BA_ICP_HD inline float icp_d2(float px, float py, float pz, float qx, float qy, float qz) {
  const float dx = mp_sub(px, qx), dy = mp_sub(py, qy), dz = mp_sub(pz, qz);
  return mp_add(mp_add(mp_mul(dx, dx), mp_mul(dy, dy)), mp_mul(dz, dz));
}
BA_ICP_HD inline float icp_gate(float max_corr_dist) { return mp_mul(max_corr_dist, max_corr_dist); }

// cur <- M cur + t
BA_ICP_HD inline void icp_apply(const float* M, const float* t, float& x, float& y, float& z) {
  const float a = mp_add(mp_add(mp_add(mp_mul(M[0], x), mp_mul(M[1], y)), mp_mul(M[2], z)), t[0]);
  const float b = mp_add(mp_add(mp_add(mp_mul(M[3], x), mp_mul(M[4], y)), mp_mul(M[5], z)), t[1]);
  const float c = mp_add(mp_add(mp_add(mp_mul(M[6], x), mp_mul(M[7], y)), mp_mul(M[8], z)), t[2]);
  x = a; y = b; z = c;
}

BA_ICP_HD inline int icp_cell(float x, float mn, float h, int n) {
  const double v = ((double)x - (double)mn) / (double)h;
  return v >= (double)n ? n - 1 : (v > 0.0 ? (int)v : 0);
}

BA_ICP_HD inline void icp_scan(const IcpPt* pts, int p0, int p1, float px, float py, float pz, uint64_t& best) {
  for (int p = p0; p < p1; ++p) {
    const IcpPt q = pts[p];
    const uint64_t key = match_key(icp_d2(px, py, pz, q.x, q.y, q.z), (uint32_t)q.j);
    best = key < best ? key : best;
  }
}

// The key minimum over the target through the grid: true, or false when the
// walk passed max_ring undecided.  cs: the grid's cell_start run; pts: the
// set's cell-sorted points; gate: no point with d2 > gate is wanted.
BA_ICP_HD inline bool icp_grid_nn(const IcpGrid& G, const int32_t* cs, const IcpPt* pts, float px, float py, float pz,
                                  float gate, int max_ring, uint64_t& best) {
  const int n0 = G.n[0], n1 = G.n[1], n2 = G.n[2];
  const int qi = icp_cell(px, G.mn[0], G.h, n0), qj = icp_cell(py, G.mn[1], G.h, n1), qk = icp_cell(pz, G.mn[2], G.h, n2);
  const double h = (double)G.h;
  best = kMatchNone;
  for (int r = 0;; ++r) {
    const int i0 = qi - r > 0 ? qi - r : 0, i1 = qi + r < n0 - 1 ? qi + r : n0 - 1;
    const int j0 = qj - r > 0 ? qj - r : 0, j1 = qj + r < n1 - 1 ? qj + r : n1 - 1;
    const int k0 = qk - r > 0 ? qk - r : 0, k1 = qk + r < n2 - 1 ? qk + r : n2 - 1;
    for (int k = k0; k <= k1; ++k)
      for (int j = j0; j <= j1; ++j) {
        const int row = (k * n1 + j) * n0;
        if (k == qk - r || k == qk + r || j == qj - r || j == qj + r) {
          icp_scan(pts, cs[row + i0], cs[row + i1 + 1], px, py, pz, best);
        } else {
          if (qi - r >= 0) icp_scan(pts, cs[row + qi - r], cs[row + qi - r + 1], px, py, pz, best);
          if (qi + r < n0) icp_scan(pts, cs[row + qi + r], cs[row + qi + r + 1], px, py, pz, best);
        }
      }
    double B = DBL_MAX;
    bool open = false;
    if (qi - r > 0) { open = true; B = fmin(B, (double)px - ((double)G.mn[0] + (double)(qi - r) * h)); }
    if (qi + r < n0 - 1) { open = true; B = fmin(B, ((double)G.mn[0] + (double)(qi + r + 1) * h) - (double)px); }
    if (qj - r > 0) { open = true; B = fmin(B, (double)py - ((double)G.mn[1] + (double)(qj - r) * h)); }
    if (qj + r < n1 - 1) { open = true; B = fmin(B, ((double)G.mn[1] + (double)(qj + r + 1) * h) - (double)py); }
    if (qk - r > 0) { open = true; B = fmin(B, (double)pz - ((double)G.mn[2] + (double)(qk - r) * h)); }
    if (qk + r < n2 - 1) { open = true; B = fmin(B, ((double)G.mn[2] + (double)(qk + r + 1) * h) - (double)pz); }
    if (!open) return true;
    const double Bs = B - kIcpMargin * (fabs(B) + h);
    if (Bs > 0.0 && Bs * Bs > kIcpTiny) {
      if (best != kMatchNone && (double)match_float((uint32_t)(best >> 32)) < Bs * Bs) return true;
      if ((double)gate < Bs * Bs) return true;
    }
    if (r >= max_ring) return false;
  }
}
// (the else branch runs from r >= 1 only: at r == 0 the one row of the block is
// on the shell, so its two single-cell scans never name the same cell)

// The result record of one query from its key and the gate
BA_ICP_HD inline void icp_record(uint64_t best, float gate, int32_t& idx, float& d2) {
  const float v = match_float((uint32_t)(best >> 32));
  if (best != kMatchNone && v <= gate) { idx = (int32_t)(uint32_t)best; d2 = v; }
  else { idx = -1; d2 = match_float(0x7f800000u); }
}

// ---- the step: s = the kIcpSums sums over the kept points about c0
// (a = cur - c0, b = target - c0).  M = c R (row-major) and t as floats.
BA_ICP_HD inline void icp_estimate(const double* s, const float* c0, int with_scale, float* M, float* t) {
  const double n = s[17];
  double ma[3], mb[3], H[9];
  for (int r = 0; r < 3; ++r) { ma[r] = s[r] / n; mb[r] = s[3 + r] / n; }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) H[3 * r + c] = s[6 + 3 * r + c] - n * mb[r] * ma[c];
  double U[3][3], V[3][3], sv[3];
  const double sgn = tv_svd3(H, U, sv, V);
  double R[9];
  bool ok = true;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      R[3 * r + c] = U[0][r] * V[0][c] + U[1][r] * V[1][c] + U[2][r] * V[2][c];
      ok = ok && fabs(R[3 * r + c]) <= 2.0;   // false for a NaN
    }
  double sc = 1.0;
  if (!ok) {
    for (int e = 0; e < 9; ++e) R[e] = e % 4 == 0 ? 1.0 : 0.0;
  } else if (with_scale) {
    const double var = s[15] - n * (ma[0] * ma[0] + ma[1] * ma[1] + ma[2] * ma[2]);
    const double c = (sv[0] + sv[1] + sgn * sv[2]) / var;
    if (c > 0.0 && c < DBL_MAX) sc = c;
  }
  for (int e = 0; e < 9; ++e) M[e] = (float)(sc * R[e]);
  for (int r = 0; r < 3; ++r) {
    const double a0 = (double)c0[0] + ma[0], a1 = (double)c0[1] + ma[1], a2 = (double)c0[2] + ma[2];
    t[r] = (float)(((double)c0[r] + mb[r]) - sc * (R[3 * r] * a0 + R[3 * r + 1] * a1 + R[3 * r + 2] * a2));
  }
}

// final <- T final, T = [M t; 0 0 0 1]
BA_ICP_HD inline void icp_compose(const float* M, const float* t, float* fin) {
  float o[12];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j)
      o[4 * i + j] = mp_add(mp_add(mp_add(mp_mul(M[3 * i], fin[j]), mp_mul(M[3 * i + 1], fin[4 + j])),
                                   mp_mul(M[3 * i + 2], fin[8 + j])), mp_mul(t[i], fin[12 + j]));
  for (int e = 0; e < 12; ++e) fin[e] = o[e];
}

struct IcpRules { int max_iter, min_corr, with_scale; double abs_eps, rel_eps, tr_eps; };

// One iteration's decisions from the sums; S.state is NOT_CONVERGED on entry.
// round: the launch round, for apply_at.  Returns the recorded mse (0: none).
BA_ICP_HD inline double icp_step(IcpState& S, const double* s, const float* c0, const IcpRules& o, int round) {
  const int n = (int)s[17];
  S.n_corr = n;
  if (n < o.min_corr) {
    S.state = BA_ICP_NO_CORRESPONDENCES; S.converged = 0; S.apply_at = -1;
    return 0.0;
  }
  icp_estimate(s, c0, o.with_scale, S.M, S.t);
  icp_compose(S.M, S.t, S.fin);
  S.iterations += 1;
  const double mse = s[16] / (double)n;
  const double cos_angle = 0.5 * (((double)S.M[0] + (double)S.M[4] + (double)S.M[8]) - 1.0);
  const double t2 = (double)S.t[0] * (double)S.t[0] + (double)S.t[1] * (double)S.t[1] + (double)S.t[2] * (double)S.t[2];
  int st = BA_ICP_NOT_CONVERGED;
  if (S.iterations >= o.max_iter) st = BA_ICP_ITERATIONS;
  else if (cos_angle >= 1.0 - o.tr_eps && t2 <= o.tr_eps) st = BA_ICP_TRANSFORM;
  else if (fabs(mse - S.prev) < o.abs_eps) st = BA_ICP_ABS_MSE;
  else if (o.rel_eps > 0.0 && fabs(mse - S.prev) / S.prev < o.rel_eps) st = BA_ICP_REL_MSE;
  S.state = st;
  S.converged = st != BA_ICP_NOT_CONVERGED ? 1 : 0;
  S.apply_at = S.converged ? o.max_iter : round + 1;
  if (!S.converged) S.prev = mse;
  return mse;
}

}  // namespace bahip
