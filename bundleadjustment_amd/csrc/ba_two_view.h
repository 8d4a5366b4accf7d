// ba_two_view.h — the sampler, the minimal solvers and the per-pair geometry of
// ba_two_view_ransac (include/ba_hip.h), written once for the device
// (ba_two_view.hip) and for host programs (tests/cpp/two_view_host.cpp): plain
// C++ with no HIP dependency beyond the __host__ __device__ qualifiers.
//
// Null vector.  Both minimal solvers end in the null vector of an 8x9 system
// A.  tv_null9 takes it from the Householder QR of A^T: the k-th reflector
// H_k (k = 0 .. 7) maps the remainder of row k of A onto alpha_k e_k and is
// applied to the rows below, so A^T = (H_0 .. H_7) R with R upper triangular,
// and x = H_0 .. H_7 e_8 is orthogonal to every row of A.  The method works
// on A itself (A^T A is never formed) and is backward stable: |A x| is of the
// order of eps |A| whatever the conditioning.  A zero remainder gives the
// identity reflector, so a rank-deficient A (a degenerate sample) still
// yields a unit vector of its null space.  |x| = 1 up to rounding.
//
// E: the normalised eight-point on the bearings K^-1 [u, v, 1], dehomogenised
// to (x, y, 1); each side is Hartley-normalised over the eight samples
// (centroid to the origin, mean distance sqrt 2); row i of A is
// [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1]; E = T2^T E^ T1, scaled to
// Frobenius norm 1 (the sign is whatever the reflectors give).
//
// H: the four-point DLT on Hartley-normalised pixels; rows 2i, 2i+1 of A are
// [x1, y1, 1, 0, 0, 0, -x2 x1, -x2 y1, -x2] and [0, 0, 0, x1, y1, 1, -y2 x1,
// -y2 y1, -y2]; H = T2^-1 H^ T1, scaled to Frobenius norm 1, negated if the
// first sample transfers with w < 0.  H is invalid if any entry is non-finite
// or |det H| <= 1e-10 r0 r1 r2 with r_i the norms of its rows (Hadamard: the
// ratio is at most 1).
//
// 3x3 SVD (tv_svd3): one-sided Jacobi on the columns, singular values sorted
// decreasingly; u3 = u1 x u2 and v3 = v1 x v2, so U and V are rotations and
// A = U diag(s1, s2, sgn s3) V^T with sgn = +-1 returned.
#pragma once
#include <math.h>
#include <stdint.h>

#include "ba_p3p.h"

namespace bahip {

constexpr double kTvChi1 = 3.841, kTvChi2 = 5.991;   // the reference's th and thScore (SfMHelper.cpp:503-504)

// ---------------------------------------------------------------------------
// sampler
// ---------------------------------------------------------------------------
BA_P3P_HD inline uint32_t tv_draw(uint64_t seed, uint32_t h, uint32_t j, uint32_t m) {
  const uint64_t z = pnp_mix(seed + (16ull * h + j + 1ull) * 0x9E3779B97F4A7C15ull);
  return (uint32_t)(((z >> 32) * (uint64_t)m) >> 32);
}
// eight distinct local match indices of hypothesis h among n >= 8
BA_P3P_HD inline void tv_sample(uint64_t seed, uint32_t h, int n, int s[8]) {
  int srt[8];   // the earlier picks, increasing
  BA_P3P_UNROLL
  for (int j = 0; j < 8; ++j) {
    int c = (int)tv_draw(seed, h, (uint32_t)j, (uint32_t)(n - j));
    BA_P3P_UNROLL
    for (int i = 0; i < j; ++i)
      if (c >= srt[i]) ++c;
    s[j] = c;
    srt[j] = c;
    BA_P3P_UNROLL
    for (int i = j; i > 0; --i) {
      const int lo = srt[i - 1] < srt[i] ? srt[i - 1] : srt[i], hi = srt[i - 1] < srt[i] ? srt[i] : srt[i - 1];
      srt[i - 1] = lo; srt[i] = hi;
    }
  }
}

// ---------------------------------------------------------------------------
// the null vector of an 8x9 system (A is overwritten)
// ---------------------------------------------------------------------------
BA_P3P_HD inline void tv_null9(double A[8][9], double x[9]) {
  double beta[8];
  BA_P3P_UNROLL
  for (int k = 0; k < 8; ++k) {
    double sig = 0.0;
    BA_P3P_UNROLL
    for (int i = k; i < 9; ++i) sig += A[k][i] * A[k][i];
    const double akk = A[k][k];
    const double alpha = akk > 0.0 ? -sqrt(sig) : sqrt(sig);
    const double vk = akk - alpha;          // no cancellation: alpha has the other sign
    const double vn2 = -2.0 * alpha * vk;   // |v|^2
    const double b = vn2 > 0.0 ? 2.0 / vn2 : 0.0;
    A[k][k] = vk;
    beta[k] = b;
    BA_P3P_UNROLL
    for (int j = k + 1; j < 8; ++j) {
      double dot = 0.0;
      BA_P3P_UNROLL
      for (int i = k; i < 9; ++i) dot += A[k][i] * A[j][i];
      const double f = b * dot;
      BA_P3P_UNROLL
      for (int i = k; i < 9; ++i) A[j][i] -= f * A[k][i];
    }
  }
  BA_P3P_UNROLL
  for (int i = 0; i < 9; ++i) x[i] = i == 8 ? 1.0 : 0.0;
  BA_P3P_UNROLL
  for (int k = 7; k >= 0; --k) {
    double dot = 0.0;
    BA_P3P_UNROLL
    for (int i = k; i < 9; ++i) dot += A[k][i] * x[i];
    const double f = beta[k] * dot;
    BA_P3P_UNROLL
    for (int i = k; i < 9; ++i) x[i] -= f * A[k][i];
  }
}

BA_P3P_HD inline bool tv_finite9(const double M[9]) {
  bool ok = true;
  BA_P3P_UNROLL
  for (int e = 0; e < 9; ++e) ok = ok && fabs(M[e]) < HUGE_VAL;   // false for NaN
  return ok;
}
BA_P3P_HD inline void tv_unit9(double M[9]) {
  double s = 0.0;
  BA_P3P_UNROLL
  for (int e = 0; e < 9; ++e) s += M[e] * M[e];
  const double r = 1.0 / sqrt(s);
  BA_P3P_UNROLL
  for (int e = 0; e < 9; ++e) M[e] *= r;
}

// Hartley normalisation of NP points: p <- s (p - c); returns (cx, cy, s)
template <int NP>
BA_P3P_HD inline void tv_hartley(double p[NP][2], double T[3]) {
  double cx = 0.0, cy = 0.0, md = 0.0;
  BA_P3P_UNROLL
  for (int i = 0; i < NP; ++i) { cx += p[i][0]; cy += p[i][1]; }
  cx /= NP; cy /= NP;
  BA_P3P_UNROLL
  for (int i = 0; i < NP; ++i) {
    const double dx = p[i][0] - cx, dy = p[i][1] - cy;
    md += sqrt(dx * dx + dy * dy);
  }
  const double s = 1.4142135623730951 * NP / md;
  BA_P3P_UNROLL
  for (int i = 0; i < NP; ++i) { p[i][0] = s * (p[i][0] - cx); p[i][1] = s * (p[i][1] - cy); }
  T[0] = cx; T[1] = cy; T[2] = s;
}
// M = X T1 with T1 = [s 0 -s cx; 0 s -s cy; 0 0 1] (row-major 3x3)
BA_P3P_HD inline void tv_times_T(const double X[9], const double T[3], double M[9]) {
  BA_P3P_UNROLL
  for (int i = 0; i < 3; ++i) {
    M[3 * i] = X[3 * i] * T[2];
    M[3 * i + 1] = X[3 * i + 1] * T[2];
    M[3 * i + 2] = X[3 * i + 2] - T[2] * (T[0] * X[3 * i] + T[1] * X[3 * i + 1]);
  }
}

// (x, y) of the bearing K^-1 [u, v, 1] dehomogenised (Ki col-major)
BA_P3P_HD inline void tv_bearing(const double Ki[9], double u, double v, double b[2]) {
  const double x = Ki[0] * u + Ki[3] * v + Ki[6], y = Ki[1] * u + Ki[4] * v + Ki[7], z = Ki[2] * u + Ki[5] * v + Ki[8];
  b[0] = x / z; b[1] = y / z;
}

// the eight-point E (row-major, norm 1) of eight bearing pairs; false: invalid
BA_P3P_HD inline bool tv_solve_e(double b1[8][2], double b2[8][2], double E[9]) {
  double T1[3], T2[3], A[8][9], x[9], M[9];
  tv_hartley<8>(b1, T1);
  tv_hartley<8>(b2, T2);
  BA_P3P_UNROLL
  for (int i = 0; i < 8; ++i) {
    const double x1 = b1[i][0], y1 = b1[i][1], x2 = b2[i][0], y2 = b2[i][1];
    A[i][0] = x2 * x1; A[i][1] = x2 * y1; A[i][2] = x2;
    A[i][3] = y2 * x1; A[i][4] = y2 * y1; A[i][5] = y2;
    A[i][6] = x1; A[i][7] = y1; A[i][8] = 1.0;
  }
  tv_null9(A, x);
  tv_times_T(x, T1, M);
  // E = T2^T M
  BA_P3P_UNROLL
  for (int j = 0; j < 3; ++j) {
    E[j] = T2[2] * M[j];
    E[3 + j] = T2[2] * M[3 + j];
    E[6 + j] = M[6 + j] - T2[2] * (T2[0] * M[j] + T2[1] * M[3 + j]);
  }
  tv_unit9(E);
  return tv_finite9(E);
}

BA_P3P_HD inline double tv_det3(const double M[9]) {
  return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}
// inverse of a row-major 3x3 by cofactors
BA_P3P_HD inline void tv_inv3(const double M[9], double I[9]) {
  const double r = 1.0 / tv_det3(M);
  I[0] = (M[4] * M[8] - M[5] * M[7]) * r; I[1] = (M[2] * M[7] - M[1] * M[8]) * r; I[2] = (M[1] * M[5] - M[2] * M[4]) * r;
  I[3] = (M[5] * M[6] - M[3] * M[8]) * r; I[4] = (M[0] * M[8] - M[2] * M[6]) * r; I[5] = (M[2] * M[3] - M[0] * M[5]) * r;
  I[6] = (M[3] * M[7] - M[4] * M[6]) * r; I[7] = (M[1] * M[6] - M[0] * M[7]) * r; I[8] = (M[0] * M[4] - M[1] * M[3]) * r;
}

// the four-point H (row-major, norm 1, x2 ~ H x1) of four pixel pairs; false: invalid
BA_P3P_HD inline bool tv_solve_h(double p1[4][2], double p2[4][2], double H[9]) {
  const double u0 = p1[0][0], v0 = p1[0][1];
  double T1[3], T2[3], A[8][9], x[9], M[9];
  tv_hartley<4>(p1, T1);
  tv_hartley<4>(p2, T2);
  BA_P3P_UNROLL
  for (int i = 0; i < 4; ++i) {
    const double x1 = p1[i][0], y1 = p1[i][1], x2 = p2[i][0], y2 = p2[i][1];
    double* r0 = A[2 * i];
    double* r1 = A[2 * i + 1];
    r0[0] = x1; r0[1] = y1; r0[2] = 1.0; r0[3] = 0.0; r0[4] = 0.0; r0[5] = 0.0; r0[6] = -x2 * x1; r0[7] = -x2 * y1; r0[8] = -x2;
    r1[0] = 0.0; r1[1] = 0.0; r1[2] = 0.0; r1[3] = x1; r1[4] = y1; r1[5] = 1.0; r1[6] = -y2 * x1; r1[7] = -y2 * y1; r1[8] = -y2;
  }
  tv_null9(A, x);
  tv_times_T(x, T1, M);
  // H = T2^-1 M, T2^-1 = [1/s 0 cx; 0 1/s cy; 0 0 1]
  const double is = 1.0 / T2[2];
  BA_P3P_UNROLL
  for (int j = 0; j < 3; ++j) {
    H[j] = is * M[j] + T2[0] * M[6 + j];
    H[3 + j] = is * M[3 + j] + T2[1] * M[6 + j];
    H[6 + j] = M[6 + j];
  }
  tv_unit9(H);
  if (H[6] * u0 + H[7] * v0 + H[8] < 0.0) {
    BA_P3P_UNROLL
    for (int e = 0; e < 9; ++e) H[e] = -H[e];
  }
  const double r0 = sqrt(H[0] * H[0] + H[1] * H[1] + H[2] * H[2]), r1 = sqrt(H[3] * H[3] + H[4] * H[4] + H[5] * H[5]),
               r2 = sqrt(H[6] * H[6] + H[7] * H[7] + H[8] * H[8]);
  return tv_finite9(H) && fabs(tv_det3(H)) > 1e-10 * (r0 * r1 * r2);
}

// ---------------------------------------------------------------------------
// predicates (the operation order the header pins)
// ---------------------------------------------------------------------------
// F = K2^-T E K1^-1 (row-major; Ki1, Ki2 col-major inverses)
BA_P3P_HD inline void tv_fundamental(const double E[9], const double Ki1[9], const double Ki2[9], double F[9]) {
  double M[9];
  BA_P3P_UNROLL
  for (int k = 0; k < 3; ++k)
    BA_P3P_UNROLL
    for (int j = 0; j < 3; ++j) M[3 * k + j] = E[3 * k] * Ki1[3 * j] + E[3 * k + 1] * Ki1[3 * j + 1] + E[3 * k + 2] * Ki1[3 * j + 2];
  BA_P3P_UNROLL
  for (int i = 0; i < 3; ++i)
    BA_P3P_UNROLL
    for (int j = 0; j < 3; ++j) F[3 * i + j] = Ki2[3 * i] * M[j] + Ki2[3 * i + 1] * M[3 + j] + Ki2[3 * i + 2] * M[6 + j];
}
// squared distances to the epipolar lines: d1 in image 1 (line F^T x2), d2 in image 2 (line F x1)
BA_P3P_HD inline void tv_e_dist2(const double F[9], double u1, double v1, double u2, double v2, double* d1, double* d2) {
  const double a0 = F[0] * u1 + F[1] * v1 + F[2], a1 = F[3] * u1 + F[4] * v1 + F[5], a2 = F[6] * u1 + F[7] * v1 + F[8];
  const double n2 = u2 * a0 + v2 * a1 + a2;
  *d2 = n2 * n2 / (a0 * a0 + a1 * a1);
  const double b0 = F[0] * u2 + F[3] * v2 + F[6], b1 = F[1] * u2 + F[4] * v2 + F[7], b2 = F[2] * u2 + F[5] * v2 + F[8];
  const double n1 = u1 * b0 + v1 * b1 + b2;
  *d1 = n1 * n1 / (b0 * b0 + b1 * b1);
}
// squared transfer error of (u, v) -> (ut, vt) under M; HUGE_VAL when w <= 0
BA_P3P_HD inline double tv_h_err2(const double M[9], double u, double v, double ut, double vt) {
  const double p0 = M[0] * u + M[1] * v + M[2], p1 = M[3] * u + M[4] * v + M[5], w = M[6] * u + M[7] * v + M[8];
  const double e0 = ut - p0 / w, e1 = vt - p1 / w;
  return w > 0.0 ? e0 * e0 + e1 * e1 : HUGE_VAL;
}

// ---------------------------------------------------------------------------
// 3x3 SVD and the decompositions
// ---------------------------------------------------------------------------
BA_P3P_HD inline void tv_cross(const double a[3], const double b[3], double c[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

// A (row-major) = U diag(s0, s1, sgn s2) V^T, s0 >= s1 >= s2 >= 0, U and V
// rotations whose columns are U[c], V[c]; returns sgn
BA_P3P_HD inline double tv_svd3(const double A[9], double U[3][3], double s[3], double V[3][3]) {
  double B[3][3];   // B[c] = column c
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < 3; ++r) { B[c][r] = A[3 * r + c]; V[c][r] = r == c ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < 20; ++sweep) {
    bool rotated = false;
    for (int pq = 0; pq < 3; ++pq) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      const double al = B[p][0] * B[p][0] + B[p][1] * B[p][1] + B[p][2] * B[p][2];
      const double be = B[q][0] * B[q][0] + B[q][1] * B[q][1] + B[q][2] * B[q][2];
      const double ga = B[p][0] * B[q][0] + B[p][1] * B[q][1] + B[p][2] * B[q][2];
      if (!(fabs(ga) > 1e-15 * sqrt(al * be))) continue;
      rotated = true;
      const double zeta = (be - al) / (2.0 * ga);
      const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
      const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
      for (int r = 0; r < 3; ++r) {
        const double bp = B[p][r], bq = B[q][r], vp = V[p][r], vq = V[q][r];
        B[p][r] = cs * bp - sn * bq; B[q][r] = sn * bp + cs * bq;
        V[p][r] = cs * vp - sn * vq; V[q][r] = sn * vp + cs * vq;
      }
    }
    if (!rotated) break;
  }
  for (int c = 0; c < 3; ++c) s[c] = sqrt(B[c][0] * B[c][0] + B[c][1] * B[c][1] + B[c][2] * B[c][2]);
  // sort decreasingly: (0,1) (1,2) (0,1)
  for (int pass = 0; pass < 3; ++pass) {
    const int a = pass == 1 ? 1 : 0, b = a + 1;
    if (s[a] < s[b]) {
      const double ts = s[a]; s[a] = s[b]; s[b] = ts;
      for (int r = 0; r < 3; ++r) {
        const double tb = B[a][r]; B[a][r] = B[b][r]; B[b][r] = tb;
        const double tv = V[a][r]; V[a][r] = V[b][r]; V[b][r] = tv;
      }
    }
  }
  for (int r = 0; r < 3; ++r) { U[0][r] = B[0][r] / s[0]; U[1][r] = B[1][r] / s[1]; }
  // u1 orthogonal to u0 exactly enough for the cross product to be a unit vector
  double v3[3];
  tv_cross(U[0], U[1], U[2]);
  tv_cross(V[0], V[1], v3);
  const double su = B[2][0] * U[2][0] + B[2][1] * U[2][1] + B[2][2] * U[2][2];
  const double sv = V[2][0] * v3[0] + V[2][1] * v3[1] + V[2][2] * v3[2];
  for (int r = 0; r < 3; ++r) V[2][r] = v3[r];
  return (su < 0.0) != (sv < 0.0) ? -1.0 : 1.0;
}

// The essential projection: E (row-major) -> U, V (rotations) and the nearest
// E' = (u0 v0^T + u1 v1^T) / sqrt 2.  false: rank below 2 or non-finite.
BA_P3P_HD inline bool tv_project_e(const double E[9], double Ep[9], double U[3][3], double V[3][3]) {
  double s[3];
  tv_svd3(E, U, s, V);
  const double r = 0.7071067811865476;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Ep[3 * i + j] = r * (U[0][i] * V[0][j] + U[1][i] * V[1][j]);
  return tv_finite9(Ep) && s[1] > 0.0;
}

// Candidate c = 0 .. 3 of E: (U W V^T, +u2), (U W V^T, -u2), (U W^T V^T, +u2),
// (U W^T V^T, -u2), W = [0 -1 0; 1 0 0; 0 0 1].  R row-major.
BA_P3P_HD inline void tv_e_candidate(const double U[3][3], const double V[3][3], int c, double R[9], double t[3]) {
  const double w = c < 2 ? 1.0 : -1.0, st = (c & 1) ? -1.0 : 1.0;
  // U W V^T = w (u1 v0^T - u0 v1^T) + u2 v2^T
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) R[3 * i + j] = w * (U[1][i] * V[0][j] - U[0][i] * V[1][j]) + U[2][i] * V[2][j];
    t[i] = st * U[2][i];
  }
}

// The SVD decomposition of A = K2^-1 H K1 (Faugeras; the case split and the
// order of ORB-SLAM's ReconstructH): candidates 0 .. 3 take d' = +d2,
// 4 .. 7 d' = -d2; within each, (e1, e3) = (+,+) (+,-) (-,+) (-,-) are the
// signs of the plane normal's first and third SVD coordinates.  n has n_z >= 0
// and |t| = 1.  tv_h_decompose returns false when two singular values
// coincide within 1e-5 relative (or are not finite).
struct TvHDecomp { double U[3][3], V[3][3], d[3], sgn; };
BA_P3P_HD inline bool tv_h_decompose(const double A[9], TvHDecomp* D) {
  D->sgn = tv_svd3(A, D->U, D->d, D->V);
  for (int r = 0; r < 3; ++r) D->U[2][r] *= D->sgn;   // A = U diag(d) V^T with det U det V = sgn
  const double d1 = D->d[0], d2 = D->d[1], d3 = D->d[2];
  return d1 < HUGE_VAL && d3 == d3 && d1 / d2 >= 1.00001 && d2 / d3 >= 1.00001;
}
BA_P3P_HD inline void tv_h_candidate(const TvHDecomp* D, int c, double R[9], double t[3], double n[3]) {
  const double d1 = D->d[0], d2 = D->d[1], d3 = D->d[2], s = D->sgn;
  const double q1 = d1 * d1, q2 = d2 * d2, q3 = d3 * d3;
  const double e1 = (c & 2) ? -1.0 : 1.0, e3 = (c & 1) ? -1.0 : 1.0;
  const double x1 = e1 * sqrt((q1 - q2) / (q1 - q3)), x3 = e3 * sqrt((q2 - q3) / (q1 - q3));
  const double root = sqrt((q1 - q2) * (q2 - q3));
  double Rp[9], tp[3];
  if (c < 4) {
    const double st = e1 * e3 * root / ((d1 + d3) * d2), ct = (q2 + d1 * d3) / ((d1 + d3) * d2);
    Rp[0] = ct; Rp[1] = 0.0; Rp[2] = -st; Rp[3] = 0.0; Rp[4] = 1.0; Rp[5] = 0.0; Rp[6] = st; Rp[7] = 0.0; Rp[8] = ct;
    tp[0] = (d1 - d3) * x1; tp[1] = 0.0; tp[2] = -(d1 - d3) * x3;
  } else {
    const double sp = e1 * e3 * root / ((d1 - d3) * d2), cp = (d1 * d3 - q2) / ((d1 - d3) * d2);
    Rp[0] = cp; Rp[1] = 0.0; Rp[2] = sp; Rp[3] = 0.0; Rp[4] = -1.0; Rp[5] = 0.0; Rp[6] = sp; Rp[7] = 0.0; Rp[8] = -cp;
    tp[0] = (d1 + d3) * x1; tp[1] = 0.0; tp[2] = (d1 + d3) * x3;
  }
  // R = s U Rp V^T, t = U tp / |.|, n = V (x1, 0, x3)
  double M[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) M[3 * i + j] = D->U[0][i] * Rp[j] + D->U[1][i] * Rp[3 + j] + D->U[2][i] * Rp[6 + j];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[3 * i + j] = s * (M[3 * i] * D->V[0][j] + M[3 * i + 1] * D->V[1][j] + M[3 * i + 2] * D->V[2][j]);
  double tn = 0.0;
  for (int i = 0; i < 3; ++i) {
    t[i] = D->U[0][i] * tp[0] + D->U[2][i] * tp[2];
    n[i] = D->V[0][i] * x1 + D->V[2][i] * x3;
    tn += t[i] * t[i];
  }
  tn = 1.0 / sqrt(tn);
  const double ns = n[2] < 0.0 ? -1.0 : 1.0;
  for (int i = 0; i < 3; ++i) { t[i] *= tn; n[i] *= ns; }
}

// Positive depth in both views: (l1, l2) of the least-squares solve of
// l2 b2 = l1 R b1 + t, b = (x, y, 1); a determinant at or below 1e-12 |R b1|^2
// |b2|^2 (no parallax) is not good.
BA_P3P_HD inline bool tv_depth_good(const double R[9], const double t[3], const double b1[2], const double b2[2]) {
  const double a[3] = {R[0] * b1[0] + R[1] * b1[1] + R[2], R[3] * b1[0] + R[4] * b1[1] + R[5], R[6] * b1[0] + R[7] * b1[1] + R[8]};
  const double b[3] = {b2[0], b2[1], 1.0};
  const double aa = a[0] * a[0] + a[1] * a[1] + a[2] * a[2], bb = b[0] * b[0] + b[1] * b[1] + b[2] * b[2];
  const double ab = a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
  const double at = a[0] * t[0] + a[1] * t[1] + a[2] * t[2], bt = b[0] * t[0] + b[1] * t[1] + b[2] * t[2];
  const double det = aa * bb - ab * ab;
  const double l1 = (ab * bt - bb * at) / det, l2 = (aa * bt - ab * at) / det;
  return det > 1e-12 * (aa * bb) && l1 > 0.0 && l2 > 0.0;
}

}  // namespace bahip
