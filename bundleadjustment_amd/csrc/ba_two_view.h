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
// E, five-point (BA_TV_E_FIVE_POINT): tv_solve_e5, described where it stands.
//
// 3x3 SVD (tv_svd3): one-sided Jacobi on the columns, singular values sorted
// decreasingly; u3 = u1 x u2 and v3 = v1 x v2, so U and V are rotations and
// A = U diag(s1, s2, sgn s3) V^T with sgn = +-1 returned.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

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

// ---------------------------------------------------------------------------
// The five-point E (BA_TV_E_FIVE_POINT; include/ba_hip.h pins the semantics).
//
// tv_solve_e5 works in a strided store S: element i lives at S[i * st].  A
// host program passes a local array (st = 1); the device passes its lane's
// column of an LDS array (st = 64), so that everything a run-time index
// addresses (the 10x20 system, the basis, the derivative table, the
// breakpoints) sits in LDS and nothing needs scratch memory.  Layout of S:
//   [0, 200)    the system M, row-major 10x20; after the elimination the
//               space is reused: [0, 121) the derivatives D[m][j] of the
//               tenth-degree polynomial, [121, 134) and [134, 147) the two
//               breakpoint arrays
//   [200, 236)  the basis X, Y, Z, W (row-major 3x3 each)
// Columns of M, Nister's order:
//   x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
// ---------------------------------------------------------------------------
BA_P3P_HD inline void tv_cross(const double a[3], const double b[3], double c[3]);
BA_P3P_HD inline void tv_inv3(const double M[9], double I[9]);

constexpr int kTv5Store = 236;          // doubles of S per hypothesis
constexpr int kTv5Basis = 200;
constexpr double kTv5PivotFloor = 1e-13;   // relative to the largest |entry| of M
constexpr int kTv5PolishSteps = 12;
constexpr double kTv5PolishDone = 1e-30;    // |C(E / |E|)|^2
constexpr double kTv5RootBound = 1e25;     // roots are sought in [-B, B], B = min(Fujiwara, this)

// The null space of the 5x9 system A (overwritten): X, Y, Z, W = H_0 .. H_4 e_j,
// j = 5 .. 8, of the Householder QR of A^T (tv_null9's method); orthonormal
// whatever the rank of A.  B: S + kTv5Basis * st.
BA_P3P_HD inline void tv5_null_basis(double A[5][9], double* B, int st) {
  double beta[5];
  BA_P3P_UNROLL
  for (int k = 0; k < 5; ++k) {
    double sig = 0.0;
    BA_P3P_UNROLL
    for (int i = k; i < 9; ++i) sig += A[k][i] * A[k][i];
    const double akk = A[k][k];
    const double alpha = akk > 0.0 ? -sqrt(sig) : sqrt(sig);
    const double vk = akk - alpha;
    const double vn2 = -2.0 * alpha * vk;
    const double b = vn2 > 0.0 ? 2.0 / vn2 : 0.0;
    A[k][k] = vk;
    beta[k] = b;
    BA_P3P_UNROLL
    for (int j = k + 1; j < 5; ++j) {
      double dot = 0.0;
      BA_P3P_UNROLL
      for (int i = k; i < 9; ++i) dot += A[k][i] * A[j][i];
      const double f = b * dot;
      BA_P3P_UNROLL
      for (int i = k; i < 9; ++i) A[j][i] -= f * A[k][i];
    }
  }
  BA_P3P_UNROLL
  for (int v = 0; v < 4; ++v) {
    double x[9];
    BA_P3P_UNROLL
    for (int i = 0; i < 9; ++i) x[i] = i == 5 + v ? 1.0 : 0.0;
    BA_P3P_UNROLL
    for (int k = 4; k >= 0; --k) {
      double dot = 0.0;
      BA_P3P_UNROLL
      for (int i = k; i < 9; ++i) dot += A[k][i] * x[i];
      const double f = beta[k] * dot;
      BA_P3P_UNROLL
      for (int i = k; i < 9; ++i) x[i] -= f * A[k][i];
    }
    BA_P3P_UNROLL
    for (int i = 0; i < 9; ++i) B[(9 * v + i) * st] = x[i];
  }
}

// entry e of E = xX + yY + zZ + W as a linear polynomial (x, y, z, 1)
// with the roles turned by h: (x, y, z) multiply basis matrices h, h + 1, h + 2 (mod 3)
BA_P3P_HD inline void tv5_entry(const double* B, int st, int h, int e, double p[4]) {
  const int v0 = h, v1 = h == 2 ? 0 : h + 1, v2 = h == 0 ? 2 : h - 1;
  p[0] = B[(9 * v0 + e) * st]; p[1] = B[(9 * v1 + e) * st]; p[2] = B[(9 * v2 + e) * st]; p[3] = B[(27 + e) * st];
}
// d += s a b; quadratics as (xx, yy, zz, xy, xz, yz, x, y, z, 1)
BA_P3P_HD inline void tv5_mul11(const double a[4], const double b[4], double s, double d[10]) {
  d[0] += s * (a[0] * b[0]); d[1] += s * (a[1] * b[1]); d[2] += s * (a[2] * b[2]);
  d[3] += s * (a[0] * b[1] + a[1] * b[0]); d[4] += s * (a[0] * b[2] + a[2] * b[0]); d[5] += s * (a[1] * b[2] + a[2] * b[1]);
  d[6] += s * (a[0] * b[3] + a[3] * b[0]); d[7] += s * (a[1] * b[3] + a[3] * b[1]); d[8] += s * (a[2] * b[3] + a[3] * b[2]);
  d[9] += s * (a[3] * b[3]);
}
// r += d c; cubics in the column order of M
BA_P3P_HD inline void tv5_mul21(const double d[10], const double c[4], double r[20]) {
  r[0] += d[0] * c[0];
  r[1] += d[1] * c[1];
  r[2] += d[0] * c[1] + d[3] * c[0];
  r[3] += d[1] * c[0] + d[3] * c[1];
  r[4] += d[0] * c[2] + d[4] * c[0];
  r[5] += d[0] * c[3] + d[6] * c[0];
  r[6] += d[1] * c[2] + d[5] * c[1];
  r[7] += d[1] * c[3] + d[7] * c[1];
  r[8] += d[3] * c[2] + d[4] * c[1] + d[5] * c[0];
  r[9] += d[3] * c[3] + d[6] * c[1] + d[7] * c[0];
  r[10] += d[2] * c[0] + d[4] * c[2];
  r[11] += d[4] * c[3] + d[6] * c[2] + d[8] * c[0];
  r[12] += d[6] * c[3] + d[9] * c[0];
  r[13] += d[2] * c[1] + d[5] * c[2];
  r[14] += d[5] * c[3] + d[7] * c[2] + d[8] * c[1];
  r[15] += d[7] * c[3] + d[9] * c[1];
  r[16] += d[2] * c[2];
  r[17] += d[2] * c[3] + d[8] * c[2];
  r[18] += d[8] * c[3] + d[9] * c[2];
  r[19] += d[9] * c[3];
}
// Constraint row r of M: r = 3i + j < 9 is entry (i, j) of 2 E E^T E -
// tr(E E^T) E = sum_l (2 sum_k E_ik E_lk - [l = i] tr) E_lj; r = 9 is det E by
// the first row's cofactors.
BA_P3P_HD inline void tv5_constraint_row(const double* B, int st, int h, int r, double row[20]) {
  BA_P3P_UNROLL
  for (int c = 0; c < 20; ++c) row[c] = 0.0;
  double a[4], b[4], c[4], d[10];
  if (r < 9) {
    const int i = r / 3, j = r - 3 * i;
    double tr[10];
    BA_P3P_UNROLL
    for (int q = 0; q < 10; ++q) tr[q] = 0.0;
    for (int e = 0; e < 9; ++e) {
      tv5_entry(B, st, h, e, a);
      tv5_mul11(a, a, 1.0, tr);
    }
    for (int l = 0; l < 3; ++l) {
      const double w = l == i ? 1.0 : 0.0;
      BA_P3P_UNROLL
      for (int q = 0; q < 10; ++q) d[q] = -w * tr[q];
      for (int k = 0; k < 3; ++k) {
        tv5_entry(B, st, h, 3 * i + k, a);
        tv5_entry(B, st, h, 3 * l + k, b);
        tv5_mul11(a, b, 2.0, d);
      }
      tv5_entry(B, st, h, 3 * l + j, c);
      tv5_mul21(d, c, row);
    }
  } else {
    for (int k = 0; k < 3; ++k) {
      const int k1 = k == 2 ? 0 : k + 1, k2 = k == 0 ? 2 : k - 1;   // E_0k (E_1k1 E_2k2 - E_1k2 E_2k1)
      BA_P3P_UNROLL
      for (int q = 0; q < 10; ++q) d[q] = 0.0;
      tv5_entry(B, st, h, 3 + k1, a);
      tv5_entry(B, st, h, 6 + k2, b);
      tv5_mul11(a, b, 1.0, d);
      tv5_entry(B, st, h, 3 + k2, a);
      tv5_entry(B, st, h, 6 + k1, b);
      tv5_mul11(a, b, -1.0, d);
      tv5_entry(B, st, h, k, c);
      tv5_mul21(d, c, row);
    }
  }
}

// Gauss-Jordan with partial pivoting on columns 0 .. 9 of M (ties: the lower
// row).  Rows 0 .. 3 are not reduced once they have served as pivot rows: only
// rows 4 .. 9 are read afterwards.  false: a pivot at or below the floor.
BA_P3P_HD inline bool tv5_eliminate(double* M, int st) {
  double big = 0.0;
  for (int i = 0; i < 200; ++i) { const double v = fabs(M[i * st]); big = v > big ? v : big; }
  if (!(big < HUGE_VAL)) return false;
  const double floor_ = kTv5PivotFloor * big;
  for (int k = 0; k < 10; ++k) {
    int p = k;
    double best = fabs(M[(20 * k + k) * st]);
    for (int r = k + 1; r < 10; ++r) {
      const double v = fabs(M[(20 * r + k) * st]);
      if (v > best) { best = v; p = r; }
    }
    if (!(best > floor_)) return false;
    double piv[20];
    const double inv = 1.0 / M[(20 * p + k) * st];
    BA_P3P_UNROLL
    for (int c = 0; c < 20; ++c) {
      const double v = M[(20 * p + c) * st];
      M[(20 * p + c) * st] = M[(20 * k + c) * st];
      piv[c] = v * inv;
      M[(20 * k + c) * st] = piv[c];
    }
    for (int r = 0; r < 10; ++r) {
      if (r == k || (r < k && r < 4)) continue;
      const double f = M[(20 * r + k) * st];
      BA_P3P_UNROLL
      for (int c = 0; c < 20; ++c) M[(20 * r + c) * st] -= f * piv[c];
    }
  }
  return true;
}

// doubles <-> integers of the same order (-0 and +0 coincide)
BA_P3P_HD inline int64_t tv5_key(double v) {
  int64_t i;
  memcpy(&i, &v, sizeof i);
  return i >= 0 ? i : (int64_t)(0x8000000000000000ull - (uint64_t)i);
}
BA_P3P_HD inline double tv5_unkey(int64_t k) {
  const int64_t i = k >= 0 ? k : (int64_t)(0x8000000000000000ull - (uint64_t)k);
  double v;
  memcpy(&v, &i, sizeof v);
  return v;
}
BA_P3P_HD inline double tv5_horner(const double q[11], double z) {
  double v = q[10];
  BA_P3P_UNROLL
  for (int j = 9; j >= 0; --j) v = v * z + q[j];
  return v;
}
// <k>, <l>, <m> of Nister's elimination: row t is x px[t](z) + y py[t](z) + p1[t](z),
// degrees 3, 3, 4, coefficients by increasing power
struct Tv5Rows { double px[3][4], py[3][4], p1[3][5]; };
BA_P3P_HD inline void tv5_rows_at(const Tv5Rows& P, double z, double a[3][3]) {
  BA_P3P_UNROLL
  for (int t = 0; t < 3; ++t) {
    a[t][0] = ((P.px[t][3] * z + P.px[t][2]) * z + P.px[t][1]) * z + P.px[t][0];
    a[t][1] = ((P.py[t][3] * z + P.py[t][2]) * z + P.py[t][1]) * z + P.py[t][0];
    a[t][2] = (((P.p1[t][4] * z + P.p1[t][3]) * z + P.p1[t][2]) * z + P.p1[t][1]) * z + P.p1[t][0];
  }
}
// q(z) by Horner, or (direct) the determinant the tenth-degree polynomial expands
BA_P3P_HD inline double tv5_eval(const double q[11], const Tv5Rows& P, bool direct, double z) {
  if (!direct) return tv5_horner(q, z);
  double a[3][3];
  tv5_rows_at(P, z, a);
  return a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]) - a[1][2] * (a[0][0] * a[2][1] - a[0][1] * a[2][0]) +
         a[2][2] * (a[0][0] * a[1][1] - a[0][1] * a[1][0]);
}
// The root in [a, b], value(a) < 0 being `neg_a` and value(b) < 0 its
// opposite: at most 64 bisections on the ordered integers of the doubles (the
// midpoint of the keys), to adjacent doubles; the end with the smaller
// |value| is returned.
BA_P3P_HD inline double tv5_bisect(const double q[11], const Tv5Rows& P, bool direct, double a, double b, bool neg_a) {
  int64_t ka = tv5_key(a), kb = tv5_key(b);
  for (int it = 0; it < 64; ++it) {
    if ((uint64_t)kb - (uint64_t)ka <= 1ull) break;
    const int64_t km = (ka >> 1) + (kb >> 1) + (ka & kb & 1);
    if ((tv5_eval(q, P, direct, tv5_unkey(km)) < 0.0) == neg_a) ka = km; else kb = km;
  }
  const double za = tv5_unkey(ka), zb = tv5_unkey(kb);
  return fabs(tv5_eval(q, P, direct, za)) <= fabs(tv5_eval(q, P, direct, zb)) ? za : zb;
}

// C = 2 E E^T E - tr(E E^T) E, G = E E^T; returns tr G
BA_P3P_HD inline double tv5_cubic(const double E[9], double G[9], double C[9]) {
  BA_P3P_UNROLL
  for (int i = 0; i < 3; ++i)
    BA_P3P_UNROLL
    for (int j = 0; j < 3; ++j) G[3 * i + j] = E[3 * i] * E[3 * j] + E[3 * i + 1] * E[3 * j + 1] + E[3 * i + 2] * E[3 * j + 2];
  const double tr = G[0] + G[4] + G[8];
  BA_P3P_UNROLL
  for (int i = 0; i < 3; ++i)
    BA_P3P_UNROLL
    for (int j = 0; j < 3; ++j)
      C[3 * i + j] = 2.0 * (G[3 * i] * E[j] + G[3 * i + 1] * E[3 + j] + G[3 * i + 2] * E[6 + j]) - tr * E[3 * i + j];
  return tr;
}
// E = xX + yY + zZ + W, C(E) and cost = |C|^2 / |E|^6 (the squared residual of E / |E|)
BA_P3P_HD inline double tv5_point(const double* B, int st, const double v[3], double E[9], double G[9], double C[9], double* tr) {
  BA_P3P_UNROLL
  for (int e = 0; e < 9; ++e) E[e] = v[0] * B[e * st] + v[1] * B[(9 + e) * st] + v[2] * B[(18 + e) * st] + B[(27 + e) * st];
  *tr = tv5_cubic(E, G, C);
  double c2 = 0.0;
  BA_P3P_UNROLL
  for (int e = 0; e < 9; ++e) c2 += C[e] * C[e];
  return c2 / (*tr * *tr * *tr);
}
// Up to kTv5PolishSteps Gauss-Newton steps of (x, y, z) on the nine cubic
// constraints.  The polish ends at a cost of rounding size (kTv5PolishDone)
// or at the first step that does not lower the cost (that step is not kept).
// A root of the tenth-degree polynomial that two solutions (nearly) share has
// no well-defined (x, y) of its own and needs the steps; every other root
// ends after one or two.
BA_P3P_HD inline void tv5_polish(const double* B, int st, double v[3], double E[9]) {
  double G[9], C[9], tr;
  double cost = tv5_point(B, st, v, E, G, C, &tr);
  for (int it = 0; it < kTv5PolishSteps && cost > kTv5PolishDone; ++it) {
    double J[3][9];
    BA_P3P_UNROLL
    for (int k = 0; k < 3; ++k) {
      double D[9], dG[9];
      BA_P3P_UNROLL
      for (int e = 0; e < 9; ++e) D[e] = B[(9 * k + e) * st];
      double dtr = 0.0;
      BA_P3P_UNROLL
      for (int e = 0; e < 9; ++e) dtr += 2.0 * E[e] * D[e];
      BA_P3P_UNROLL
      for (int i = 0; i < 3; ++i)
        BA_P3P_UNROLL
        for (int j = 0; j < 3; ++j)
          dG[3 * i + j] = D[3 * i] * E[3 * j] + D[3 * i + 1] * E[3 * j + 1] + D[3 * i + 2] * E[3 * j + 2] +
                          E[3 * i] * D[3 * j] + E[3 * i + 1] * D[3 * j + 1] + E[3 * i + 2] * D[3 * j + 2];
      BA_P3P_UNROLL
      for (int i = 0; i < 3; ++i)
        BA_P3P_UNROLL
        for (int j = 0; j < 3; ++j)
          J[k][3 * i + j] = 2.0 * (dG[3 * i] * E[j] + dG[3 * i + 1] * E[3 + j] + dG[3 * i + 2] * E[6 + j] +
                                   G[3 * i] * D[j] + G[3 * i + 1] * D[3 + j] + G[3 * i + 2] * D[6 + j]) -
                            dtr * E[3 * i + j] - tr * D[3 * i + j];
    }
    double N[9], Ni[9], g[3];
    BA_P3P_UNROLL
    for (int a = 0; a < 3; ++a) {
      g[a] = 0.0;
      BA_P3P_UNROLL
      for (int e = 0; e < 9; ++e) g[a] += J[a][e] * C[e];
      BA_P3P_UNROLL
      for (int b = 0; b < 3; ++b) {
        double d = 0.0;
        BA_P3P_UNROLL
        for (int e = 0; e < 9; ++e) d += J[a][e] * J[b][e];
        N[3 * a + b] = d;
      }
    }
    tv_inv3(N, Ni);
    double w[3], E2[9], G2[9], C2[9], tr2;
    BA_P3P_UNROLL
    for (int a = 0; a < 3; ++a) w[a] = v[a] - (Ni[3 * a] * g[0] + Ni[3 * a + 1] * g[1] + Ni[3 * a + 2] * g[2]);
    const double cost2 = tv5_point(B, st, w, E2, G2, C2, &tr2);
    if (!(cost2 < cost)) break;
    cost = cost2; tr = tr2;
    BA_P3P_UNROLL
    for (int a = 0; a < 3; ++a) v[a] = w[a];
    BA_P3P_UNROLL
    for (int e = 0; e < 9; ++e) { E[e] = E2[e]; G[e] = G2[e]; C[e] = C2[e]; }
  }
}

// a (deg na) times b (deg nb) into c (deg na + nb)
template <int NA, int NB>
BA_P3P_HD inline void tv5_polymul(const double (&a)[NA], const double (&b)[NB], double (&c)[NA + NB - 1]) {
  BA_P3P_UNROLL
  for (int i = 0; i < NA + NB - 1; ++i) c[i] = 0.0;
  BA_P3P_UNROLL
  for (int i = 0; i < NA; ++i)
    BA_P3P_UNROLL
    for (int j = 0; j < NB; ++j) c[i + j] += a[i] * b[j];
}

// The five-point essential matrices of five bearing pairs (the first five of
// the eight picks): up to ten real solutions, ordered by increasing z, each
// row-major with Frobenius norm 1, solution s at out + s * sol_stride; the
// entries of the solutions not found are zero.  Returns their number.
BA_P3P_HD inline int tv_solve_e5(const double b1[5][2], const double b2[5][2], double* S, int st, double* out,
                                 size_t sol_stride) {
  for (int s = 0; s < 10; ++s)
    for (int e = 0; e < 9; ++e) out[s * sol_stride + e] = 0.0;
  double* B = S + (size_t)kTv5Basis * st;
  {
    double A[5][9];
    BA_P3P_UNROLL
    for (int i = 0; i < 5; ++i) {
      const double x1 = b1[i][0], y1 = b1[i][1], x2 = b2[i][0], y2 = b2[i][1];
      A[i][0] = x2 * x1; A[i][1] = x2 * y1; A[i][2] = x2;
      A[i][3] = y2 * x1; A[i][4] = y2 * y1; A[i][5] = y2;
      A[i][6] = x1; A[i][7] = y1; A[i][8] = 1.0;
    }
    tv5_null_basis(A, B, st);
  }
  // The hidden variable: of the three turns of (X, Y, Z), the one whose
  // reduced rows 4 .. 9 have the smallest largest |entry| (ties: the earlier);
  // a turn whose elimination fails is not a candidate.
  Tv5Rows P;
  double least = HUGE_VAL;
  int hid = -1;
  for (int h = 0; h < 3; ++h) {
    for (int r = 0; r < 10; ++r) {
      double row[20];
      tv5_constraint_row(B, st, h, r, row);
      BA_P3P_UNROLL
      for (int c = 0; c < 20; ++c) S[(20 * r + c) * st] = row[c];
    }
    if (!tv5_eliminate(S, st)) continue;
    // <k> = row 4 - z row 5, <l> = row 6 - z row 7, <m> = row 8 - z row 9
    Tv5Rows Q;
    double big = 0.0;
    BA_P3P_UNROLL
    for (int t = 0; t < 3; ++t) {
      double u[10], v[10];
      BA_P3P_UNROLL
      for (int c = 0; c < 10; ++c) {
        u[c] = S[(20 * (4 + 2 * t) + 10 + c) * st]; v[c] = S[(20 * (5 + 2 * t) + 10 + c) * st];
        big = fabs(u[c]) > big ? fabs(u[c]) : big;
        big = fabs(v[c]) > big ? fabs(v[c]) : big;
      }
      Q.px[t][0] = u[2]; Q.px[t][1] = u[1] - v[2]; Q.px[t][2] = u[0] - v[1]; Q.px[t][3] = -v[0];
      Q.py[t][0] = u[5]; Q.py[t][1] = u[4] - v[5]; Q.py[t][2] = u[3] - v[4]; Q.py[t][3] = -v[3];
      Q.p1[t][0] = u[9]; Q.p1[t][1] = u[8] - v[9]; Q.p1[t][2] = u[7] - v[8]; Q.p1[t][3] = u[6] - v[7]; Q.p1[t][4] = -v[6];
    }
    if (big < least) { least = big; hid = h; P = Q; }
  }
  if (hid < 0) return 0;
  double (&px)[3][4] = P.px, (&py)[3][4] = P.py, (&p1)[3][5] = P.p1;
  // det = p1_0 (px_1 py_2 - py_1 px_2) - p1_1 (px_0 py_2 - py_0 px_2) + p1_2 (px_0 py_1 - py_0 px_1)
  double p[11];
  BA_P3P_UNROLL
  for (int j = 0; j < 11; ++j) p[j] = 0.0;
  BA_P3P_UNROLL
  for (int t = 0; t < 3; ++t) {
    const int t1 = t == 0 ? 1 : 0, t2 = t == 2 ? 1 : 2;
    double m1[7], m2[7], m3[11];
    tv5_polymul<4, 4>(px[t1], py[t2], m1);
    tv5_polymul<4, 4>(py[t1], px[t2], m2);
    BA_P3P_UNROLL
    for (int j = 0; j < 7; ++j) m1[j] -= m2[j];
    tv5_polymul<7, 5>(m1, p1[t], m3);
    BA_P3P_UNROLL
    for (int j = 0; j < 11; ++j) p[j] += t == 1 ? -m3[j] : m3[j];
  }
  double pmax = 0.0;
  BA_P3P_UNROLL
  for (int j = 0; j < 11; ++j) { const double v = fabs(p[j]); pmax = v > pmax ? v : pmax; }
  if (!(pmax > 0.0 && pmax < HUGE_VAL)) return 0;
  // Fujiwara's bound 2 max_k |p_(10-k) / p_10|^(1/k)
  double bound = 0.0;
  BA_P3P_UNROLL
  for (int k = 1; k <= 10; ++k) {
    const double v = pow(fabs(p[10 - k] / p[10]), 1.0 / k);
    bound = v > bound ? v : bound;
  }
  bound = 2.0 * bound;
  if (!(bound < kTv5RootBound)) bound = kTv5RootBound;   // also a zero leading coefficient (NaN, inf)
  // D[m] = the m-th derivative of p / pmax, 11 coefficients each (zeros above its degree)
  double* D = S;
  {
    double q[11];
    BA_P3P_UNROLL
    for (int j = 0; j < 11; ++j) q[j] = p[j] / pmax;
    for (int m = 0; m <= 10; ++m) {
      BA_P3P_UNROLL
      for (int j = 0; j < 11; ++j) D[(11 * m + j) * st] = q[j];
      BA_P3P_UNROLL
      for (int j = 0; j < 10; ++j) q[j] = (j + 1) * q[j + 1];
      q[10] = 0.0;
    }
  }
  // The real roots of D[10 - d], d = 1 .. 10, between the roots (or their
  // placeholders) of D[10 - d + 1]: on each interval the polynomial is
  // monotonic, so a sign change (v < 0 against v >= 0) brackets its one root;
  // an interval without one hands its upper end on as a placeholder.
  double* bpa = S + (size_t)121 * st;
  double* bpb = S + (size_t)134 * st;
  bpa[0] = -bound; bpa[st] = bound;
  unsigned found = 0u;
  for (int d = 1; d <= 10; ++d) {
    double q[11];
    BA_P3P_UNROLL
    for (int j = 0; j < 11; ++j) q[j] = D[(11 * (10 - d) + j) * st];
    found = 0u;
    bpb[0] = -bound;
    const bool direct = d == 10;   // the last level takes its signs from the determinant itself
    bool neg_a = tv5_eval(q, P, direct, -bound) < 0.0;
    for (int i = 1; i <= d; ++i) {
      const double a = bpa[(i - 1) * st], b = bpa[i * st];
      const bool neg_b = tv5_eval(q, P, direct, b) < 0.0;
      double r = b;
      if (neg_a != neg_b) { r = tv5_bisect(q, P, direct, a, b, neg_a); found |= 1u << i; }
      bpb[i * st] = r;
      neg_a = neg_b;
    }
    bpb[(d + 1) * st] = bound;
    double* t = bpa; bpa = bpb; bpb = t;
  }
  // x, y from the null vector of [px py p1](z): the cross product of the two
  // rows whose third component is the largest (ties: (0,1), (0,2), (1,2))
  int n_sol = 0;
  for (int i = 1; i <= 10; ++i) {
    if (!((found >> i) & 1u)) continue;
    const double z = bpa[i * st];
    double a[3][3];
    tv5_rows_at(P, z, a);
    double c01[3], c02[3], c12[3];
    tv_cross(a[0], a[1], c01);
    tv_cross(a[0], a[2], c02);
    tv_cross(a[1], a[2], c12);
    double cx = c01[0], cy = c01[1], cw = c01[2];
    if (fabs(c02[2]) > fabs(cw)) { cx = c02[0]; cy = c02[1]; cw = c02[2]; }
    if (fabs(c12[2]) > fabs(cw)) { cx = c12[0]; cy = c12[1]; cw = c12[2]; }
    double v[3], E[9];
    v[hid] = cx / cw; v[hid == 2 ? 0 : hid + 1] = cy / cw; v[hid == 0 ? 2 : hid - 1] = z;
    tv5_polish(B, st, v, E);
    tv_unit9(E);
    if (!tv_finite9(E)) continue;
    BA_P3P_UNROLL
    for (int e = 0; e < 9; ++e) out[n_sol * sol_stride + e] = E[e];
    ++n_sol;
  }
  return n_sol;
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
