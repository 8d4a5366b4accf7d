// ba_p3p.h — the sampler and the minimal solver of ba_pnp_ransac
// (include/ba_hip.h), written once for the device (ba_pnp.hip) and for host
// programs (tests/cpp/pnp_host.cpp): plain C++ with no HIP dependency beyond
// the __host__ __device__ qualifiers, which vanish under a host compiler.
//
// Sampler: the pinned rule of the header (splitmix64 finaliser, multiply-shift
// range reduction, three distinct local observation indices).
//
// Solver: P3P in fp64 by elimination on the distance ratios.  With unit
// bearings f_i, world points X_i, c_ij = f_i . f_j, D_ij = |X_i - X_j|^2 and
// the unknown distances s_i (camera point P_i = s_i f_i), put u = s_2 / s_1,
// v = s_3 / s_1.  The three law-of-cosines equations give two conics in (u, v)
//   A: (D23 - D12) u^2 + (2 D12 c23 v - 2 D23 c12) u + (D23 - D12 v^2) = 0
//   B: -D13 u^2 + 2 D13 c23 v u + (D23 (1 + v^2 - 2 v c13) - D13 v^2) = 0
// both quadratic in u: a2 u^2 + a1(v) u + a0(v), b2 u^2 + b1(v) u + b0(v).
// Their resultant (a2 b0 - a0 b2)^2 - (a2 b1 - a1 b2)(a1 b0 - a0 b1) is a
// quartic in v; the common root is u = -(a2 b0 - a0 b2) / (a2 b1 - a1 b2).
// The quartic is solved in closed form: a real root y of the resolvent cubic
// (the largest; Cardano / the trigonometric form, two Newton steps) splits it
// into two real quadratics (x^2 + p1 x + q1)(x^2 + p2 x + q2), p = a/2 +- g,
// q = y/2 +- h; each real root takes two Newton steps on the quartic.  The
// roots are sorted increasingly: THE ORDER OF A HYPOTHESIS'S SOLUTIONS IS
// INCREASING v = s_3 / s_1 of the quartic root they come from.  Every
// candidate (u, v) > 0 gives s_1 from the better conditioned of equations 1
// and 2, and (s_1, s_2, s_3) is polished by five Newton steps on the three
// distance equations; a candidate is kept iff the polished distances are
// positive and satisfy the equations to 1e-10 of D12 + D13 + D23.  The pose
// is the rigid motion between the orthonormal triads of the two triangles
// (e1 along 1->2, e3 the normal), t from the centroids; solutions that do not
// put all three points at positive depth are dropped.  Slightly negative
// discriminants (a double root split by rounding) are clamped to zero, so a
// candidate may appear twice; duplicates are harmless to the vote.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BA_P3P_HD __host__ __device__
#define BA_P3P_UNROLL _Pragma("unroll")
#else
#define BA_P3P_HD
#define BA_P3P_UNROLL
#endif

namespace bahip {

// ---------------------------------------------------------------------------
// sampler
// ---------------------------------------------------------------------------
BA_P3P_HD inline uint64_t pnp_mix(uint64_t z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
// draw j of hypothesis h in [0, m)
BA_P3P_HD inline uint32_t pnp_draw(uint64_t seed, uint32_t h, uint32_t j, uint32_t m) {
  const uint64_t z = pnp_mix(seed + (4ull * h + j + 1ull) * 0x9E3779B97F4A7C15ull);
  return (uint32_t)(((z >> 32) * (uint64_t)m) >> 32);
}
// three distinct local observation indices of hypothesis h among n >= 3
BA_P3P_HD inline void pnp_sample(uint64_t seed, uint32_t h, int n, int s[3]) {
  const int a = (int)pnp_draw(seed, h, 0, (uint32_t)n);
  int b = (int)pnp_draw(seed, h, 1, (uint32_t)(n - 1));
  if (b >= a) ++b;
  int c = (int)pnp_draw(seed, h, 2, (uint32_t)(n - 2));
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  if (c >= lo) ++c;
  if (c >= hi) ++c;
  s[0] = a; s[1] = b; s[2] = c;
}

// ---------------------------------------------------------------------------
// bearings
// ---------------------------------------------------------------------------
// inverse of a col-major 3x3 (K[c * 3 + r]) by cofactors, col-major
BA_P3P_HD inline void p3p_inv3(const double K[9], double Ki[9]) {
  const double a = K[0], d = K[1], g = K[2], b = K[3], e = K[4], h = K[5], c = K[6], f = K[7], i = K[8];
  // rows: (a b c) (d e f) (g h i)
  const double A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
  const double det = a * A + b * B + c * C, r = 1.0 / det;
  Ki[0] = A * r;                  Ki[3] = -(b * i - c * h) * r;  Ki[6] = (b * f - c * e) * r;
  Ki[1] = B * r;                  Ki[4] = (a * i - c * g) * r;   Ki[7] = -(a * f - c * d) * r;
  Ki[2] = C * r;                  Ki[5] = -(a * h - b * g) * r;  Ki[8] = (a * e - b * d) * r;
}
// unit bearing K^-1 [u, v, 1]
BA_P3P_HD inline void p3p_bearing(const double Ki[9], double u, double v, double f[3]) {
  const double x = Ki[0] * u + Ki[3] * v + Ki[6], y = Ki[1] * u + Ki[4] * v + Ki[7], z = Ki[2] * u + Ki[5] * v + Ki[8];
  const double r = 1.0 / sqrt(x * x + y * y + z * z);
  f[0] = x * r; f[1] = y * r; f[2] = z * r;
}

// ---------------------------------------------------------------------------
// polynomial roots
// ---------------------------------------------------------------------------
// largest real root of y^3 + A y^2 + B y + C
BA_P3P_HD inline double p3p_cubic_largest(double A, double B, double C) {
  const double third = 1.0 / 3.0;
  const double P = B - A * A * third, Q = (2.0 * A * A * A) / 27.0 - A * B * third + C;
  const double disc = 0.25 * Q * Q + (P * P * P) / 27.0;
  double z;
  if (disc > 0.0) {
    const double sq = sqrt(disc);
    const double w = Q > 0.0 ? -0.5 * Q - sq : -0.5 * Q + sq;   // the larger magnitude: no cancellation
    const double cw = cbrt(w);
    z = cw != 0.0 ? cw - P / (3.0 * cw) : 0.0;
  } else if (P < 0.0) {
    const double m = 2.0 * sqrt(-P * third);
    double arg = (3.0 * Q) / (P * m);
    arg = arg > 1.0 ? 1.0 : (arg < -1.0 ? -1.0 : arg);
    z = m * cos(acos(arg) * third);
  } else {
    z = 0.0;   // P == 0 and Q == 0
  }
  double y = z - A * third;
  for (int it = 0; it < 2; ++it) {
    const double fy = ((y + A) * y + B) * y + C, dy = (3.0 * y + 2.0 * A) * y + B;
    const double yn = y - fy / dy;
    if (dy != 0.0 && yn == yn && fabs(yn) < 1.7976931348623157e308) y = yn;
  }
  return y;
}

// real roots of x^2 + p x + q into r[0], r[1] (HUGE_VAL where there is none);
// a discriminant in [-tol, 0) counts as a double root
BA_P3P_HD inline void p3p_quadratic(double p, double q, double* r0, double* r1) {
  const double hp = 0.5 * p;
  double disc = hp * hp - q;
  const double tol = 1e-7 * (hp * hp + fabs(q));
  *r0 = HUGE_VAL; *r1 = HUGE_VAL;
  if (!(disc >= -tol)) return;
  if (disc < 0.0) disc = 0.0;
  const double s = sqrt(disc);
  const double big = hp > 0.0 ? -(hp + s) : -(hp - s);
  *r0 = big;
  *r1 = big != 0.0 ? q / big : 0.0;
}

// real roots of c[4] x^4 + ... + c[0], sorted increasingly, HUGE_VAL padded
BA_P3P_HD inline void p3p_quartic(const double c[5], double r[4]) {
  r[0] = r[1] = r[2] = r[3] = HUGE_VAL;
  if (c[4] == 0.0) return;
  const double i4 = 1.0 / c[4];
  const double a = c[3] * i4, b = c[2] * i4, cc = c[1] * i4, d = c[0] * i4;
  const double y = p3p_cubic_largest(-b, a * cc - 4.0 * d, 4.0 * b * d - a * a * d - cc * cc);
  double g2 = 0.25 * a * a - b + y, h2 = 0.25 * y * y - d;
  if (g2 < 0.0) g2 = 0.0;
  if (h2 < 0.0) h2 = 0.0;
  double g = sqrt(g2), h = sqrt(h2);
  const double cross = 0.5 * a * y - cc;   // = 2 g h with h's sign
  // the relatively larger of g, h from its square, the other (with its sign) from the cross term
  const double gs = 0.25 * a * a + fabs(b) + fabs(y), hs = 0.25 * y * y + fabs(d);
  if (g2 * hs >= h2 * gs) {
    if (g > 0.0) h = cross / (2.0 * g);
  } else {
    g = cross / (2.0 * h);
  }
  p3p_quadratic(0.5 * a + g, 0.5 * y + h, &r[0], &r[1]);
  p3p_quadratic(0.5 * a - g, 0.5 * y - h, &r[2], &r[3]);
  BA_P3P_UNROLL
  for (int k = 0; k < 4; ++k) {
    double x = r[k];
    if (x < HUGE_VAL) {
      for (int it = 0; it < 2; ++it) {
        const double f = (((c[4] * x + c[3]) * x + c[2]) * x + c[1]) * x + c[0];
        const double df = ((4.0 * c[4] * x + 3.0 * c[3]) * x + 2.0 * c[2]) * x + c[1];
        const double xn = x - f / df;
        if (df != 0.0 && xn == xn && fabs(xn) < 1e300) x = xn;
      }
      r[k] = x;
    }
  }
  // sorting network (0,1) (2,3) (0,2) (1,3) (1,2)
#define BA_P3P_CSWAP(i, j) { const double lo = r[i] < r[j] ? r[i] : r[j], hi = r[i] < r[j] ? r[j] : r[i]; r[i] = lo; r[j] = hi; }
  BA_P3P_CSWAP(0, 1) BA_P3P_CSWAP(2, 3) BA_P3P_CSWAP(0, 2) BA_P3P_CSWAP(1, 3) BA_P3P_CSWAP(1, 2)
#undef BA_P3P_CSWAP
}

// ---------------------------------------------------------------------------
// the solver
// ---------------------------------------------------------------------------
BA_P3P_HD inline void p3p_triad(const double P[3][3], double E[3][3]) {   // E[k] = k-th axis
  double a[3], b[3];
  for (int i = 0; i < 3; ++i) { a[i] = P[1][i] - P[0][i]; b[i] = P[2][i] - P[0][i]; }
  const double na = 1.0 / sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
  for (int i = 0; i < 3; ++i) E[0][i] = a[i] * na;
  double n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
  const double nn = 1.0 / sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  for (int i = 0; i < 3; ++i) E[2][i] = n[i] * nn;
  E[1][0] = E[2][1] * E[0][2] - E[2][2] * E[0][1];
  E[1][1] = E[2][2] * E[0][0] - E[2][0] * E[0][2];
  E[1][2] = E[2][0] * E[0][1] - E[2][1] * E[0][0];
}

// World points X[i], unit bearings f[i] of the three sample observations.
// Slot k of R (row-major 3x3) and t holds the solution of the k-th smallest
// quartic root; bit k of the returned mask says whether the slot holds a
// solution.  A hypothesis's solutions are its set slots in increasing k.
BA_P3P_HD inline int p3p_solve(const double X[3][3], const double f[3][3], double R[4][9], double t[4][3]) {
  const double c12 = f[0][0] * f[1][0] + f[0][1] * f[1][1] + f[0][2] * f[1][2];
  const double c13 = f[0][0] * f[2][0] + f[0][1] * f[2][1] + f[0][2] * f[2][2];
  const double c23 = f[1][0] * f[2][0] + f[1][1] * f[2][1] + f[1][2] * f[2][2];
  double d12 = 0.0, d13 = 0.0, d23 = 0.0;
  for (int i = 0; i < 3; ++i) {
    const double e12 = X[0][i] - X[1][i], e13 = X[0][i] - X[2][i], e23 = X[1][i] - X[2][i];
    d12 += e12 * e12; d13 += e13 * e13; d23 += e23 * e23;
  }
  const double dsum = d12 + d13 + d23;
  if (!(d12 > 0.0 && d13 > 0.0 && d23 > 0.0 && dsum < 1.7976931348623157e308)) return 0;
  const double sc = 1.0 / dsum;
  const double D12 = d12 * sc, D13 = d13 * sc, D23 = d23 * sc;
  // the two conics as polynomials in v (low to high)
  const double a2 = D23 - D12, b2 = -D13;
  const double a1[2] = {-2.0 * D23 * c12, 2.0 * D12 * c23};
  const double a0[3] = {D23, 0.0, -D12};
  const double b1[2] = {0.0, 2.0 * D13 * c23};
  const double b0[3] = {D23, -2.0 * D23 * c13, D23 - D13};
  double p[3], q[2], s[4];
  for (int i = 0; i < 3; ++i) p[i] = a2 * b0[i] - a0[i] * b2;
  for (int i = 0; i < 2; ++i) q[i] = a2 * b1[i] - a1[i] * b2;
  s[0] = a1[0] * b0[0] - a0[0] * b1[0];
  s[1] = a1[0] * b0[1] + a1[1] * b0[0] - a0[0] * b1[1] - a0[1] * b1[0];
  s[2] = a1[0] * b0[2] + a1[1] * b0[1] - a0[1] * b1[1] - a0[2] * b1[0];
  s[3] = a1[1] * b0[2] - a0[2] * b1[1];
  double c[5];
  c[0] = p[0] * p[0] - q[0] * s[0];
  c[1] = 2.0 * p[0] * p[1] - q[0] * s[1] - q[1] * s[0];
  c[2] = 2.0 * p[0] * p[2] + p[1] * p[1] - q[0] * s[2] - q[1] * s[1];
  c[3] = 2.0 * p[1] * p[2] - q[0] * s[3] - q[1] * s[2];
  c[4] = p[2] * p[2] - q[1] * s[3];
  double root[4];
  p3p_quartic(c, root);

  // world triad and centroid (shared by the solutions)
  double Ew[3][3], cw[3];
  p3p_triad(X, Ew);
  for (int i = 0; i < 3; ++i) cw[i] = (X[0][i] + X[1][i] + X[2][i]) / 3.0;

  int mask = 0;
  BA_P3P_UNROLL
  for (int k = 0; k < 4; ++k) {
    const double v = root[k];
    if (!(v > 0.0 && v < HUGE_VAL)) continue;
    const double Pv = (p[2] * v + p[1]) * v + p[0], q0 = q[0], q1v = q[1] * v, Qv = q0 + q1v;
    double u;
    if (fabs(Qv) > 1e-10 * (fabs(q0) + fabs(q1v))) {
      u = -Pv / Qv;
    } else {
      // the linear relation degenerates: B's roots in u, the one that fits A
      const double B1 = b1[1] * v, B0 = (b0[2] * v + b0[1]) * v + b0[0];
      double u0, u1;
      p3p_quadratic(B1 / b2, B0 / b2, &u0, &u1);
      const double A1 = a1[1] * v + a1[0], A0 = a0[2] * v * v + a0[0];
      const double f0 = fabs((a2 * u0 + A1) * u0 + A0), f1 = fabs((a2 * u1 + A1) * u1 + A0);
      u = (u0 > 0.0 && u0 < HUGE_VAL && (!(u1 > 0.0 && u1 < HUGE_VAL) || f0 <= f1)) ? u0 : u1;
    }
    if (!(u > 0.0 && u < HUGE_VAL)) continue;
    const double e1 = 1.0 + u * u - 2.0 * u * c12, e2 = 1.0 + v * v - 2.0 * v * c13;
    double s1 = e1 >= e2 ? sqrt(d12 / e1) : sqrt(d13 / e2);
    double s2 = u * s1, s3 = v * s1;
    // Newton on the three distance equations
    for (int it = 0; it < 5; ++it) {
      const double F1 = s1 * s1 + s2 * s2 - 2.0 * s1 * s2 * c12 - d12;
      const double F2 = s1 * s1 + s3 * s3 - 2.0 * s1 * s3 * c13 - d13;
      const double F3 = s2 * s2 + s3 * s3 - 2.0 * s2 * s3 * c23 - d23;
      const double j11 = 2.0 * (s1 - s2 * c12), j12 = 2.0 * (s2 - s1 * c12);
      const double j21 = 2.0 * (s1 - s3 * c13), j23 = 2.0 * (s3 - s1 * c13);
      const double j32 = 2.0 * (s2 - s3 * c23), j33 = 2.0 * (s3 - s2 * c23);
      // J = [j11 j12 0; j21 0 j23; 0 j32 j33]
      const double det = -j11 * j23 * j32 - j12 * j21 * j33;
      const double x1 = (-F1 * j23 * j32 - j12 * (F2 * j33 - j23 * F3)) / det;
      const double x2 = (j11 * (F2 * j33 - j23 * F3) - F1 * j21 * j33) / det;
      const double x3 = (j11 * (-F2 * j32) - j12 * j21 * F3 + F1 * j21 * j32) / det;
      if (det != 0.0 && x1 == x1 && x2 == x2 && x3 == x3) { s1 -= x1; s2 -= x2; s3 -= x3; }
    }
    const double F1 = s1 * s1 + s2 * s2 - 2.0 * s1 * s2 * c12 - d12;
    const double F2 = s1 * s1 + s3 * s3 - 2.0 * s1 * s3 * c13 - d13;
    const double F3 = s2 * s2 + s3 * s3 - 2.0 * s2 * s3 * c23 - d23;
    const double tolF = 1e-10 * dsum;
    if (!(s1 > 0.0 && s2 > 0.0 && s3 > 0.0 && fabs(F1) <= tolF && fabs(F2) <= tolF && fabs(F3) <= tolF)) continue;
    double P[3][3], Ec[3][3];
    for (int i = 0; i < 3; ++i) { P[0][i] = s1 * f[0][i]; P[1][i] = s2 * f[1][i]; P[2][i] = s3 * f[2][i]; }
    if (!(P[0][2] > 0.0 && P[1][2] > 0.0 && P[2][2] > 0.0)) continue;
    p3p_triad(P, Ec);
    double* Rk = R[k];
    for (int r = 0; r < 3; ++r)
      for (int cc = 0; cc < 3; ++cc) Rk[3 * r + cc] = Ec[0][r] * Ew[0][cc] + Ec[1][r] * Ew[1][cc] + Ec[2][r] * Ew[2][cc];
    bool fin = true;
    for (int r = 0; r < 3; ++r) {
      const double cp = (P[0][r] + P[1][r] + P[2][r]) / 3.0;
      t[k][r] = cp - (Rk[3 * r] * cw[0] + Rk[3 * r + 1] * cw[1] + Rk[3 * r + 2] * cw[2]);
      fin = fin && t[k][r] == t[k][r] && fabs(t[k][r]) < HUGE_VAL;
    }
    for (int e = 0; e < 9; ++e) fin = fin && Rk[e] == Rk[e];
    if (fin) mask |= 1 << k;
  }
  return mask;
}

// ceres::RotationMatrixToAngleAxis (host/ba_geometry.hpp states it) on a
// row-major R
BA_P3P_HD inline void p3p_rotation_to_angle_axis(const double R[9], double w[3]) {
  double q0, q1, q2, q3;
  const double r00 = R[0], r01 = R[1], r02 = R[2], r10 = R[3], r11 = R[4], r12 = R[5], r20 = R[6], r21 = R[7], r22 = R[8];
  const double trace = r00 + r11 + r22;
  if (trace >= 0.0) {
    double tt = sqrt(trace + 1.0);
    q0 = 0.5 * tt;
    tt = 0.5 / tt;
    q1 = (r21 - r12) * tt; q2 = (r02 - r20) * tt; q3 = (r10 - r01) * tt;
  } else {
    int i = 0;
    if (r11 > r00) i = 1;
    if (r22 > (i == 0 ? r00 : r11)) i = 2;
    if (i == 0) {
      double tt = sqrt(r00 - r11 - r22 + 1.0);
      q1 = 0.5 * tt; tt = 0.5 / tt;
      q0 = (r21 - r12) * tt; q2 = (r10 + r01) * tt; q3 = (r20 + r02) * tt;
    } else if (i == 1) {
      double tt = sqrt(r11 - r22 - r00 + 1.0);
      q2 = 0.5 * tt; tt = 0.5 / tt;
      q0 = (r02 - r20) * tt; q3 = (r21 + r12) * tt; q1 = (r01 + r10) * tt;
    } else {
      double tt = sqrt(r22 - r00 - r11 + 1.0);
      q3 = 0.5 * tt; tt = 0.5 / tt;
      q0 = (r10 - r01) * tt; q1 = (r02 + r20) * tt; q2 = (r12 + r21) * tt;
    }
  }
  const double sin_sq = q1 * q1 + q2 * q2 + q3 * q3;
  double kk = 2.0;
  if (sin_sq > 0.0) {
    const double sin_theta = sqrt(sin_sq), cos_theta = q0;
    const double two_theta = 2.0 * (cos_theta < 0.0 ? atan2(-sin_theta, -cos_theta) : atan2(sin_theta, cos_theta));
    kk = two_theta / sin_theta;
  }
  w[0] = q1 * kk; w[1] = q2 * kk; w[2] = q3 * kk;
}

}  // namespace bahip
