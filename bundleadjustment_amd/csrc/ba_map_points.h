// ba_map_points.h — the pinned arithmetic of ba_map_points_update and
// ba_associate (include/ba_hip.h), written once for the device
// (ba_map_points.hip) and for host programs (tests/cpp/map_points_host.cpp):
// plain C++ behind __host__ __device__.
//
// Descriptor distances are ba_match.h's (match_dot, match_d2, match_sqrt) and
// are not restated.  The geometry is float with every operation rounded to
// nearest on its own, sums in the written order (ba_accept.h's operation
// orders: matrix-vector products accumulated column by column, norms as
// sqrt((x*x + y*y) + z*z)), IEEE division and square root.  It is written
// with the primitives below and not with ba_accept.h's functions, because the
// result bits are output here and must not depend on the compiler:
//   - a product never fuses with the sum it feeds.  On the device the
//     __f*_rn intrinsics are plain operators to this compiler, which may
//     contract them into FMAs, so mp_mul passes its product through an empty
//     asm; a host program is built with -ffp-contract=off;
//   - quotients and roots are formed in double and rounded to float: 53 bits
//     are more than twice 24 plus two, so that is the correctly rounded float
//     result whatever a float division or square root compiles to (the
//     device's __fsqrt_rn is the native instruction, within an ulp of IEEE).
//
// Selection.  D >= 0, so bits(D) orders like D.  The row median is an order
// statistic on the keys bits(D[i][j]) << 32 | j; its value is found either by
// counting, per key, the keys before it (mp_key_before) or, digit by digit,
// as the largest pattern with at most k values below it (mp_select_bits): the
// two agree on the value whatever the ties.
#pragma once
#include <limits.h>

#include "ba_match.h"
#include "../../include/ba_hip.h"

#define BA_MP_HD BA_MATCH_HD

namespace bahip {

BA_MP_HD inline float mp_add(float a, float b) { return a + b; }
BA_MP_HD inline float mp_sub(float a, float b) { return a - b; }
BA_MP_HD inline float mp_mul(float a, float b) {
  float p = a * b;
#if defined(__HIP_DEVICE_COMPILE__)
  asm("" : "+v"(p));   // the rounded product is all a later sum sees
#endif
  return p;
}
BA_MP_HD inline float mp_div(float a, float b) { return (float)((double)a / (double)b); }
BA_MP_HD inline float mp_sqrt(float a) { return match_sqrt(a); }

// ---- descriptor distance between two rows whose norms are known
BA_MP_HD inline float mp_distance(const float* a, const float* b, float nrm_a, float nrm_b, int dim) {
  return match_sqrt(match_d2(match_dot(a, b, dim), nrm_a, nrm_b));
}

// ---- the rank of the row median: curDistances[(n / 2.0) - 1] after truncation
BA_MP_HD inline int mp_rank(int n) { return n / 2 - 1 > 0 ? n / 2 - 1 : 0; }

// key (bits_t, t) < key (bits_j, j)
BA_MP_HD inline bool mp_key_before(uint32_t bits_t, int t, uint32_t bits_j, int j) {
  return bits_t < bits_j || (bits_t == bits_j && t < j);
}

// The k-th smallest (0-based) of a multiset of bit patterns, given a function
// that counts the values below a pattern: the largest x with count(< x) <= k.
template <class CountBelow>
BA_MP_HD inline uint32_t mp_select_bits(int k, CountBelow count_below) {
  uint32_t x = 0;
  for (int b = 31; b >= 0; --b) {
    const uint32_t trial = x | (1u << b);
    if (count_below(trial) <= k) x = trial;
  }
  return x;
}

// ---- the choice: the smaller key wins, the lower index on equal values
// BA_MP_MEDIAN_REFERENCE: t = (int32_t)m truncated (INT_MAX from 2^31 on); BA_MP_MEDIAN_FLOAT: bits(m)
BA_MP_HD inline int32_t mp_trunc(float m) { return m >= 2147483648.0f ? INT_MAX : (int32_t)m; }
BA_MP_HD inline uint64_t mp_choice_key(float m, int i, int rule) {
  const uint32_t hi = rule == BA_MP_MEDIAN_FLOAT ? match_bits(m) : (uint32_t)mp_trunc(m);
  return ((uint64_t)hi << 32) | (uint32_t)i;
}

// ---- geometry
// u = v.normalized() for v = X - c (Eigen: v / sqrt(squaredNorm) when that is positive)
BA_MP_HD inline void mp_view_unit(const float* c, const float* X, float (&u)[3]) {
  const float v0 = mp_sub(X[0], c[0]), v1 = mp_sub(X[1], c[1]), v2 = mp_sub(X[2], c[2]);
  const float s = mp_add(mp_add(mp_mul(v0, v0), mp_mul(v1, v1)), mp_mul(v2, v2));
  if (s > 0.0f) {
    const float r = mp_sqrt(s);
    u[0] = mp_div(v0, r); u[1] = mp_div(v1, r); u[2] = mp_div(v2, r);
  } else {
    u[0] = v0; u[1] = v1; u[2] = v2;
  }
}
BA_MP_HD inline float mp_dot3(const float* a, const float* b) {
  return mp_add(mp_add(mp_mul(a[0], b[0]), mp_mul(a[1], b[1])), mp_mul(a[2], b[2]));
}

// |X - c|: acc_world_dist's operation order, the root by mp_sqrt
BA_MP_HD inline float mp_world_dist(const float* c, const float* X) {
  const float d0 = mp_sub(X[0], c[0]), d1 = mp_sub(X[1], c[1]), d2 = mp_sub(X[2], c[2]);
  return mp_sqrt(mp_add(mp_add(mp_mul(d0, d0), mp_mul(d1, d1)), mp_mul(d2, d2)));
}
// v = extr * [X; 1] (col-major 4x4), column by column
BA_MP_HD inline void mp_cam_h(const float* e, const float* X, float (&v)[4]) {
  for (int i = 0; i < 4; ++i)
    v[i] = mp_add(mp_add(mp_add(mp_mul(e[i], X[0]), mp_mul(e[4 + i], X[1])), mp_mul(e[8 + i], X[2])), e[12 + i]);
}
// (K * c).hnormalized() (col-major 3x3), column by column
BA_MP_HD inline void mp_pixel(const float* k, float cx, float cy, float cz, float& px, float& py) {
  float q[3];
  for (int i = 0; i < 3; ++i) q[i] = mp_add(mp_add(mp_mul(k[i], cx), mp_mul(k[3 + i], cy)), mp_mul(k[6 + i], cz));
  px = mp_div(q[0], q[2]);
  py = mp_div(q[1], q[2]);
}

// max_dist, min_dist of a point from its reference observation
BA_MP_HD inline void mp_depth_bounds(const float* c_ref, const float* X, float scale, float max_scale, float& min_dist,
                                     float& max_dist) {
  max_dist = mp_mul(mp_world_dist(c_ref, X), scale);
  min_dist = mp_div(max_dist, max_scale);
}

BA_MP_HD inline float mp_inv_sigma(float scale) { return (float)(1.0 / (double)scale); }

// ---- ba_associate: one item.  The descriptor rows are walked by the caller's
// thread: item row, current row (null: not observed), the point's descriptor.
BA_MP_HD inline ba_assoc_result mp_associate(const float* extr, const float* center, const float* K, int w, int h,
                                             const float* X, const float* view_dir, const float* dist, const float* uv,
                                             float scale, const float* row, const float* cur_row, const float* pt_desc,
                                             int dim, const ba_assoc_options& o) {
  ba_assoc_result r;
  r.status = BA_AS_BEHIND;
  r.chi = r.cosine = r.world_dist = r.dist_matched = r.dist_current = -1.0f;
  float v[4];
  mp_cam_h(extr, X, v);
  const float cz = mp_div(v[2], v[3]);
  if (cz <= 0.0f) return r;
  const float cx = mp_div(v[0], v[3]), cy = mp_div(v[1], v[3]);
  float px, py;
  mp_pixel(K, cx, cy, cz, px, py);
  r.status = BA_AS_BOUNDS;
  if (px < 0.0f || px >= (float)w || py < 0.0f || py >= (float)h) return r;
  const float e0 = mp_sub(px, uv[0]), e1 = mp_sub(py, uv[1]);
  r.chi = mp_mul(mp_sqrt(mp_add(mp_mul(e0, e0), mp_mul(e1, e1))), mp_inv_sigma(scale));
  r.status = BA_AS_CHI2;
  if (r.chi > o.chi2) return r;
  float u[3];
  mp_view_unit(center, X, u);
  r.cosine = mp_dot3(u, view_dir);
  r.status = BA_AS_ANGLE;
  if (r.cosine < o.min_cos) return r;
  r.world_dist = mp_world_dist(center, X);
  r.status = BA_AS_DEPTH;
  if (r.world_dist > dist[1] || r.world_dist < dist[0]) return r;
  const float nrm_p = match_dot(pt_desc, pt_desc, dim);
  r.dist_matched = mp_distance(row, pt_desc, match_dot(row, row, dim), nrm_p, dim);
  if (!cur_row) {
    r.status = r.dist_matched < o.max_desc_dist ? BA_AS_ADD : BA_AS_DESC;
    return r;
  }
  r.dist_current = mp_distance(cur_row, pt_desc, match_dot(cur_row, cur_row, dim), nrm_p, dim);
  r.status = r.dist_matched < r.dist_current ? BA_AS_REPLACE : BA_AS_WORSE;
  return r;
}

BA_MP_HD inline ba_fuse_result mp_fuse(const float* dir_p, const float* dir_q, const float* desc_p, const float* desc_q,
                                       int dim, const ba_assoc_options& o) {
  ba_fuse_result r;
  r.cosine = mp_dot3(dir_p, dir_q);
  r.dist = -1.0f;
  r.status = BA_FUSE_ANGLE;
  if (r.cosine < o.fuse_min_cos) return r;
  r.dist = mp_distance(desc_p, desc_q, match_dot(desc_p, desc_p, dim), match_dot(desc_q, desc_q, dim), dim);
  r.status = r.dist < o.fuse_max_desc_dist ? BA_FUSE_OK : BA_FUSE_DESC;
  return r;
}

}  // namespace bahip
