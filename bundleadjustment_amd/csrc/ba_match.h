// ba_match.h — the pinned arithmetic of ba_match_descriptors (include/ba_hip.h),
// written once for the device (ba_match.hip) and for host programs
// (tests/cpp/match_host.cpp): plain C++ with no HIP dependency beyond the
// __host__ __device__ qualifiers.
//
// Distance.  Everything is float32.  dot(q, t) is the chain acc = fmaf(q_k,
// t_k, acc) over k ascending from 0: one rounding per term, and the very
// chain v_mfma_f32_32x32x2_f32 evaluates when its accumulator is carried
// through the k steps in order, so the matrix cores and this loop give the
// same bits.  d2 = fmaf(-2, dot, nrm(q) + nrm(t)) clamped at 0 with x > 0 ? x
// : 0 (which also pins the sign of a zero).  For t == q the three chains are
// one chain, nrm + nrm = 2 nrm is exact and so is the fma: d2 = 0.  The root
// is taken in double and rounded to float: 53 bits are more than twice 24
// plus two, so that is the correctly rounded float root whatever the
// compiler's float sqrt is.
//
// Order.  d2 >= 0, so its bit pattern orders like its value; the key
// bits(d2) << 32 | index orders by distance, then by index.  A top-2 list is
// its two smallest keys (kMatchNone past the end); lists over disjoint index
// sets merge exactly, whatever the grouping.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BA_MATCH_HD __host__ __device__
#else
#define BA_MATCH_HD
#endif

namespace bahip {

constexpr uint64_t kMatchNone = ~0ull;   // above every key: bits(d2) <= bits(+inf)

BA_MATCH_HD inline float match_dot(const float* q, const float* t, int dim) {
  float acc = 0.0f;
  for (int k = 0; k < dim; ++k) acc = fmaf(q[k], t[k], acc);
  return acc;
}

BA_MATCH_HD inline float match_d2(float dot, float nrm_q, float nrm_t) {
  const float s = nrm_q + nrm_t;
  const float x = fmaf(-2.0f, dot, s);
  return x > 0.0f ? x : 0.0f;
}

BA_MATCH_HD inline float match_sqrt(float d2) { return (float)sqrt((double)d2); }

BA_MATCH_HD inline uint32_t match_bits(float v) {
  uint32_t u;
  memcpy(&u, &v, sizeof u);
  return u;
}
BA_MATCH_HD inline float match_float(uint32_t u) {
  float v;
  memcpy(&v, &u, sizeof v);
  return v;
}
BA_MATCH_HD inline uint64_t match_key(float d2, uint32_t index) { return ((uint64_t)match_bits(d2) << 32) | index; }

struct MatchTop2 { uint64_t k0, k1; };   // k0 <= k1

BA_MATCH_HD inline void match_push(MatchTop2& a, uint64_t key) {
  if (key < a.k0) { a.k1 = a.k0; a.k0 = key; }
  else if (key < a.k1) a.k1 = key;
}
// two lists over disjoint index sets
BA_MATCH_HD inline MatchTop2 match_merge(const MatchTop2& a, const MatchTop2& b) {
  MatchTop2 r;
  if (a.k0 < b.k0) { r.k0 = a.k0; r.k1 = a.k1 < b.k0 ? a.k1 : b.k0; }
  else { r.k0 = b.k0; r.k1 = b.k1 < a.k0 ? b.k1 : a.k0; }
  return r;
}

// the dense record of one query: index -1 and d2 = +inf where there is no neighbour
struct MatchKnn { int32_t idx0, idx1; float d2_0, d2_1; };
BA_MATCH_HD inline MatchKnn match_knn_record(const MatchTop2& a) {
  MatchKnn r;
  r.idx0 = a.k0 == kMatchNone ? -1 : (int32_t)(uint32_t)a.k0;
  r.idx1 = a.k1 == kMatchNone ? -1 : (int32_t)(uint32_t)a.k1;
  r.d2_0 = a.k0 == kMatchNone ? INFINITY : match_float((uint32_t)(a.k0 >> 32));
  r.d2_1 = a.k1 == kMatchNone ? INFINITY : match_float((uint32_t)(a.k1 >> 32));
  return r;
}

// Lowe's ratio test and the distance cap
BA_MATCH_HD inline bool match_survives(const MatchKnn& r, float ratio, float max_distance) {
  if (r.idx1 < 0) return false;
  const float d0 = match_sqrt(r.d2_0), d1 = match_sqrt(r.d2_1);
  const float bound = ratio * d1;
  return d0 < bound && d0 <= max_distance;
}

}  // namespace bahip
