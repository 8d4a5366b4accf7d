// ba_map_points.hip — map-point upkeep and the association gates of
// searchInNeighbors (gfx950, wave64).  The arithmetic is pinned in
// ba_map_points.h (distances: ba_match.h).
//
//   k_mp_group<DIM, G>  a group of G lanes per point (G = 16: tracks of up to
//                   16 observations, four points per wave; G = 64: up to 64, a
//                   wave per point).  The wave brings its up to 64 descriptor
//                   rows into LDS with coalesced 16-byte loads (rows DIM + 1
//                   floats apart, k_match_norms' stride: the lanes' walks stay
//                   on different banks).  Lane j of a group owns observation
//                   j: its norm, and for every row i the distance D[i][j],
//                   one serial chain (row i is an LDS broadcast).  The row
//                   median is taken by rank: every lane counts the keys
//                   before its own among the group's (shuffles), and the one
//                   lane that counts k holds m_i.  The choice is a
//                   min-butterfly on integer keys.  Lane j also forms the unit
//                   vector of observation j; the sum over the track is taken
//                   in caller order by shuffles.
//   k_mp_long<DIM>  a workgroup per point for tracks of 65 .. 1024.  D is never
//                   held: a wave forms one row at a time (row i in LDS, the
//                   lane's up to 16 columns read through the caches), keeps
//                   its values in registers and finds the k-th smallest
//                   pattern digit by digit from wave-wide counts.
//   k_associate     one lane per item or fuse pair, in the style of k_prune;
//                   the lane walks its descriptor chains.
// Every float is formed by one lane in a fixed order and every selection is on
// integer keys, so the routes give the same bits.  No atomics.
#include <hip/hip_runtime.h>

#include "ba_kernels.h"
#include "ba_map_points.h"

namespace bahip {

static_assert(sizeof(ba_map_point) == 32, "record");
static_assert(kMpShort == 16 && kMpWave == 64 && BA_MP_MAX_TRACK == 1024, "tiers of k_mp_group / k_mp_long");

__device__ __forceinline__ void mp_write_record(const MapPointsArgs& A, int p, int o0, int n, int best, float median,
                                                float v0, float v1, float v2) {
  ba_map_point r;
  if (n == 0) {
    r.status = BA_MP_EMPTY; r.best = -1; r.median = 0.0f;
    r.view_dir[0] = r.view_dir[1] = r.view_dir[2] = 0.0f; r.min_dist = r.max_dist = 0.0f;
  } else {
    const int ref = A.ref_obs ? A.ref_obs[p] : 0;
    const float scale = A.obs_scale ? A.obs_scale[o0 + ref] : 1.0f;
    r.status = BA_MP_OK; r.best = best; r.median = median;
    const float fn = (float)n;
    r.view_dir[0] = mp_div(v0, fn); r.view_dir[1] = mp_div(v1, fn); r.view_dir[2] = mp_div(v2, fn);
    mp_depth_bounds(A.center + 3 * (size_t)A.obs_cam[o0 + ref], A.pts + 3 * (size_t)p, scale, A.max_scale, r.min_dist,
                    r.max_dist);
  }
  A.out[(size_t)p * A.out_stride] = r;
}

template <int DIM, int G>
__global__ __launch_bounds__(64) void k_mp_group(MapPointsArgs A, int tier) {
  constexpr int LD = DIM + 1, V = DIM / 4;
  __shared__ float rows[64 * LD];
  __shared__ int srow[64];
  const int lane = (int)threadIdx.x, g = lane / G, j = lane % G;
  const int slot = (int)blockIdx.x * (64 / G) + g;
  const bool have = slot < A.count[tier];
  const int p = have ? A.order[A.first[tier] + slot] : 0;
  const int o0 = have ? A.obs_offset[p] : 0;
  const int n = have ? A.obs_offset[p + 1] - o0 : 0;
  const bool mine = j < n;
  srow[lane] = mine ? A.obs_row[o0 + j] : -1;
  __syncthreads();
#pragma unroll 4
  for (int e = lane; e < 64 * V; e += 64) {
    const int r = e / V, k = 4 * (e - r * V), src = srow[r];
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (src >= 0) v = *reinterpret_cast<const float4*>(A.desc + (size_t)src * DIM + k);
    float* o = rows + r * LD + k;
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  }
  __syncthreads();
  int nmax = n;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) nmax = max(nmax, __shfl_xor(nmax, off, 64));
  const float* own = rows + lane * LD;
  const float nrm = match_dot(own, own, DIM);
  const int k = mp_rank(n);
  float m_own = 0.0f;
  for (int i = 0; i < nmax; ++i) {
    const float nrm_i = __shfl(nrm, i, G);
    const bool act = mine && i < n;
    float d = 0.0f;
    if (act) d = mp_distance(rows + (g * G + i) * LD, own, nrm_i, nrm, DIM);
    const uint32_t bits = act ? match_bits(d) : 0xffffffffu;
    int before = 0;
    for (int t = 0; t < nmax; ++t) {
      const uint32_t bt = (uint32_t)__shfl((int)bits, t, G);
      before += (t < n && mp_key_before(bt, t, bits, j)) ? 1 : 0;
    }
    uint32_t mb = (act && before == k) ? bits : 0u;   // exactly one lane of the group
#pragma unroll
    for (int off = 1; off < G; off <<= 1) mb |= (uint32_t)__shfl_xor((int)mb, off, G);
    if (j == i) m_own = match_float(mb);
    if (A.dbg_D && act) A.dbg_D[(size_t)i * n + j] = d;
  }
  if (A.dbg_m && mine) A.dbg_m[j] = m_own;
  unsigned long long key = mine ? mp_choice_key(m_own, j, A.median_rule) : ~0ull;
#pragma unroll
  for (int off = 1; off < G; off <<= 1) {
    const unsigned long long o = __shfl_xor(key, off, G);
    key = o < key ? o : key;
  }
  const int best = n > 0 ? (int)(uint32_t)key : 0;
  const float median = __shfl(m_own, best, G);
  // ---- viewing direction: lane j's unit vector, the sum in caller order
  float u[3] = {0.0f, 0.0f, 0.0f};
  if (mine) mp_view_unit(A.center + 3 * (size_t)A.obs_cam[o0 + j], A.pts + 3 * (size_t)p, u);
  float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
  for (int t = 0; t < nmax; ++t) {
    const float a = __shfl(u[0], t, G), b = __shfl(u[1], t, G), c = __shfl(u[2], t, G);
    if (t < n) { s0 = mp_add(s0, a); s1 = mp_add(s1, b); s2 = mp_add(s2, c); }
  }
  if (have && j == 0) mp_write_record(A, p, o0, n, best, median, s0, s1, s2);
  if (have && A.desc_out) {
    const float* src = rows + (g * G + best) * LD;
    for (int e = j; e < DIM; e += G) A.desc_out[(size_t)p * DIM + e] = n > 0 ? src[e] : 0.0f;
  }
}

template <int DIM>
__global__ __launch_bounds__(256) void k_mp_long(MapPointsArgs A) {
  constexpr int T = BA_MP_MAX_TRACK / 64;   // columns per lane
  __shared__ float row_i[4][DIM];
  __shared__ float nrm[BA_MP_MAX_TRACK], med[BA_MP_MAX_TRACK], su[3][BA_MP_MAX_TRACK];
  __shared__ int srow[BA_MP_MAX_TRACK];
  __shared__ unsigned long long wkey[4];
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int p = A.order[A.first[2] + (int)blockIdx.x];
  const int o0 = A.obs_offset[p], n = min(A.obs_offset[p + 1] - o0, BA_MP_MAX_TRACK);
  for (int t = tid; t < n; t += 256) {
    const int r = A.obs_row[o0 + t];
    const float* x = A.desc + (size_t)r * DIM;
    srow[t] = r;
    nrm[t] = match_dot(x, x, DIM);
    float u[3];
    mp_view_unit(A.center + 3 * (size_t)A.obs_cam[o0 + t], A.pts + 3 * (size_t)p, u);
    su[0][t] = u[0]; su[1][t] = u[1]; su[2][t] = u[2];
  }
  __syncthreads();
  const int k = mp_rank(n);
  for (int i0 = 0; i0 < n; i0 += 4) {   // (the same trip count in every wave)
    const int i = i0 + wave;
    const bool valid = i < n;
    if (valid)
      for (int e = lane; e < DIM; e += 64) row_i[wave][e] = A.desc[(size_t)srow[i] * DIM + e];
    __syncthreads();
    if (valid) {
      uint32_t bits[T];
#pragma unroll
      for (int t = 0; t < T; ++t) {
        const int j = lane + 64 * t;
        bits[t] = 0xffffffffu;
        if (j < n) {
          const float d = mp_distance(row_i[wave], A.desc + (size_t)srow[j] * DIM, nrm[i], nrm[j], DIM);
          bits[t] = match_bits(d);
          if (A.dbg_D) A.dbg_D[(size_t)i * n + j] = d;
        }
      }
      const uint32_t mb = mp_select_bits(k, [&](uint32_t x) {
        int c = 0;
#pragma unroll
        for (int t = 0; t < T; ++t) c += bits[t] < x ? 1 : 0;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) c += __shfl_xor(c, off, 64);
        return c;
      });
      if (lane == 0) med[i] = match_float(mb);
    }
    __syncthreads();
  }
  if (A.dbg_m)
    for (int t = tid; t < n; t += 256) A.dbg_m[t] = med[t];
  unsigned long long key = ~0ull;
  for (int t = tid; t < n; t += 256) {
    const unsigned long long o = mp_choice_key(med[t], t, A.median_rule);
    key = o < key ? o : key;
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long o = __shfl_xor(key, off, 64);
    key = o < key ? o : key;
  }
  if (lane == 0) wkey[wave] = key;
  __syncthreads();
  key = wkey[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) key = wkey[w] < key ? wkey[w] : key;
  const int best = (int)(uint32_t)key;
  if (tid == 0) {
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int t = 0; t < n; ++t) { s0 = mp_add(s0, su[0][t]); s1 = mp_add(s1, su[1][t]); s2 = mp_add(s2, su[2][t]); }
    mp_write_record(A, p, o0, n, best, med[best], s0, s1, s2);
  }
  if (A.desc_out)
    for (int e = tid; e < DIM; e += 256) A.desc_out[(size_t)p * DIM + e] = A.desc[(size_t)srow[best] * DIM + e];
}

void launch_map_points(const MapPointsArgs& A, hipStream_t s) {
  if (A.count[0] > 0) {
    const dim3 g((A.count[0] + 3) / 4);
    if (A.dim == 64) hipLaunchKernelGGL((k_mp_group<64, 16>), g, dim3(64), 0, s, A, 0);
    else hipLaunchKernelGGL((k_mp_group<128, 16>), g, dim3(64), 0, s, A, 0);
  }
  if (A.count[1] > 0) {
    if (A.dim == 64) hipLaunchKernelGGL((k_mp_group<64, 64>), dim3(A.count[1]), dim3(64), 0, s, A, 1);
    else hipLaunchKernelGGL((k_mp_group<128, 64>), dim3(A.count[1]), dim3(64), 0, s, A, 1);
  }
  if (A.count[2] > 0) {
    if (A.dim == 64) hipLaunchKernelGGL(k_mp_long<64>, dim3(A.count[2]), dim3(256), 0, s, A);
    else hipLaunchKernelGGL(k_mp_long<128>, dim3(A.count[2]), dim3(256), 0, s, A);
  }
}

__global__ __launch_bounds__(256) void k_associate(AssocArgs A) {
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const size_t dim = (size_t)A.dim;
  if (t < A.n_items) {
    const int c = A.item_cam[t], p = A.item_pt[t];
    const int cur = A.item_cur_row ? A.item_cur_row[t] : -1;
    A.items[t] = mp_associate(A.extr + 16 * (size_t)c, A.center + 3 * (size_t)c, A.K + 9 * (size_t)c, A.image_size[2 * c],
                              A.image_size[2 * c + 1], A.pts + 3 * (size_t)p, A.pt_view_dir + 3 * (size_t)p,
                              A.pt_dist + 2 * (size_t)p, A.item_uv + 2 * (size_t)t, A.item_scale ? A.item_scale[t] : 1.0f,
                              A.desc + dim * (size_t)A.item_row[t], cur >= 0 ? A.desc + dim * (size_t)cur : nullptr,
                              A.pt_desc + dim * (size_t)p, A.dim, A.opt);
  } else if (t < A.n_items + A.n_fuse) {
    const int f = t - A.n_items, p = A.fuse_pairs[2 * f], q = A.fuse_pairs[2 * f + 1];
    A.fuse[f] = mp_fuse(A.pt_view_dir + 3 * (size_t)p, A.pt_view_dir + 3 * (size_t)q, A.pt_desc + dim * (size_t)p,
                        A.pt_desc + dim * (size_t)q, A.dim, A.opt);
  }
}

void launch_associate(const AssocArgs& A, hipStream_t s) {
  const int n = A.n_items + A.n_fuse;
  if (n <= 0) return;
  hipLaunchKernelGGL(k_associate, dim3((n + 255) / 256), dim3(256), 0, s, A);
}

}  // namespace bahip
