// ba_map_graph.hip — covisibility lists, culling votes and local-BA windows
// of a chunk of query frames (gfx950, wave64).  The rules are pinned in
// ba_map_graph.h; everything is integer counts, integer keys and bitmaps, so
// the results do not depend on the order in which lanes arrive.  A workgroup of
// kMgThreads lanes takes one query in every kernel.
//
//   k_mg_weights  a lane takes one observation of q from the frame-sorted
//                 permutation and walks that point's track: one LDS integer
//                 atomic add per other observation into a histogram over a
//                 column tile of frame indices.  Frame counts beyond the tile
//                 take several passes.  The tile is stored to the W row.
//   k_mg_list     candidates W > th && key, counted; the fallback is an LDS
//                 atomic max on W << 32 | ~g.  The order is found by counting,
//                 per candidate, the candidates whose key is smaller (the row
//                 of candidate weights sits in LDS up to kMgTileMax frames),
//                 and the best frames are the ranks below n_best.
//   k_mg_vote     a lane per observation of q counts the qualifying other
//                 views along the track; integer totals.
//   k_mg_mark     the local frames' observations set the point bitmap
//                 (integer atomicOr on global scratch).
//   k_mg_fixed    the tracks of the marked points set a frame bitmap in LDS
//                 (fixed frames, 65536 frames per pass) and count the window's
//                 points and observations; one lane then forms the prefix
//                 counts of the fixed bitmap.
//   k_mg_fill     after the host has scanned the counts: the lists.  Ascending
//                 order comes from popcount prefix sums over the bitmaps (a
//                 block scan per 256 words); local indices are ranks.
//   k_mg_status   a lane per point.
// No float atomics; every store is an ordinary vector store.
#include <hip/hip_runtime.h>

#include "ba_kernels.h"
#include "ba_map_graph.h"

namespace bahip {

static_assert(sizeof(ba_graph_frame) == 40, "record");
static_assert(sizeof(ba_graph_options) == 40, "options");

namespace {

constexpr int kT = kMgThreads;
constexpr int kFixTile = 65536;          // frames per pass of k_mg_fixed's LDS bitmap (8 KiB)

__device__ __forceinline__ bool mg_outlier(const MapGraphArgs& A, int o) { return A.obs_outlier && A.obs_outlier[o] != 0; }
__device__ __forceinline__ bool mg_invalid(const MapGraphArgs& A, int p) { return A.pt_invalid && A.pt_invalid[p] != 0; }
__device__ __forceinline__ bool mg_key(const MapGraphArgs& A, int g) { return !A.is_key || A.is_key[g] != 0; }
__device__ __forceinline__ int mg_octave(const MapGraphArgs& A, int o) { return A.obs_octave ? A.obs_octave[o] : 0; }
__device__ __forceinline__ size_t mg_fw(const MapGraphArgs& A) { return ((size_t)A.n_frames + 31) / 32; }
__device__ __forceinline__ size_t mg_pw(const MapGraphArgs& A) { return ((size_t)A.n_pts + 31) / 32; }

__global__ __launch_bounds__(kT) void k_mg_weights(MapGraphArgs A) {
  extern __shared__ int hist[];
  const int qi = blockIdx.x, q = A.query[qi], tid = threadIdx.x, nf = A.n_frames, T = A.tile;
  const int i0 = A.frame_off[q], i1 = A.frame_off[q + 1];
  int* Wr = A.W + (size_t)qi * nf;
  for (int t0 = 0; t0 < nf; t0 += T) {
    const int width = min(T, nf - t0);
    for (int j = tid; j < width; j += kT) hist[j] = 0;
    __syncthreads();
    for (int i = i0 + tid; i < i1; i += kT) {
      const int o = A.perm[i];
      if (mg_outlier(A, o)) continue;
      const int p = A.obs_pt[o];
      for (int k = A.obs_offset[p], k1 = A.obs_offset[p + 1]; k < k1; ++k) {
        const int g = A.obs_frame[k];
        if (g != q && (unsigned)(g - t0) < (unsigned)width) atomicAdd(&hist[g - t0], 1);
      }
    }
    __syncthreads();
    for (int j = tid; j < width; j += kT) Wr[t0 + j] = hist[j];
    __syncthreads();
  }
}

__global__ __launch_bounds__(kT) void k_mg_list(MapGraphArgs A) {
  __shared__ int cw[kMgTileMax];          // candidate weight, or -1
  __shared__ int s_cnt;
  __shared__ unsigned long long s_fb;
  const int qi = blockIdx.x, tid = threadIdx.x, nf = A.n_frames;
  const int* Wr = A.W + (size_t)qi * nf;
  const bool in_lds = nf <= kMgTileMax;
  if (tid == 0) { s_cnt = 0; s_fb = 0ull; }
  __syncthreads();
  auto cand = [&](int g) { const int w = Wr[g]; return w > A.th && mg_key(A, g) ? w : -1; };
  int cnt = 0;
  unsigned long long fb = 0ull;
  for (int g = tid; g < nf; g += kT) {
    const int w = Wr[g], c = cand(g);
    if (in_lds) cw[g] = c;
    cnt += c >= 0 ? 1 : 0;
    if (w > 0) fb = max(fb, (unsigned long long)mg_fallback_key(w, g));
  }
  if (cnt) atomicAdd(&s_cnt, cnt);
  if (fb) atomicMax(&s_fb, fb);
  __syncthreads();
  const int degree_c = s_cnt;
  const unsigned long long best_fb = s_fb;
  int* lf = A.lst_f + (size_t)qi * nf;
  int* lw = A.lst_w + (size_t)qi * nf;
  int* bst = A.best + (size_t)qi * BA_WINDOW_MAX_CAMS;
  int status = BA_GRAPH_OK, degree = degree_c;
  if (degree_c == 0) {
    if (best_fb != 0ull) {
      status = BA_GRAPH_FALLBACK; degree = 1;
      if (tid == 0) {
        const int g = (int)(0xffffffffu - (unsigned)best_fb);
        lf[0] = g; lw[0] = Wr[g];
        if (A.n_best > 0) bst[0] = g;
      }
    } else {
      status = BA_GRAPH_ISOLATED;
    }
  } else {
    for (int g = tid; g < nf; g += kT) {
      const int w = in_lds ? cw[g] : cand(g);
      if (w < 0) continue;
      int before = 0, stronger = 0;
      for (int h = 0; h < nf; ++h) {
        const int v = in_lds ? cw[h] : cand(h);
        if (v < 0) continue;
        before += mg_list_key(v, h) < mg_list_key(w, g) ? 1 : 0;
        stronger += mg_stronger(v, h, w, g) ? 1 : 0;
      }
      lf[before] = g; lw[before] = w;
      const int r = A.order == BA_GRAPH_STRONGEST_FIRST ? stronger : before;
      if (r < A.n_best) bst[r] = g;
    }
  }
  if (tid == 0) {
    ba_graph_frame& r = A.rec[qi];
    r.status = status; r.degree = degree; r.max_weight = (int)(best_fb >> 32);
    r.n_local = A.build_windows ? min(A.n_best, degree) + 1 : 0;
    r.n_fixed = 0; r.n_win_pts = 0; r.n_win_obs = 0;
  }
}

__global__ __launch_bounds__(kT) void k_mg_vote(MapGraphArgs A) {
  __shared__ int s_map, s_red;
  const int qi = blockIdx.x, q = A.query[qi], tid = threadIdx.x;
  if (tid == 0) { s_map = 0; s_red = 0; }
  __syncthreads();
  int n_map = 0, n_red = 0;
  for (int i = A.frame_off[q] + tid; i < A.frame_off[q + 1]; i += kT) {
    const int o = A.perm[i], p = A.obs_pt[o];
    if (mg_invalid(A, p)) continue;
    ++n_map;
    const int k0 = A.obs_offset[p], k1 = A.obs_offset[p + 1];
    if (k1 - k0 <= kMgMinTrack) continue;
    const int oct = mg_octave(A, o);
    int views = 0;
    for (int k = k0; k < k1; ++k) views += A.obs_frame[k] != q && mg_view_counts(mg_octave(A, k), oct) ? 1 : 0;
    n_red += views >= kMgMinViews ? 1 : 0;
  }
  if (n_map) atomicAdd(&s_map, n_map);
  if (n_red) atomicAdd(&s_red, n_red);
  __syncthreads();
  if (tid == 0) {
    ba_graph_frame& r = A.rec[qi];
    r.n_map = s_map; r.n_redundant = s_red; r.cull = mg_cull(A.frame_id[q], s_map, s_red, A.fraction);
  }
}

// the local frames of query qi into LDS: the best frames in order, then q
__device__ __forceinline__ int mg_local_frames(const MapGraphArgs& A, int qi, int* s_local) {
  const int nl = A.rec[qi].n_local;
  if ((int)threadIdx.x < nl)
    s_local[threadIdx.x] = (int)threadIdx.x == nl - 1 ? A.query[qi] : A.best[(size_t)qi * BA_WINDOW_MAX_CAMS + threadIdx.x];
  __syncthreads();
  return nl;
}

__global__ __launch_bounds__(kT) void k_mg_mark(MapGraphArgs A) {
  __shared__ int s_local[BA_WINDOW_MAX_CAMS];
  const int qi = blockIdx.x, tid = threadIdx.x;
  const int nl = mg_local_frames(A, qi, s_local);
  unsigned* loc = A.locbits + (size_t)qi * mg_fw(A);
  unsigned* pb = A.ptbits + (size_t)qi * mg_pw(A);
  if (tid < nl) atomicOr(&loc[s_local[tid] >> 5], 1u << (s_local[tid] & 31));
  for (int c = 0; c < nl; ++c) {
    const int f = s_local[c];
    for (int i = A.frame_off[f] + tid; i < A.frame_off[f + 1]; i += kT) {
      const int o = A.perm[i];
      if (mg_outlier(A, o)) continue;
      const int p = A.obs_pt[o];
      if (mg_invalid(A, p)) continue;
      atomicOr(&pb[p >> 5], 1u << (p & 31));
    }
  }
}

__global__ __launch_bounds__(kT) void k_mg_fixed(MapGraphArgs A) {
  __shared__ unsigned s_fix[kFixTile / 32];
  __shared__ int s_pts, s_obs;
  const int qi = blockIdx.x, tid = threadIdx.x, nf = A.n_frames;
  const size_t fw = mg_fw(A), pw = mg_pw(A);
  const unsigned* loc = A.locbits + (size_t)qi * fw;
  const unsigned* pb = A.ptbits + (size_t)qi * pw;
  unsigned* fix = A.fixbits + (size_t)qi * fw;
  int* pre = A.fixpre + (size_t)qi * fw;
  if (tid == 0) { s_pts = 0; s_obs = 0; }
  int running = 0;   // lane 0: fixed frames before the tile
  for (int f0 = 0; f0 < nf; f0 += kFixTile) {
    const int width = min(kFixTile, nf - f0), words = (width + 31) / 32;
    for (int j = tid; j < words; j += kT) s_fix[j] = 0u;
    __syncthreads();
    int n_pts = 0, n_obs = 0;
    for (size_t w = tid; w < pw; w += kT) {
      unsigned bits = pb[w];
      n_pts += __popc(bits);
      while (bits) {
        const int p = (int)(w * 32) + __ffs(bits) - 1;
        bits &= bits - 1;
        for (int k = A.obs_offset[p], k1 = A.obs_offset[p + 1]; k < k1; ++k) {
          if (mg_outlier(A, k)) continue;
          const int g = A.obs_frame[k];
          if ((loc[g >> 5] >> (g & 31)) & 1u) { ++n_obs; continue; }
          if (!mg_key(A, g)) continue;
          ++n_obs;
          const int j = g - f0;
          if ((unsigned)j < (unsigned)width && !((s_fix[j >> 5] >> (j & 31)) & 1u)) atomicOr(&s_fix[j >> 5], 1u << (j & 31));
        }
      }
    }
    if (f0 == 0) {   // the counts do not depend on the tile
      if (n_pts) atomicAdd(&s_pts, n_pts);
      if (n_obs) atomicAdd(&s_obs, n_obs);
    }
    __syncthreads();
    for (int j = tid; j < words; j += kT) fix[f0 / 32 + j] = s_fix[j];
    if (tid == 0)
      for (int j = 0; j < words; ++j) { pre[f0 / 32 + j] = running; running += __popc(s_fix[j]); }
    __syncthreads();
  }
  if (tid == 0) {
    ba_graph_frame& r = A.rec[qi];
    r.n_fixed = running; r.n_win_pts = s_pts; r.n_win_obs = s_obs;
  }
}

// exclusive scan of one int per lane over the workgroup; *total: the sum
__device__ __forceinline__ int mg_block_scan(int v, int* s, int* total) {
  const int tid = threadIdx.x;
  s[tid] = v;
  __syncthreads();
  for (int d = 1; d < kT; d <<= 1) {
    const int add = tid >= d ? s[tid - d] : 0;
    __syncthreads();
    s[tid] += add;
    __syncthreads();
  }
  const int incl = s[tid];
  *total = s[kT - 1];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(kT) void k_mg_fill(MapGraphArgs A) {
  __shared__ int s_local[BA_WINDOW_MAX_CAMS];
  __shared__ int s_scan[kT];
  const int qi = blockIdx.x, tid = threadIdx.x, nf = A.n_frames;
  const ba_graph_frame r = A.rec[qi];
  const long long* off = A.off + (size_t)qi * 4;
  for (int j = tid; j < r.degree; j += kT) {
    A.nbr_frame[off[0] + j] = A.lst_f[(size_t)qi * nf + j];
    A.nbr_weight[off[0] + j] = A.lst_w[(size_t)qi * nf + j];
  }
  if (!A.build_windows) return;
  const int nl = mg_local_frames(A, qi, s_local);
  const size_t fw = mg_fw(A), pw = mg_pw(A);
  const unsigned* loc = A.locbits + (size_t)qi * fw;
  const unsigned* fix = A.fixbits + (size_t)qi * fw;
  const int* pre = A.fixpre + (size_t)qi * fw;
  const unsigned* pb = A.ptbits + (size_t)qi * pw;
  if (tid < nl) {
    A.win_cam[off[1] + tid] = s_local[tid];
    A.win_cam_fixed[off[1] + tid] = A.frame_id[s_local[tid]] == 0 ? 1 : 0;
  }
  for (size_t w = tid; w < fw; w += kT) {
    unsigned bits = fix[w];
    long long at = off[1] + nl + pre[w];
    while (bits) {
      A.win_cam[at] = (int)(w * 32) + __ffs(bits) - 1;
      A.win_cam_fixed[at] = 1;
      ++at;
      bits &= bits - 1;
    }
  }
  // a camera's index in the window, or -1 when the frame is not in it
  auto cam_of = [&](int g) -> int {
    const unsigned bit = 1u << (g & 31);
    if (loc[g >> 5] & bit) {
      int c = 0;
      while (s_local[c] != g) ++c;
      return c;
    }
    if (fix[g >> 5] & bit) return nl + pre[g >> 5] + __popc(fix[g >> 5] & (bit - 1u));
    return -1;
  };
  int pt_base = 0, obs_base = 0;
  for (size_t wb = 0; wb < pw; wb += kT) {
    const size_t w = wb + tid;
    const unsigned word = w < pw ? pb[w] : 0u;
    int n_obs = 0;
    for (unsigned bits = word; bits; bits &= bits - 1) {
      const int p = (int)(w * 32) + __ffs(bits) - 1;
      for (int k = A.obs_offset[p], k1 = A.obs_offset[p + 1]; k < k1; ++k)
        n_obs += !mg_outlier(A, k) && cam_of(A.obs_frame[k]) >= 0 ? 1 : 0;
    }
    int pt_total, obs_total;
    int pt_at = pt_base + mg_block_scan(__popc(word), s_scan, &pt_total);
    long long obs_at = off[3] + obs_base + mg_block_scan(n_obs, s_scan, &obs_total);
    for (unsigned bits = word; bits; bits &= bits - 1) {
      const int p = (int)(w * 32) + __ffs(bits) - 1;
      A.win_pt[off[2] + pt_at] = p;
      for (int k = A.obs_offset[p], k1 = A.obs_offset[p + 1]; k < k1; ++k) {
        if (mg_outlier(A, k)) continue;
        const int c = cam_of(A.obs_frame[k]);
        if (c < 0) continue;
        A.win_obs[obs_at] = k; A.win_obs_cam[obs_at] = c; A.win_obs_pt[obs_at] = pt_at;
        ++obs_at;
      }
      ++pt_at;
    }
    pt_base += pt_total; obs_base += obs_total;
  }
}

__global__ __launch_bounds__(kT) void k_mg_status(MapGraphArgs A, const int* pt_ref_frame, int current_frame_id,
                                                  uint8_t* pt_status) {
  const int p = blockIdx.x * kT + threadIdx.x;
  if (p >= A.n_pts) return;
  pt_status[p] = mg_point_status(mg_invalid(A, p), (int64_t)current_frame_id - A.frame_id[pt_ref_frame[p]],
                                 A.obs_offset[p + 1] - A.obs_offset[p]);
}

}  // namespace

void launch_map_graph_weights(const MapGraphArgs& A, hipStream_t s) {
  if (A.n_chunk == 0 || A.n_frames == 0) return;
  hipLaunchKernelGGL(k_mg_weights, dim3(A.n_chunk), dim3(kT), sizeof(int) * (size_t)A.tile, s, A);
}

void launch_map_graph_count(const MapGraphArgs& A, hipStream_t s) {
  if (A.n_chunk == 0) return;
  launch_map_graph_weights(A, s);
  hipLaunchKernelGGL(k_mg_list, dim3(A.n_chunk), dim3(kT), 0, s, A);
  hipLaunchKernelGGL(k_mg_vote, dim3(A.n_chunk), dim3(kT), 0, s, A);
  if (!A.build_windows) return;
  hipLaunchKernelGGL(k_mg_mark, dim3(A.n_chunk), dim3(kT), 0, s, A);
  hipLaunchKernelGGL(k_mg_fixed, dim3(A.n_chunk), dim3(kT), 0, s, A);
}

void launch_map_graph_fill(const MapGraphArgs& A, hipStream_t s) {
  if (A.n_chunk == 0) return;
  hipLaunchKernelGGL(k_mg_fill, dim3(A.n_chunk), dim3(kT), 0, s, A);
}

void launch_map_graph_status(const MapGraphArgs& A, const int* pt_ref_frame, int current_frame_id, uint8_t* pt_status,
                             hipStream_t s) {
  if (A.n_pts == 0) return;
  hipLaunchKernelGGL(k_mg_status, dim3((A.n_pts + kT - 1) / kT), dim3(kT), 0, s, A, pt_ref_frame, current_frame_id, pt_status);
}

}  // namespace bahip
