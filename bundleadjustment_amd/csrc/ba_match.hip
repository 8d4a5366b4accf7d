// ba_match.hip — batched descriptor matching (gfx950, wave64): the exact 2-NN
// of every query on the f32 matrix cores, Lowe's ratio test, the
// one-match-per-train filter and the compaction in train order
// (FeatureProcessor::matchFeatures, FeatureProcessor.cpp:39-95).  The
// arithmetic is pinned in ba_match.h.
//
//   k_match_norms   one lane per descriptor (and reference descriptor): nrm(x),
//                   the fmaf chain over its row, read from an LDS copy that
//                   the wave fills with coalesced loads.
//   k_match_nn      grid (pair, query tile of 128, train chunk), four waves.
//                   A wave owns 32 queries and keeps their rows in registers
//                   as the A operand of v_mfma_f32_32x32x2_f32 (lane l: row
//                   l & 31, the elements k = 2 s + (l >> 5) of step s).  The
//                   workgroup stages 64 train rows at a time through LDS;
//                   every wave reads them as the B operand and forms two
//                   32 x 32 tiles of dot products, each accumulator carried
//                   through the dim / 2 steps in order: per element that is
//                   the chain acc = fmaf(q_k, t_k, acc), k ascending from 0.
//                   LDS image: a row holds its even-k elements, then its
//                   odd-k elements, so a lane's operands of four consecutive
//                   steps are one ds_read_b128; rows are dim + 4 floats apart,
//                   which puts the 16 lanes of every ds_read_b128 group on 16
//                   different 16-byte slots of the 256-byte bank row (row
//                   stride = 4 banks mod 64): conflict-free.  The epilogue on
//                   the accumulator registers (lane: one train column, 16
//                   query rows) forms d2 and keeps a top-2 per row and lane;
//                   a lane meets its columns in increasing index, so a strict
//                   comparison keeps the lower index on ties.  At the end the
//                   32 lanes that share a row merge by a min-butterfly on the
//                   keys and one lane writes the chunk's partial list.
//   k_match_merge   one lane per query: the chunks' lists merged by key, the
//                   dense record, the ratio test and the vote for the train
//                   row: a 64-bit atomicMin of (bits(d2) << 32 | query) with
//                   unique, an integer count without.
//   k_match_select  one workgroup per pair: a prefix sum over the train rows
//                   places the matches in (train, query) order; the thread
//                   that writes a record also forms its reference distance.
// The only atomics are integer minima and counts, whose results do not depend
// on the order; every float is formed by one thread in a fixed order.
#include <hip/hip_runtime.h>

#include "ba_kernels.h"
#include "ba_match.h"
#include "../../include/ba_hip.h"

namespace bahip {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kMatchPad = 4;   // floats between LDS rows beyond dim
static_assert(sizeof(MatchKnn) == sizeof(ba_match_neighbors), "dense record");
static_assert(kMatchQTile == 128 && kMatchTTile == 64, "k_match_nn: four waves of 32 queries, two 32-column tiles");

// One wave per 64 rows.  The chain of a row is serial, so a lane owns a row;
// the wave first brings its rows into LDS with coalesced loads (a row stride of
// dim + 1 floats keeps the lanes' walks on different banks).
template <int DIM>
__global__ __launch_bounds__(64) void k_match_norms(MatchArgs A) {
  constexpr int LD = DIM + 1, V = DIM / 4;
  __shared__ float sh[64 * LD];
  const int lane = (int)threadIdx.x, r0 = (int)blockIdx.x * 64, total = A.rows + A.n_ref;
#pragma unroll 8
  for (int e = lane; e < 64 * V; e += 64) {
    const int r = e / V, k = 4 * (e - r * V), row = r0 + r;
    if (row < total) {
      const float* x = row < A.rows ? A.desc + (size_t)row * DIM : A.ref + (size_t)(row - A.rows) * DIM;
      const float4 v = *reinterpret_cast<const float4*>(x + k);
      float* o = sh + r * LD + k;
      o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    }
  }
  __syncthreads();
  if (r0 + lane < total) A.norms[r0 + lane] = match_dot(sh + lane * LD, sh + lane * LD, DIM);
}

// A tile of 64 rows on its way from global memory to the LDS image, in two
// steps so that the loads of the next tile fly while the matrix cores work on
// this one: the thread's DIM / 32 segments of eight floats (rows at or past
// `end` are zeros), then their even-k / odd-k halves into the image.
template <int DIM>
struct MatchStage {
  static constexpr int LD = DIM + kMatchPad, SEG = DIM / 8, N = kMatchTTile * SEG / 256;
  float4 v[N][2];
  __device__ __forceinline__ void load(const float* src, int first, int end) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int s = (int)threadIdx.x + 256 * i, r = s / SEG, g = s - r * SEG;
      v[i][0] = v[i][1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (first + r < end) {
        const float4* p = reinterpret_cast<const float4*>(src + (size_t)(first + r) * DIM + 8 * g);
        v[i][0] = p[0]; v[i][1] = p[1];
      }
    }
  }
  __device__ __forceinline__ void store(float* tile) const {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int s = (int)threadIdx.x + 256 * i, r = s / SEG, g = s - r * SEG;
      float* row = tile + r * LD;
      *reinterpret_cast<float4*>(row + 4 * g) = make_float4(v[i][0].x, v[i][0].z, v[i][1].x, v[i][1].z);             // k = 8 g + 0, 2, 4, 6
      *reinterpret_cast<float4*>(row + DIM / 2 + 4 * g) = make_float4(v[i][0].y, v[i][0].w, v[i][1].y, v[i][1].w);   // k = 8 g + 1, 3, 5, 7
    }
  }
};

// (two workgroups per compute unit at dim 64, so that one wave's epilogue runs
// under another's MFMAs; at dim 128 the query rows alone take 64 registers and
// the kernel keeps one workgroup per unit rather than spill)
template <int DIM>
__global__ __launch_bounds__(256, DIM == 64 ? 2 : 1) void k_match_nn(MatchArgs A) {
  constexpr int LD = DIM + kMatchPad, NF = DIM / 2;
  __shared__ __attribute__((aligned(16))) float tile[kMatchTTile * LD];
  const MatchPair P = A.pair[blockIdx.x];
  const int q0 = (int)blockIdx.y * kMatchQTile;
  if (q0 >= P.nq) return;
  const int chunk = (int)blockIdx.z;
  const int t_begin = chunk * A.chunk_rows, t_end = min(P.nt, t_begin + A.chunk_rows);
  const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31, half = lane >> 5;
  unsigned long long* part = A.part + 2 * ((size_t)P.qoff * A.chunks + chunk);   // row q: part + 2 * chunks * q
  if (t_begin >= t_end) {   // this pair's train set ends before the chunk
    if (tid < kMatchQTile && q0 + tid < P.nq) {
      part[2 * (size_t)A.chunks * (q0 + tid)] = kMatchNone;
      part[2 * (size_t)A.chunks * (q0 + tid) + 1] = kMatchNone;
    }
    return;
  }
  // ---- the wave's 32 queries: lane (col, half) keeps row col's elements k = 2 s + half
  float a[NF];
  MatchStage<DIM> stage;
  for (int round = 0; round < 2; ++round) {
    stage.load(A.desc + (size_t)P.q0 * DIM, q0 + 64 * round, P.nq);
    __syncthreads();
    stage.store(tile);
    __syncthreads();
    if ((wave >> 1) == round) {
      const float* row = tile + (32 * (wave & 1) + col) * LD + half * NF;
#pragma unroll
      for (int m = 0; m < NF / 4; ++m) {
        const float4 v = *reinterpret_cast<const float4*>(row + 4 * m);
        a[4 * m] = v.x; a[4 * m + 1] = v.y; a[4 * m + 2] = v.z; a[4 * m + 3] = v.w;
      }
    }
  }
  // accumulator register r of this lane: query row (r & 3) + 8 (r >> 2) + 4 half of the wave's 32
  const int qw = q0 + 32 * wave;
  float nq[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int q = qw + (r & 3) + 8 * (r >> 2) + 4 * half;
    nq[r] = q < P.nq ? A.norms[P.q0 + q] : 0.0f;
  }
  uint32_t d0[16], i0[16], d1[16], i1[16];   // per row: best and second (bits(d2), train); all ones: none
#pragma unroll
  for (int r = 0; r < 16; ++r) { d0[r] = i0[r] = d1[r] = i1[r] = 0xffffffffu; }

  const float* train = A.desc + (size_t)P.t0 * DIM;
  stage.load(train, t_begin, t_end);
  for (int tt = t_begin; tt < t_end; tt += kMatchTTile) {
    __syncthreads();   // (the reads of the tile before)
    stage.store(tile);
    __syncthreads();
    if (tt + kMatchTTile < t_end) stage.load(train, tt + kMatchTTile, t_end);
    f32x16 acc0 = {0}, acc1 = {0};
    const float* b0 = tile + col * LD + half * NF;
    const float* b1 = b0 + 32 * LD;
#pragma unroll
    for (int m = 0; m < NF / 4; ++m) {
      const float4 u = *reinterpret_cast<const float4*>(b0 + 4 * m);
      const float4 v = *reinterpret_cast<const float4*>(b1 + 4 * m);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * m], u.x, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * m], v.x, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * m + 1], u.y, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * m + 1], v.y, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * m + 2], u.z, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * m + 2], v.z, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * m + 3], u.w, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * m + 3], v.w, acc1, 0, 0, 0);
    }
    // ---- epilogue: this lane's two train columns (the lower index first)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int t = tt + 32 * c + col;
      if (t < t_end) {
        const float nt = A.norms[P.t0 + t];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const uint32_t d = match_bits(match_d2(c ? acc1[r] : acc0[r], nq[r], nt));
          if (d < d0[r]) { d1[r] = d0[r]; i1[r] = i0[r]; d0[r] = d; i0[r] = (uint32_t)t; }
          else if (d < d1[r]) { d1[r] = d; i1[r] = (uint32_t)t; }
        }
      }
    }
  }
  // ---- the 32 lanes of a row: min-butterfly on the keys; lane col == r writes row r
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    MatchTop2 m{((unsigned long long)d0[r] << 32) | i0[r], ((unsigned long long)d1[r] << 32) | i1[r]};
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) {
      const MatchTop2 o{__shfl_xor(m.k0, off, 64), __shfl_xor(m.k1, off, 64)};
      m = match_merge(m, o);
    }
    const int q = qw + (r & 3) + 8 * (r >> 2) + 4 * half;
    if (col == r && q < P.nq) {
      part[2 * (size_t)A.chunks * q] = m.k0;
      part[2 * (size_t)A.chunks * q + 1] = m.k1;
    }
  }
}

__global__ __launch_bounds__(256) void k_match_merge(MatchArgs A) {
  const MatchPair P = A.pair[blockIdx.x];
  const int q = (int)(blockIdx.y * 256 + threadIdx.x);
  if (q >= P.nq) return;
  MatchTop2 m{kMatchNone, kMatchNone};
  if (P.nt > 0) {
    const unsigned long long* part = A.part + 2 * (size_t)A.chunks * ((size_t)P.qoff + q);
    for (int c = 0; c < A.chunks; ++c) m = match_merge(m, MatchTop2{part[2 * c], part[2 * c + 1]});
  }
  const MatchKnn k = match_knn_record(m);
  ba_match_neighbors* o = A.knn + (size_t)P.qoff + q;
  o->idx0 = k.idx0; o->idx1 = k.idx1; o->d2_0 = k.d2_0; o->d2_1 = k.d2_1;
  if (!A.select) return;
  const bool s = match_survives(k, A.ratio, A.max_distance);
  A.surv[(size_t)P.qoff + q] = s ? 1 : 0;
  if (!s) return;
  if (A.unique) atomicMin(A.win + (size_t)P.toff + k.idx0, match_key(k.d2_0, (uint32_t)q));
  else atomicAdd(A.hist + (size_t)P.toff + k.idx0, 1);
}

// exclusive prefix sum of v over the workgroup's 256 threads; total: the sum
__device__ __forceinline__ int match_block_scan(int v, int* sh, int* total) {
  const int lane = (int)threadIdx.x & 63, w = (int)threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(inc, off, 64);
    if (lane >= off) inc += o;
  }
  __syncthreads();
  if (lane == 63) sh[w] = inc;
  __syncthreads();
  int base = 0, sum = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) { base += i < w ? sh[i] : 0; sum += sh[i]; }
  *total = sum;
  return base + inc - v;
}

__device__ __forceinline__ void match_write(const MatchArgs& A, const MatchPair& P, int pos, int q, int t) {
  const ba_match_neighbors k = A.knn[(size_t)P.qoff + q];
  ba_match m;
  m.query = q; m.train = t;
  m.distance = match_sqrt(k.d2_0); m.second_distance = match_sqrt(k.d2_1);
  m.ref_distance = -1.0f;
  const int ref = A.row_ref ? A.row_ref[P.q0 + q] : -1;
  if (ref >= 0) {
    const float dot = match_dot(A.desc + (size_t)(P.t0 + t) * A.dim, A.ref + (size_t)ref * A.dim, A.dim);
    m.ref_distance = match_sqrt(match_d2(dot, A.norms[P.t0 + t], A.norms[A.rows + ref]));
  }
  A.matches[(size_t)P.moff + pos] = m;
}

__global__ __launch_bounds__(256) void k_match_select(MatchArgs A) {
  __shared__ int sh[4];
  __shared__ int st[256];
  const MatchPair P = A.pair[blockIdx.x];
  const int tid = (int)threadIdx.x;
  int carry = 0, total;
  if (A.unique) {
    for (int base = 0; base < P.nt; base += 256) {
      const int t = base + tid;
      const unsigned long long w = t < P.nt ? A.win[(size_t)P.toff + t] : kMatchNone;
      const int pos = carry + match_block_scan(w != kMatchNone ? 1 : 0, sh, &total);
      if (w != kMatchNone) match_write(A, P, pos, (int)(uint32_t)w, t);
      carry += total;
    }
  } else {
    // counts -> first slots
    for (int base = 0; base < P.nt; base += 256) {
      const int t = base + tid;
      const int c = t < P.nt ? A.hist[(size_t)P.toff + t] : 0;
      const int pos = carry + match_block_scan(c, sh, &total);
      if (t < P.nt) A.hist[(size_t)P.toff + t] = pos;
      carry += total;
    }
    // queries in increasing order, 256 at a time: a survivor's slot is its
    // train row's next free one plus the survivors of that row before it in
    // the batch; the last of them moves the row's free slot on
    for (int base = 0; base < P.nq; base += 256) {
      const int q = base + tid;
      const bool s = q < P.nq && A.surv[(size_t)P.qoff + q] != 0;
      const int t = s ? A.knn[(size_t)P.qoff + q].idx0 : -1;
      __syncthreads();
      st[tid] = t;
      __syncthreads();
      int rank = 0;
      bool last = true;
      if (s) {
        for (int j = 0; j < 256; ++j) {
          const bool same = st[j] == t;
          rank += same && j < tid ? 1 : 0;
          last = last && !(same && j > tid);
        }
      }
      const int pos = s ? A.hist[(size_t)P.toff + t] + rank : 0;
      __syncthreads();
      if (s && last) A.hist[(size_t)P.toff + t] = pos + 1;
      if (s) match_write(A, P, pos, q, t);
    }
  }
  if (tid == 0) A.cnt[blockIdx.x] = carry;
}

void launch_match(const MatchArgs& A, hipStream_t s, hipEvent_t* ev) {
  const int nr = A.rows + A.n_ref;
  if (nr > 0) {
    if (A.dim == 64) hipLaunchKernelGGL(k_match_norms<64>, dim3((nr + 63) / 64), dim3(64), 0, s, A);
    else hipLaunchKernelGGL(k_match_norms<128>, dim3((nr + 63) / 64), dim3(64), 0, s, A);
  }
  if (ev) (void)hipEventRecord(ev[0], s);
  if (A.n_pair > 0 && A.max_nq > 0) {
    const dim3 g(A.n_pair, (A.max_nq + kMatchQTile - 1) / kMatchQTile, A.chunks);
    if (A.max_nt > 0) {
      if (A.dim == 64) hipLaunchKernelGGL(k_match_nn<64>, g, dim3(256), 0, s, A);
      else hipLaunchKernelGGL(k_match_nn<128>, g, dim3(256), 0, s, A);
    }
  }
  if (ev) (void)hipEventRecord(ev[1], s);
  if (A.n_pair > 0 && A.max_nq > 0)
    hipLaunchKernelGGL(k_match_merge, dim3(A.n_pair, (A.max_nq + 255) / 256), dim3(256), 0, s, A);
  if (A.n_pair > 0 && A.select) hipLaunchKernelGGL(k_match_select, dim3(A.n_pair), dim3(256), 0, s, A);
  if (ev) (void)hipEventRecord(ev[2], s);
}

}  // namespace bahip
