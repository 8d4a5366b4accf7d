// match_host.cpp — the pinned arithmetic of ba_match_descriptors
// (bundleadjustment_amd/csrc/ba_match.h) and its host-side packing
// (check_match, match_plan, match_layout: host/ba_batch_pack.hpp) compiled as
// a host program, run under ASan + UBSan by tests/test_match_cpu.py.  It
// matches a batch serially the way the kernels do (norms first, partial top-2
// lists per train chunk of the plan merged by key, ratio test, the winner per
// train row by the smallest key, (train, query) order).  Floats travel as the
// hexadecimal bit patterns of their float32 values.
//
// Input (the file named on the command line):
//   dim n_sets n_pairs n_ref have_ref rows ratio unique max_distance
//   set_offset[n_sets + 1]
//   n_pairs x (query set, train set)
//   desc[rows * dim]
//   have_ref: row_ref[rows], ref_desc[n_ref * dim]
// Output: "plan <chunks> <chunk_rows> <NQ> <NT> <NM> <layout bytes>", then per pair
//   "pair <i> <n_q> <n_t> <n_matches>", n_q lines of d2 (n_t values), n_q lines
//   "idx0 idx1 d2_0 d2_1", n_matches lines "query train distance second ref".
// A batch the checker refuses prints "invalid <message>" and exits 0.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../bundleadjustment_amd/csrc/ba_match.h"
#include "../../bundleadjustment_amd/host/ba_batch_pack.hpp"

using namespace bahip;

static bool read_f32(std::FILE* in, float* v) {
  uint32_t u;
  if (std::fscanf(in, "%" SCNx32, &u) != 1) return false;
  *v = match_float(u);
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: match_host <case>\n"); return 2; }
  std::FILE* in = std::fopen(argv[1], "r");
  if (!in) { std::perror(argv[1]); return 2; }
  ba_match_batch b{};
  ba_match_options opt{};
  int have_ref = 0, n_rows = 0;
  bool ok = std::fscanf(in, "%d %d %d %d %d %d", &b.dim, &b.n_sets, &b.n_pairs, &b.n_ref, &have_ref, &n_rows) == 6 &&
            read_f32(in, &opt.ratio) && std::fscanf(in, "%d", &opt.unique) == 1 && read_f32(in, &opt.max_distance);
  ok = ok && b.n_sets >= 0 && b.n_pairs >= 0 && b.n_ref >= 0 && b.dim > 0 && n_rows >= 0;
  if (!ok) { std::fprintf(stderr, "bad case file\n"); return 3; }
  std::vector<int32_t> off((size_t)b.n_sets + 1), pq((size_t)b.n_pairs), pt((size_t)b.n_pairs);
  for (int32_t& v : off) ok = ok && std::fscanf(in, "%" SCNd32, &v) == 1;
  for (int i = 0; i < b.n_pairs && ok; ++i) ok = std::fscanf(in, "%" SCNd32 " %" SCNd32, &pq[(size_t)i], &pt[(size_t)i]) == 2;
  // (the arrays are sized by the declared row count: it covers the offsets of every case, refused ones included)
  const size_t rows = (size_t)n_rows;
  ok = ok && off.back() <= n_rows;
  std::vector<float> desc(rows * (size_t)b.dim), ref(have_ref ? (size_t)b.n_ref * (size_t)b.dim : 0);
  std::vector<int32_t> row_ref(have_ref ? rows : 0);
  for (float& v : desc) ok = ok && read_f32(in, &v);
  for (int32_t& v : row_ref) ok = ok && std::fscanf(in, "%" SCNd32, &v) == 1;
  for (float& v : ref) ok = ok && read_f32(in, &v);
  std::fclose(in);
  if (!ok) { std::fprintf(stderr, "bad case file\n"); return 3; }
  b.set_offset = off.data(); b.desc = desc.data(); b.pair_query = pq.data(); b.pair_train = pt.data();
  b.row_ref = have_ref ? row_ref.data() : nullptr; b.ref_desc = have_ref ? ref.data() : nullptr;

  ba_match_options p;
  MatchPlan M;
  try {
    p = check_match("match_host: ", &b, &opt);
    M = match_plan("match_host: ", &b, p.unique, 0, b.n_pairs);
  } catch (const BaError& e) {
    std::printf("invalid %s\n", e.msg.c_str());
    return 0;
  }
  const MatchLayout L = match_layout(M, rows, (size_t)b.n_ref, b.dim, have_ref != 0, false);
  std::printf("plan %d %d %zu %zu %zu %zu\n", M.chunks, M.chunk_rows, M.NQ, M.NT, M.NM, L.L.total);

  const int dim = b.dim;
  std::vector<float> norms(rows + ref.size() / (size_t)dim);
  for (size_t r = 0; r < rows; ++r) norms[r] = match_dot(&desc[r * dim], &desc[r * dim], dim);
  for (size_t r = 0; r < ref.size() / (size_t)dim; ++r) norms[rows + r] = match_dot(&ref[r * dim], &ref[r * dim], dim);

  for (int i = 0; i < b.n_pairs; ++i) {
    const MatchPair& P = M.pair[(size_t)i];
    std::vector<float> d2((size_t)P.nq * (size_t)P.nt);
    std::vector<MatchKnn> knn((size_t)P.nq);
    std::vector<uint64_t> win((size_t)P.nt, kMatchNone);
    std::vector<char> surv((size_t)P.nq, 0);
    for (int q = 0; q < P.nq; ++q) {
      const float* x = &desc[(size_t)(P.q0 + q) * dim];
      MatchTop2 best{kMatchNone, kMatchNone};
      for (int c = 0; c < M.chunks; ++c) {   // the kernels' split: partial lists per chunk, merged by key
        MatchTop2 part{kMatchNone, kMatchNone};
        for (int t = c * M.chunk_rows; t < std::min(P.nt, (c + 1) * M.chunk_rows); ++t) {
          const float v = match_d2(match_dot(x, &desc[(size_t)(P.t0 + t) * dim], dim), norms[(size_t)(P.q0 + q)],
                                   norms[(size_t)(P.t0 + t)]);
          d2[(size_t)q * P.nt + t] = v;
          match_push(part, match_key(v, (uint32_t)t));
        }
        best = match_merge(best, part);
      }
      knn[(size_t)q] = match_knn_record(best);
      surv[(size_t)q] = match_survives(knn[(size_t)q], p.ratio, p.max_distance) ? 1 : 0;
      if (surv[(size_t)q]) {
        uint64_t& w = win[(size_t)knn[(size_t)q].idx0];
        w = std::min(w, match_key(knn[(size_t)q].d2_0, (uint32_t)q));
      }
    }
    std::vector<ba_match> out;
    for (int t = 0; t < P.nt; ++t)
      for (int q = 0; q < P.nq; ++q) {
        const MatchKnn& k = knn[(size_t)q];
        if (!surv[(size_t)q] || k.idx0 != t) continue;
        if (p.unique && (uint32_t)win[(size_t)t] != (uint32_t)q) continue;
        ba_match m{q, t, match_sqrt(k.d2_0), match_sqrt(k.d2_1), -1.0f};
        const int r = have_ref ? row_ref[(size_t)(P.q0 + q)] : -1;
        if (r >= 0)
          m.ref_distance = match_sqrt(match_d2(match_dot(&desc[(size_t)(P.t0 + t) * dim], &ref[(size_t)r * dim], dim),
                                               norms[(size_t)(P.t0 + t)], norms[rows + (size_t)r]));
        out.push_back(m);
      }
    if (out.size() > (size_t)P.cap) { std::fprintf(stderr, "capacity exceeded\n"); return 4; }
    std::printf("pair %d %d %d %zu\n", i, P.nq, P.nt, out.size());
    for (int q = 0; q < P.nq; ++q) {
      for (int t = 0; t < P.nt; ++t) std::printf("%08" PRIx32 " ", match_bits(d2[(size_t)q * P.nt + t]));
      std::printf("\n");
    }
    for (const MatchKnn& k : knn)
      std::printf("%d %d %08" PRIx32 " %08" PRIx32 "\n", k.idx0, k.idx1, match_bits(k.d2_0), match_bits(k.d2_1));
    for (const ba_match& m : out)
      std::printf("%d %d %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", m.query, m.train, match_bits(m.distance),
                  match_bits(m.second_distance), match_bits(m.ref_distance));
  }
  return 0;
}
