// icp_host.cpp — the host side of ba_icp (check_icp, icp_plan, icp_layout:
// host/ba_batch_pack.hpp) and the grid search of the kernels
// (bundleadjustment_amd/csrc/ba_icp.h) compiled as a host program, run under
// ASan + UBSan by tests/test_icp_cpu.py.  Per pair it walks the grid for every
// source point the way k_icp_nn_grid does (a point whose walk passes the ring
// limit is swept over the whole target, as k_icp_nn_brute does), and runs one
// step of the loop on the result (icp_step).  Floats travel as the hexadecimal
// bit patterns of their float32 values.
//
// Input (the file named on the command line):
//   n_sets n_pairs n_points have_guess max_ring
//   max_iterations route min_correspondences with_scale reserved max_corr_dist cell
//   set_offset[n_sets + 1]
//   n_pairs x (source set, target set)
//   xyz[3 * n_points]
//   have_guess: guess[16 * n_pairs]
// Output: per grid "grid <n0> <n1> <n2> <h> <cells> <most points in a cell>",
//   then per pair "pair <i> <ns> <nt> <route> <swept>", a line of ns indices, a
//   line of ns d2, "perm" and the ns entries, and "step <state> <iterations>
//   <n_corr> <M, t as 12 floats>".
// A batch the checker refuses prints "invalid <message>" and exits 0.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../bundleadjustment_amd/csrc/ba_icp.h"
#include "../../bundleadjustment_amd/host/ba_batch_pack.hpp"

using namespace bahip;

static bool read_f32(std::FILE* in, float* v) {
  uint32_t u;
  if (std::fscanf(in, "%" SCNx32, &u) != 1) return false;
  *v = match_float(u);
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: icp_host <case>\n"); return 2; }
  std::FILE* in = std::fopen(argv[1], "r");
  if (!in) { std::perror(argv[1]); return 2; }
  ba_icp_batch b{};
  ba_icp_options opt;
  icp_defaults(opt);
  int n_points = 0, have_guess = 0, max_ring = 0;
  bool ok = std::fscanf(in, "%d %d %d %d %d", &b.n_sets, &b.n_pairs, &n_points, &have_guess, &max_ring) == 5 &&
            std::fscanf(in, "%d %d %d %d %d", &opt.max_iterations, &opt.route, &opt.min_correspondences, &opt.with_scale,
                        &opt.reserved) == 5 &&
            read_f32(in, &opt.max_corr_dist) && read_f32(in, &opt.cell);
  ok = ok && b.n_sets >= 0 && b.n_pairs >= 0 && n_points >= 0;
  if (!ok) { std::fprintf(stderr, "bad case file\n"); return 3; }
  std::vector<int32_t> off((size_t)b.n_sets + 1), ps((size_t)b.n_pairs), pt((size_t)b.n_pairs);
  for (int32_t& v : off) ok = ok && std::fscanf(in, "%" SCNd32, &v) == 1;
  for (int i = 0; i < b.n_pairs && ok; ++i) ok = std::fscanf(in, "%" SCNd32 " %" SCNd32, &ps[(size_t)i], &pt[(size_t)i]) == 2;
  // (the arrays are sized by the declared point count: it covers the offsets of every case, refused ones included)
  ok = ok && off.back() <= n_points;
  std::vector<float> xyz(3 * (size_t)n_points), guess(have_guess ? 16 * (size_t)b.n_pairs : 0);
  for (float& v : xyz) ok = ok && read_f32(in, &v);
  for (float& v : guess) ok = ok && read_f32(in, &v);
  std::fclose(in);
  if (!ok) { std::fprintf(stderr, "bad case file\n"); return 3; }
  b.set_offset = off.data(); b.xyz = xyz.data(); b.pair_src = ps.data(); b.pair_tgt = pt.data();
  b.guess = have_guess ? guess.data() : nullptr;

  try {
    const ba_icp_options p = check_icp("icp_host: ", &b, &opt);
    const IcpPlan M = icp_plan("icp_host: ", &b, p, 0, b.n_pairs);
    const IcpLayout L = icp_layout(M, (size_t)off.back(), p.max_iterations, false);
    if (L.L.total < L.L.io_b || L.L.io_b < L.L.in_b) { std::fprintf(stderr, "layout\n"); return 4; }
    for (const IcpGrid& G : M.grid) {
      const size_t nc = (size_t)G.n[0] * G.n[1] * G.n[2];
      int most = 0;
      for (size_t c = 0; c < nc; ++c) {
        const int k = M.cell_start[G.cell0 + c + 1] - M.cell_start[G.cell0 + c];
        if (k < 0) { std::fprintf(stderr, "cell_start decreases\n"); return 4; }
        most = k > most ? k : most;
      }
      std::printf("grid %d %d %d %08" PRIx32 " %zu %d\n", G.n[0], G.n[1], G.n[2], match_bits(G.h), nc, most);
    }
    const float gate = icp_gate(p.max_corr_dist);
    for (int i = 0; i < b.n_pairs; ++i) {
      const IcpPair& P = M.pair[(size_t)i];
      const IcpGrid& G = M.grid[(size_t)P.grid];
      const IcpPt* sorted = M.sorted.data() + P.t0;
      if (M.cell_start[G.cell0 + (size_t)G.n[0] * G.n[1] * G.n[2]] != P.nt) { std::fprintf(stderr, "cell_start total\n"); return 4; }
      std::vector<char> seen((size_t)P.nt, 0);
      for (int q = 0; q < P.nt; ++q) {
        const IcpPt& s = sorted[q];
        const float* o = xyz.data() + 3 * ((size_t)P.t0 + (size_t)s.j);
        if (s.j < 0 || s.j >= P.nt || seen[(size_t)s.j] || s.x != o[0] || s.y != o[1] || s.z != o[2]) {
          std::fprintf(stderr, "sorted is not a permutation of the target\n");
          return 4;
        }
        seen[(size_t)s.j] = 1;
      }
      IcpState S{};
      const float* g = have_guess ? guess.data() + 16 * (size_t)i : nullptr;
      for (int e = 0; e < 16; ++e) S.fin[e] = g && e < 12 ? g[e] : (e % 5 == 0 ? 1.0f : 0.0f);
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) S.M[3 * r + c] = S.fin[4 * r + c];
        S.t[r] = S.fin[4 * r + 3];
      }
      S.prev = DBL_MAX; S.fitness = DBL_MAX;
      std::vector<float> cur(3 * (size_t)P.ns), d2((size_t)P.ns);
      std::vector<int32_t> idx((size_t)P.ns);
      std::vector<char> done((size_t)P.ns, 0);
      int swept = 0;
      for (int t = 0; t < P.ns; ++t) {
        const int q = M.perm[(size_t)P.soff + (size_t)t];
        if (q < 0 || q >= P.ns || done[(size_t)q]) { std::fprintf(stderr, "perm is not a permutation\n"); return 4; }
        done[(size_t)q] = 1;
        const float* s = xyz.data() + 3 * ((size_t)P.s0 + (size_t)q);
        float x = s[0], y = s[1], z = s[2];
        icp_apply(S.M, S.t, x, y, z);
        cur[3 * (size_t)q] = x; cur[3 * (size_t)q + 1] = y; cur[3 * (size_t)q + 2] = z;
        uint64_t best = kMatchNone;
        const bool grid = P.route == BA_ICP_ROUTE_GRID &&
                          icp_grid_nn(G, M.cell_start.data() + G.cell0, sorted, x, y, z, gate, max_ring, best);
        if (!grid) {
          best = kMatchNone;
          icp_scan(sorted, 0, P.nt, x, y, z, best);
          swept += P.route == BA_ICP_ROUTE_GRID;
        }
        icp_record(best, gate, idx[(size_t)q], d2[(size_t)q]);
      }
      std::printf("pair %d %d %d %d %d\n", i, P.ns, P.nt, P.route, swept);
      for (int q = 0; q < P.ns; ++q) std::printf("%d%c", idx[(size_t)q], q + 1 < P.ns ? ' ' : '\n');
      for (int q = 0; q < P.ns; ++q) std::printf("%08" PRIx32 "%c", match_bits(d2[(size_t)q]), q + 1 < P.ns ? ' ' : '\n');
      std::printf("perm");
      for (int q = 0; q < P.ns; ++q) std::printf(" %d", M.perm[(size_t)P.soff + (size_t)q]);
      std::printf("\n");
      // one step on these correspondences, the sums in index order
      double s[kIcpSums] = {0.0};
      for (int q = 0; q < P.ns; ++q) {
        if (idx[(size_t)q] < 0) continue;
        const float* tq = xyz.data() + 3 * ((size_t)P.t0 + (size_t)idx[(size_t)q]);
        double a[3], c[3];
        for (int r = 0; r < 3; ++r) { a[r] = (double)cur[3 * (size_t)q + r] - (double)G.c0[r]; c[r] = (double)tq[r] - (double)G.c0[r]; }
        for (int r = 0; r < 3; ++r) {
          s[r] += a[r]; s[3 + r] += c[r];
          for (int cc = 0; cc < 3; ++cc) s[6 + 3 * r + cc] += c[r] * a[cc];
        }
        s[15] += a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
        s[16] += (double)d2[(size_t)q];
        s[17] += 1.0;
      }
      const IcpRules rules{p.max_iterations, p.min_correspondences, p.with_scale, p.mse_abs_eps, p.mse_rel_eps, p.transformation_eps};
      icp_step(S, s, G.c0, rules, 0);
      std::printf("step %d %d %d", S.state, S.iterations, S.n_corr);
      for (int e = 0; e < 9; ++e) std::printf(" %08" PRIx32, match_bits(S.M[e]));
      for (int e = 0; e < 3; ++e) std::printf(" %08" PRIx32, match_bits(S.t[e]));
      std::printf("\n");
    }
  } catch (const BaError& e) {
    std::printf("invalid %s\n", e.msg.c_str());
  }
  return 0;
}
