// two_view_host.cpp — the sampler, the minimal solvers, the essential
// projection and the decompositions of ba_two_view_ransac
// (bundleadjustment_amd/csrc/ba_two_view.h) compiled as a host program, run
// under ASan + UBSan by tests/test_two_view_cpu.py.  Reads cases from the file
// named on the command line and prints the results:
//   sample <seed> <n> <h0> <count>           -> <count> lines of eight indices
//   models <K col-major x9> 8 x (u1 v1 u2 v2) -> "<valid E> <valid H>", E, H (row-major)
//   pose <model 1|2> <K x9> <M row-major x9> <thr2> <n> n x (u1 v1 u2 v2)
//        the per-pair stage for one model matrix, serially: the projection
//        (model 1), the final mask, the candidates and the depth vote
//        -> "<n_cand> <best> <n_good> <n_second>", R t n of the winner (15
//        values), the matrix the mask was taken at, the mask as 0/1 digits
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../bundleadjustment_amd/csrc/ba_two_view.h"

using namespace bahip;

static void print9(const double* M) {
  for (int e = 0; e < 9; ++e) std::printf("%.17g%c", M[e], e == 8 ? '\n' : ' ');
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: two_view_host <cases>\n"); return 2; }
  std::FILE* in = std::fopen(argv[1], "r");
  if (!in) { std::perror(argv[1]); return 2; }
  char word[16];
  int rc = 0;
  while (std::fscanf(in, "%15s", word) == 1) {
    if (!std::strcmp(word, "sample")) {
      uint64_t seed;
      int n, h0, count;
      if (std::fscanf(in, "%" SCNu64 " %d %d %d", &seed, &n, &h0, &count) != 4 || n < 8) { rc = 3; break; }
      for (int h = h0; h < h0 + count; ++h) {
        int s[8];
        tv_sample(seed, (uint32_t)h, n, s);
        for (int j = 0; j < 8; ++j) std::printf("%d%c", s[j], j == 7 ? '\n' : ' ');
      }
    } else if (!std::strcmp(word, "models")) {
      double K[9], Ki[9], b1[8][2], b2[8][2], p1[4][2], p2[4][2];
      bool ok = true;
      for (double& k : K) ok = ok && std::fscanf(in, "%lf", &k) == 1;
      if (ok) p3p_inv3(K, Ki);
      for (int i = 0; i < 8 && ok; ++i) {
        float m[4];   // pixels are float values, promoted
        ok = std::fscanf(in, "%f %f %f %f", &m[0], &m[1], &m[2], &m[3]) == 4;
        tv_bearing(Ki, (double)m[0], (double)m[1], b1[i]);
        tv_bearing(Ki, (double)m[2], (double)m[3], b2[i]);
        if (i < 4) { p1[i][0] = m[0]; p1[i][1] = m[1]; p2[i][0] = m[2]; p2[i][1] = m[3]; }
      }
      if (!ok) { rc = 3; break; }
      double E[9], H[9];
      const bool ve = tv_solve_e(b1, b2, E), vh = tv_solve_h(p1, p2, H);
      std::printf("%d %d\n", ve ? 1 : 0, vh ? 1 : 0);
      print9(E);
      print9(H);
    } else if (!std::strcmp(word, "pose")) {
      int model, n;
      double K[9], Ki[9], M[9], thr2;
      bool ok = std::fscanf(in, "%d", &model) == 1 && (model == 1 || model == 2);
      for (double& k : K) ok = ok && std::fscanf(in, "%lf", &k) == 1;
      for (double& m : M) ok = ok && std::fscanf(in, "%lf", &m) == 1;
      ok = ok && std::fscanf(in, "%lf %d", &thr2, &n) == 2 && n >= 0;
      if (!ok) { rc = 3; break; }
      std::vector<float> m(4 * (size_t)n);
      for (float& v : m) ok = ok && std::fscanf(in, "%f", &v) == 1;
      if (!ok) { rc = 3; break; }
      p3p_inv3(K, Ki);
      double U[3][3] = {}, V[3][3] = {}, At[9], F[9] = {}, Hi[9] = {};
      TvHDecomp HD{};
      int ncand;
      if (model == 1) {
        ncand = tv_project_e(M, At, U, V) ? 4 : 0;
        tv_fundamental(At, Ki, Ki, F);
      } else {
        std::memcpy(At, M, sizeof At);
        tv_inv3(M, Hi);
        double T[9], Am[9];
        for (int k = 0; k < 3; ++k)
          for (int j = 0; j < 3; ++j) T[3 * k + j] = M[3 * k] * K[3 * j] + M[3 * k + 1] * K[3 * j + 1] + M[3 * k + 2] * K[3 * j + 2];
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) Am[3 * i + j] = Ki[i] * T[j] + Ki[3 + i] * T[3 + j] + Ki[6 + i] * T[6 + j];
        ncand = tv_h_decompose(Am, &HD) ? 8 : 0;
      }
      std::vector<char> mask((size_t)n, 0);
      for (int k = 0; k < n; ++k) {
        const double u1 = m[4 * (size_t)k], v1 = m[4 * (size_t)k + 1], u2 = m[4 * (size_t)k + 2], v2 = m[4 * (size_t)k + 3];
        if (model == 1) {
          double d1, d2;
          tv_e_dist2(F, u1, v1, u2, v2, &d1, &d2);
          mask[k] = d1 <= thr2 && d2 <= thr2 && d1 <= kTvChi1 && d2 <= kTvChi1;
        } else {
          const double e2 = tv_h_err2(M, u1, v1, u2, v2), e1 = tv_h_err2(Hi, u2, v2, u1, v1);
          mask[k] = e1 <= thr2 && e2 <= thr2 && e1 <= kTvChi2 && e2 <= kTvChi2;
        }
      }
      int best = -1, n_good = 0, n_second = 0;
      double best_nz = 0.0, R[9] = {0}, t[3] = {0}, nrm[3] = {0};
      for (int c = 0; c < ncand; ++c) {
        if (model == 2) tv_h_candidate(&HD, c, R, t, nrm); else tv_e_candidate(U, V, c, R, t);
        int cnt = 0;
        for (int k = 0; k < n; ++k) {
          if (!mask[k]) continue;
          double b1[2], b2[2];
          tv_bearing(Ki, m[4 * (size_t)k], m[4 * (size_t)k + 1], b1);
          tv_bearing(Ki, m[4 * (size_t)k + 2], m[4 * (size_t)k + 3], b2);
          cnt += tv_depth_good(R, t, b1, b2) ? 1 : 0;
        }
        const double nz = nrm[2] < 0.0 ? -nrm[2] : nrm[2];
        if (best < 0 || cnt > n_good || (cnt == n_good && nz > best_nz)) {
          if (best >= 0) n_second = n_good;
          best = c; n_good = cnt; best_nz = nz;
        } else if (cnt > n_second) {
          n_second = cnt;
        }
      }
      if (best >= 0) { if (model == 2) tv_h_candidate(&HD, best, R, t, nrm); else tv_e_candidate(U, V, best, R, t); }
      std::printf("%d %d %d %d\n", ncand, best, n_good, n_second);
      for (int e = 0; e < 9; ++e) std::printf("%.17g ", R[e]);
      std::printf("%.17g %.17g %.17g %.17g %.17g %.17g\n", t[0], t[1], t[2], nrm[0], nrm[1], nrm[2]);
      print9(At);
      for (int k = 0; k < n; ++k) std::putchar(mask[k] ? '1' : '0');
      std::putchar('\n');
    } else {
      rc = 3;
      break;
    }
  }
  std::fclose(in);
  if (rc) std::fprintf(stderr, "bad case file\n");
  return rc;
}
