// pnp_host.cpp — the sampler and the P3P solver of ba_pnp_ransac
// (bundleadjustment_amd/csrc/ba_p3p.h) compiled as a host program, run under
// ASan + UBSan by tests/test_pnp_cpu.py.  Reads cases from the file named on
// the command line and prints the results:
//   sample <seed> <n> <h0> <count>        -> <count> lines "a b c"
//   p3p <K col-major x9> 3 x (X Y Z u v)  -> "<n_sol>", then per solution one
//                                            line of R (row-major) and t
//   aa <R row-major x9>                   -> the angle-axis "w0 w1 w2"
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../bundleadjustment_amd/csrc/ba_p3p.h"

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: pnp_host <cases>\n"); return 2; }
  std::FILE* in = std::fopen(argv[1], "r");
  if (!in) { std::perror(argv[1]); return 2; }
  char word[16];
  int rc = 0;
  while (std::fscanf(in, "%15s", word) == 1) {
    if (!std::strcmp(word, "sample")) {
      uint64_t seed;
      int n, h0, count;
      if (std::fscanf(in, "%" SCNu64 " %d %d %d", &seed, &n, &h0, &count) != 4 || n < 3) { rc = 3; break; }
      for (int h = h0; h < h0 + count; ++h) {
        int s[3];
        bahip::pnp_sample(seed, (uint32_t)h, n, s);
        std::printf("%d %d %d\n", s[0], s[1], s[2]);
      }
    } else if (!std::strcmp(word, "p3p")) {
      double K[9], Ki[9], X[3][3], f[3][3];
      bool ok = true;
      for (double& k : K) ok = ok && std::fscanf(in, "%lf", &k) == 1;
      for (int i = 0; i < 3 && ok; ++i) {
        float u, v;   // pixels are float values, promoted
        ok = std::fscanf(in, "%lf %lf %lf %f %f", &X[i][0], &X[i][1], &X[i][2], &u, &v) == 5;
        if (i == 0) bahip::p3p_inv3(K, Ki);
        bahip::p3p_bearing(Ki, (double)u, (double)v, f[i]);
      }
      if (!ok) { rc = 3; break; }
      double R[4][9], t[4][3];
      const int mask = bahip::p3p_solve(X, f, R, t);
      int ns = 0;
      for (int k = 0; k < 4; ++k) ns += (mask >> k) & 1;
      std::printf("%d\n", ns);
      for (int k = 0; k < 4; ++k) {
        if (!((mask >> k) & 1)) continue;
        for (int e = 0; e < 9; ++e) std::printf("%.17g ", R[k][e]);
        std::printf("%.17g %.17g %.17g\n", t[k][0], t[k][1], t[k][2]);
      }
    } else if (!std::strcmp(word, "aa")) {
      double R[9], w[3];
      bool ok = true;
      for (double& r : R) ok = ok && std::fscanf(in, "%lf", &r) == 1;
      if (!ok) { rc = 3; break; }
      bahip::p3p_rotation_to_angle_axis(R, w);
      std::printf("%.17g %.17g %.17g\n", w[0], w[1], w[2]);
    } else {
      rc = 3;
      break;
    }
  }
  std::fclose(in);
  if (rc) std::fprintf(stderr, "bad case file\n");
  return rc;
}
