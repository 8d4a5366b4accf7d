// two_view_e5_host.cpp — the five-point essential solver of ba_two_view_ransac
// (tv_solve_e5, bundleadjustment_amd/csrc/ba_two_view.h) compiled as a host
// program, run under ASan + UBSan by tests/test_two_view_e5_cpu.py.  Reads
// cases from the file named on the command line and prints the results:
//   solve5 <K col-major x9> 5 x (u1 v1 u2 v2)
//       -> "<n_sol>", then ten lines of E (row-major; zeros past n_sol)
// The strided store is a local array with stride 1, guarded on both sides.
#include <cstdio>
#include <cstring>

#include "../../bundleadjustment_amd/csrc/ba_two_view.h"

using namespace bahip;

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: two_view_e5_host <cases>\n"); return 2; }
  std::FILE* in = std::fopen(argv[1], "r");
  if (!in) { std::perror(argv[1]); return 2; }
  char word[16];
  int rc = 0;
  while (std::fscanf(in, "%15s", word) == 1) {
    if (std::strcmp(word, "solve5")) { rc = 3; break; }
    double K[9], Ki[9], b1[5][2], b2[5][2];
    bool ok = true;
    for (double& k : K) ok = ok && std::fscanf(in, "%lf", &k) == 1;
    if (ok) p3p_inv3(K, Ki);
    for (int i = 0; i < 5 && ok; ++i) {
      float m[4];   // pixels are float values, promoted
      ok = std::fscanf(in, "%f %f %f %f", &m[0], &m[1], &m[2], &m[3]) == 4;
      tv_bearing(Ki, (double)m[0], (double)m[1], b1[i]);
      tv_bearing(Ki, (double)m[2], (double)m[3], b2[i]);
    }
    if (!ok) { rc = 3; break; }
    double* S = new double[kTv5Store];   // on the heap: ASan sees an index one past either end
    double* E = new double[90];
    const int n_sol = tv_solve_e5(b1, b2, S, 1, E, 9);
    std::printf("%d\n", n_sol);
    for (int s = 0; s < 10; ++s)
      for (int e = 0; e < 9; ++e) std::printf("%.17g%c", E[9 * s + e], e == 8 ? '\n' : ' ');
    delete[] S;
    delete[] E;
  }
  std::fclose(in);
  if (rc) std::fprintf(stderr, "bad case file\n");
  return rc;
}
