// The GNC-TLS statement of csrc/gnc.h on the host: what pgo_gnc_weight_eval runs and k_gnc_update evaluates, compiled by g++
// with AddressSanitizer + UndefinedBehaviorSanitizer.
//     gnc_main IN OUT
// IN:  "n", then n lines "cbar mu s" (17 digits; inf and nan spelled out).
// OUT: n lines "w mu0" (17 digits): gnc_tls_weight(cbar^2, mu, s) and gnc_mu0(cbar^2, s).
// Built and run by tests/test_gnc_native.py.
#include <cstdio>
#include <vector>

#include "gnc.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "r");
  if (!in) return 1;
  long n;
  if (fscanf(in, "%ld", &n) != 1 || n < 0) return 1;
  std::vector<double> v((size_t)3 * n);
  for (long i = 0; i < n; ++i)
    if (fscanf(in, "%lf %lf %lf", &v[3 * i], &v[3 * i + 1], &v[3 * i + 2]) != 3) return 1;
  fclose(in);
  FILE* out = fopen(argv[2], "w");
  if (!out) return 1;
  for (long i = 0; i < n; ++i) {
    const double c2 = v[3 * i] * v[3 * i];
    fprintf(out, "%.17g %.17g\n", pgo::gnc_tls_weight(c2, v[3 * i + 1], v[3 * i + 2]), pgo::gnc_mu0(c2, v[3 * i + 2]));
  }
  if (fclose(out) != 0) return 1;
  printf("gnc ok: %ld weights\n", n);
  return 0;
}
