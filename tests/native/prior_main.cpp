// The pose prior of csrc/prior.h on the host: what pgo_prior_eval runs, k_prior_eval evaluates and pgo_set_priors checks,
// compiled by g++ with AddressSanitizer + UndefinedBehaviorSanitizer.
//     prior_main IN OUT
// IN:  "n", then n lines "x y t zx zy zt I11 I12 I13 I22 I23 I33 loss_type loss_a" (17 digits).
// OUT: n lines "class d0 d1 d2 chi2 rho rho' rho''" (17 digits): class = prior_info_class of the information (-2 not finite,
//      -1 indefinite, 0 positive semi-definite, 1 positive definite); the other values are 0 where class < 0.
// Built and run by tests/test_prior_native.py.
#include <cstdio>

#include "prior.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "r");
  if (!in) return 1;
  FILE* out = fopen(argv[2], "w");
  if (!out) return 1;
  long n;
  if (fscanf(in, "%ld", &n) != 1 || n < 0) return 1;
  for (long i = 0; i < n; ++i) {
    double p[3], z[3], w[6], a;
    int type;
    if (fscanf(in, "%lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %lf %d %lf", &p[0], &p[1], &p[2], &z[0], &z[1], &z[2], &w[0], &w[1], &w[2],
               &w[3], &w[4], &w[5], &type, &a) != 14)
      return 1;
    const int cls = (int)pgo::prior_info_class(w);
    double d[3] = {0, 0, 0}, q[3], chi2 = 0.0, rho[3] = {0, 0, 0};
    if (cls >= 0)
      pgo::prior_eval(pgo::make_loss_class(type, a), p[0], p[1], p[2], z[0], z[1], z[2], w[0], w[1], w[2], w[3], w[4], w[5], d[0], d[1], d[2],
                      q[0], q[1], q[2], chi2, rho);
    fprintf(out, "%d %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", cls, d[0], d[1], d[2], chi2, rho[0], rho[1], rho[2]);
  }
  fclose(in);
  if (fclose(out) != 0) return 1;
  printf("prior ok: %ld cases\n", n);
  return 0;
}
