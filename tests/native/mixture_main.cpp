// The max-mixture statement of csrc/mixture.h on the host: what pgo_mixture_eval / pgo_mixture_plan run and k_mix_select
// evaluates, compiled by g++ with AddressSanitizer + UndefinedBehaviorSanitizer.
//     mixture_main IN OUT
// IN:  "n", then n cases: a line "K loss_type loss_a" and K lines "pi w s" (17 digits; inf and nan spelled out).
// OUT: n lines "chosen q_best margin c_0 .. c_{K-1}" (17 digits): the pick over q_k = mix_q(loss, w_k, mix_const(pi_k, w_k), s_k)
//      taken in index order, and the constants.
// Built and run by tests/test_mixture_native.py.
#include <cstdio>
#include <vector>

#include "mixture.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "r");
  if (!in) return 1;
  FILE* out = fopen(argv[2], "w");
  if (!out) return 1;
  long n;
  if (fscanf(in, "%ld", &n) != 1 || n < 0) return 1;
  for (long i = 0; i < n; ++i) {
    int K, type;
    double a;
    if (fscanf(in, "%d %d %lf", &K, &type, &a) != 3 || K < 1 || K > pgo::MIX_MAX_COMPONENTS) return 1;
    const pgo::LossClass L = pgo::make_loss_class(type, a);
    std::vector<double> c((size_t)K);
    pgo::MixPick P = pgo::mix_pick_begin();
    for (int k = 0; k < K; ++k) {
      double pi, w, s;
      if (fscanf(in, "%lf %lf %lf", &pi, &w, &s) != 3) return 1;
      c[(size_t)k] = pgo::mix_const(pi, w);
      pgo::mix_pick_take(P, k, pgo::mix_q(L, w, c[(size_t)k], s));
    }
    fprintf(out, "%d %.17g %.17g", P.k, pgo::mix_pick_best(P), pgo::mix_pick_margin(P));
    for (int k = 0; k < K; ++k) fprintf(out, " %.17g", c[(size_t)k]);
    fprintf(out, "\n");
  }
  fclose(in);
  if (fclose(out) != 0) return 1;
  printf("mixture ok: %ld cases\n", n);
  return 0;
}
