// The coarsening operators of csrc/coarsen.h on the host: the statement pgo_coarsen_plan / pgo_prolong_eval run and the kernels
// of coarsen.hip.h evaluate, compiled by g++ with AddressSanitizer + UndefinedBehaviorSanitizer.
//     coarsen_main IN OUT
// IN:  "n stride m", then n - 1 lines "reversed mx my mt" (the chain edge of the pair (i, i + 1), stored as (i + 1, i) when
//      reversed), then m lines "a b mx my mt" (other edges), then K = ceil(n / stride) lines "x y theta" (coarse poses).
// OUT: n lines C, K - 1 lines Cend, m lines C_a o m o C_b^-1, n lines of the prolongation (17 digits).
// Built and run by tests/test_coarsen_native.py.
#include <cstdio>
#include <vector>

#include "coarsen.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "r");
  if (!in) return 1;
  long n, S, m;
  if (fscanf(in, "%ld %ld %ld", &n, &S, &m) != 3 || S < 2 || n <= S || m < 0) return 1;
  const long K = (n + S - 1) / S;
  std::vector<int32_t> chain((size_t)n, -1), ia((size_t)(n - 1));
  std::vector<double> meas((size_t)(3 * (n - 1)));
  for (long i = 0; i + 1 < n; ++i) {
    int rev;
    if (fscanf(in, "%d %lf %lf %lf", &rev, &meas[3 * i], &meas[3 * i + 1], &meas[3 * i + 2]) != 4) return 1;
    chain[i] = (int32_t)i;
    ia[i] = (int32_t)(rev ? i + 1 : i);
  }
  std::vector<long> ea((size_t)m), eb((size_t)m);
  std::vector<double> em((size_t)(3 * m)), X((size_t)(3 * K));
  for (long e = 0; e < m; ++e)
    if (fscanf(in, "%ld %ld %lf %lf %lf", &ea[e], &eb[e], &em[3 * e], &em[3 * e + 1], &em[3 * e + 2]) != 5 || ea[e] < 0 || ea[e] >= n ||
        eb[e] < 0 || eb[e] >= n)
      return 1;
  for (long k = 0; k < K; ++k)
    if (fscanf(in, "%lf %lf %lf", &X[3 * k], &X[3 * k + 1], &X[3 * k + 2]) != 3) return 1;
  fclose(in);
  std::vector<double> C((size_t)(3 * n)), Cend((size_t)(3 * (K - 1))), T((size_t)(3 * m)), P((size_t)(3 * n));
  pgo::coarsen_composites_serial(n, S, chain.data(), ia.data(), meas.data(), C.data(), Cend.data());
  for (long e = 0; e < m; ++e) {
    const double *ca = &C[3 * ea[e]], *cb = &C[3 * eb[e]];
    pgo::coarsen_transport(pgo::se2_make(ca[0], ca[1], ca[2]), em[3 * e], em[3 * e + 1], em[3 * e + 2], pgo::se2_make(cb[0], cb[1], cb[2]),
                           &T[3 * e]);
  }
  pgo::coarsen_prolong_serial(n, S, C.data(), Cend.data(), X.data(), P.data());
  FILE* out = fopen(argv[2], "w");
  if (!out) return 1;
  for (const std::vector<double>* v : {&C, &Cend, &T, &P})
    for (size_t i = 0; i < v->size(); i += 3) fprintf(out, "%.17g %.17g %.17g\n", (*v)[i], (*v)[i + 1], (*v)[i + 2]);
  if (fclose(out) != 0) return 1;
  printf("coarsen ok: %ld poses, %ld key poses, %ld edges\n", n, K, m);
  return 0;
}
