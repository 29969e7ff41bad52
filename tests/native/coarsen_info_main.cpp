// The pair operations of csrc/coarsen.h (motion, covariance) on the host: the statement pgo_coarsen_info_plan runs and the
// kernels k_chain_compose_info / k_coarsen_edges_info evaluate, compiled by g++ with AddressSanitizer +
// UndefinedBehaviorSanitizer.
//     coarsen_info_main IN OUT
// IN:  "n stride m", then n - 1 lines "reversed mx my mt w0..w5" (the chain edge of the pair (i, i + 1), stored as (i + 1, i)
//      when reversed, with its information in the order of info6), then m lines "a b mx my mt w0..w5" (other edges).
// OUT: n lines of the covariance of C, K - 1 lines of the covariance of Cend, then per other edge two lines: the covariance of
//      pair(C_a) o (m, Omega^-1) o pair(C_b)^-1 and its information (17 digits).
// An information matrix that is not positive definite: exit status 3.  Built and run by tests/test_coarsen_info_native.py.
#include <cstdio>
#include <cstring>
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
  std::vector<double> meas((size_t)(3 * (n - 1))), info((size_t)(6 * (n - 1)));
  for (long i = 0; i + 1 < n; ++i) {
    int rev;
    if (fscanf(in, "%d %lf %lf %lf", &rev, &meas[3 * i], &meas[3 * i + 1], &meas[3 * i + 2]) != 4) return 1;
    for (int c = 0; c < 6; ++c)
      if (fscanf(in, "%lf", &info[6 * i + c]) != 1) return 1;
    chain[i] = (int32_t)i;
    ia[i] = (int32_t)(rev ? i + 1 : i);
  }
  std::vector<long> ea((size_t)m), eb((size_t)m);
  std::vector<double> em((size_t)(3 * m)), ew((size_t)(6 * m));
  for (long e = 0; e < m; ++e) {
    if (fscanf(in, "%ld %ld %lf %lf %lf", &ea[e], &eb[e], &em[3 * e], &em[3 * e + 1], &em[3 * e + 2]) != 5 || ea[e] < 0 || ea[e] >= n ||
        eb[e] < 0 || eb[e] >= n)
      return 1;
    for (int c = 0; c < 6; ++c)
      if (fscanf(in, "%lf", &ew[6 * e + c]) != 1) return 1;
  }
  fclose(in);
  std::vector<double> C((size_t)(3 * n)), Cend((size_t)(3 * (K - 1))), Cw((size_t)(6 * n)), Cew((size_t)(6 * (K - 1))), T((size_t)(12 * m));
  if (pgo::coarsen_composites_info_serial(n, S, chain.data(), ia.data(), meas.data(), info.data(), C.data(), Cend.data(), Cw.data(), Cew.data()) >= 0)
    return 3;
  for (long e = 0; e < m; ++e) {
    pgo::Se2Cov Pa, Pb;
    Pa.m = pgo::se2_make(C[3 * ea[e]], C[3 * ea[e] + 1], C[3 * ea[e] + 2]);
    Pb.m = pgo::se2_make(C[3 * eb[e]], C[3 * eb[e] + 1], C[3 * eb[e] + 2]);
    memcpy(Pa.v, &Cw[6 * ea[e]], 48);
    memcpy(Pb.v, &Cw[6 * eb[e]], 48);
    double mm[3];
    if (!pgo::coarsen_transport_pair(Pa, em[3 * e], em[3 * e + 1], em[3 * e + 2], &ew[6 * e], Pb, mm, &T[12 * e])) return 3;
    pgo::coarsen_info_of(&T[12 * e], &T[12 * e + 6]);
  }
  FILE* out = fopen(argv[2], "w");
  if (!out) return 1;
  for (const std::vector<double>* v : {&Cw, &Cew, &T})
    for (size_t i = 0; i < v->size(); i += 6)
      fprintf(out, "%.17g %.17g %.17g %.17g %.17g %.17g\n", (*v)[i], (*v)[i + 1], (*v)[i + 2], (*v)[i + 3], (*v)[i + 4], (*v)[i + 5]);
  if (fclose(out) != 0) return 1;
  printf("coarsen info ok: %ld poses, %ld key poses, %ld edges\n", n, K, m);
  return 0;
}
