// The chordal initialisation of csrc/chordal.h on the host: what pgo_chordal_plan runs and the kernels of chordal.hip.h evaluate,
// compiled by g++ with AddressSanitizer + UndefinedBehaviorSanitizer.
//     chordal_main IN OUT
// IN:  "n E rtol max_iters mag_min rounds reject_xy reject_th", then n lines "x y theta constant" (the poses and the mask),
//      then E lines "a b mx my mt w" (the caller's order).
// OUT: n lines "x y theta", E lines "res_xy res_th w_out", one line "n_solves n_rejected n_degenerate min_mag", then per solve
//      "iters_R iters_T converged_R converged_T rel_R rel_T" (17 digits).
// Built and run by tests/test_chordal_native.py.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "chordal.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "r");
  if (!in) return 1;
  long n, E, max_iters, rounds;
  pgo_chordal_options o{};
  if (fscanf(in, "%ld %ld %lf %ld %lf %ld %lf %lf", &n, &E, &o.rtol, &max_iters, &o.mag_min, &rounds, &o.reject_xy, &o.reject_th) != 8 || n < 2 || E < n - 1)
    return 1;
  o.max_iters = (int32_t)max_iters;
  o.rounds = (int32_t)rounds;
  o.check_every = 50;
  if (!pgo::chordal_options_ok(&o)) return 1;
  std::vector<double> poses((size_t)(3 * n)), meas((size_t)(3 * E)), u((size_t)E);
  std::vector<uint8_t> is_const((size_t)n);
  std::vector<int32_t> ia((size_t)E), ib((size_t)E);
  for (long i = 0; i < n; ++i) {
    int c;
    if (fscanf(in, "%lf %lf %lf %d", &poses[3 * i], &poses[3 * i + 1], &poses[3 * i + 2], &c) != 4) return 1;
    is_const[i] = c != 0;
  }
  for (long e = 0; e < E; ++e) {
    if (fscanf(in, "%d %d %lf %lf %lf %lf", &ia[e], &ib[e], &meas[3 * e], &meas[3 * e + 1], &meas[3 * e + 2], &u[e]) != 6 || ia[e] < 0 || ia[e] >= n ||
        ib[e] < 0 || ib[e] >= n)
      return 1;
    if (ia[e] == ib[e]) u[e] = 0.0;
  }
  fclose(in);
  const std::vector<double> w(u);
  // the chain: the first edge between i and i + 1, in either orientation
  std::vector<int32_t> chain((size_t)n, -1);
  for (long e = 0; e < E; ++e) {
    const int32_t lo = std::min(ia[e], ib[e]), hi = std::max(ia[e], ib[e]);
    if (hi == lo + 1 && chain[lo] < 0) chain[lo] = (int32_t)e;
  }
  for (long i = 0; i + 1 < n; ++i)
    if (chain[i] < 0) return 1;
  std::vector<double> T((size_t)(n * pgo::SUPPORT_POSE));
  pgo::support_trajectory_serial(n, chain.data(), ia.data(), meas.data(), T.data());
  std::vector<double> out((size_t)(3 * n)), res((size_t)(2 * E) + 1);
  pgo_chordal_summary sum;
  int32_t where = -1;
  const int st = pgo::chordal_serial(n, E, ia.data(), ib.data(), meas.data(), poses.data(), is_const.data(), chain.data(), T.data(), &o, u.data(), out.data(),
                                     res.data(), &sum, &where);
  if (st != PGO_OK) {
    printf("chordal status %d at %d\n", st, where);
    return 3;
  }
  FILE* f = fopen(argv[2], "w");
  if (!f) return 1;
  for (long i = 0; i < n; ++i) fprintf(f, "%.17g %.17g %.17g\n", out[3 * i], out[3 * i + 1], out[3 * i + 2]);
  for (long e = 0; e < E; ++e) fprintf(f, "%.17g %.17g %.17g\n", res[2 * e], res[2 * e + 1], w[e] > 0.0 && !(u[e] > 0.0) ? 0.0 : w[e]);
  fprintf(f, "%d %d %d %.17g\n", sum.n_solves, sum.n_rejected, sum.n_degenerate, sum.min_mag);
  for (int k = 0; k < sum.n_solves; ++k) {
    const pgo_chordal_solve& S = sum.solve[k];
    fprintf(f, "%d %d %d %d %.17g %.17g\n", S.iters[0], S.iters[1], S.converged[0], S.converged[1], S.rel_residual[0], S.rel_residual[1]);
  }
  if (fclose(f) != 0) return 1;
  printf("chordal ok: %ld poses, %ld edges, %d solves\n", n, E, sum.n_solves);
  return 0;
}
