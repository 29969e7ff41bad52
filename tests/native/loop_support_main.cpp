// The loop support statement of csrc/loop_support.h on the host: what pgo_loop_support_plan runs and the kernels of
// loop_support.hip.h evaluate, compiled by g++ with AddressSanitizer + UndefinedBehaviorSanitizer.
//     loop_support_main IN OUT
// IN:  "n E window tol_xy tol_th min_support", then E lines "a b mx my mt selected" (the caller's order; `selected` already
//      resolved from kind or mask, chain edges included -- they are taken out here).
// OUT: n lines "x y theta" (T), E lines "selected n_pairs n_consistent best q_min", one line "n_selected n_supported
//      n_pairs_total max_pairs" (17 digits).
// Built and run by tests/test_loop_support_native.py.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "loop_support.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "r");
  if (!in) return 1;
  long n, E, window, min_support;
  double tol_xy, tol_th;
  if (fscanf(in, "%ld %ld %ld %lf %lf %ld", &n, &E, &window, &tol_xy, &tol_th, &min_support) != 6 || n < 2 || E < n - 1 || window < 1) return 1;
  std::vector<int32_t> ia((size_t)E), ib((size_t)E);
  std::vector<double> meas((size_t)(3 * E));
  std::vector<uint8_t> sel((size_t)E);
  for (long e = 0; e < E; ++e) {
    int s;
    if (fscanf(in, "%d %d %lf %lf %lf %d", &ia[e], &ib[e], &meas[3 * e], &meas[3 * e + 1], &meas[3 * e + 2], &s) != 6 || ia[e] < 0 || ia[e] >= n ||
        ib[e] < 0 || ib[e] >= n)
      return 1;
    sel[e] = s != 0;
  }
  fclose(in);
  // the chain: the first edge between i and i + 1, in either orientation
  std::vector<int32_t> chain((size_t)n, -1);
  for (long e = 0; e < E; ++e) {
    const int32_t lo = std::min(ia[e], ib[e]), hi = std::max(ia[e], ib[e]);
    if (hi == lo + 1 && chain[lo] < 0) chain[lo] = (int32_t)e;
  }
  for (long i = 0; i + 1 < n; ++i) {
    if (chain[i] < 0) return 1;
    sel[chain[i]] = 0;
  }
  const int P = pgo::SUPPORT_POSE;
  std::vector<double> T((size_t)(n * P));
  pgo::support_trajectory_serial(n, chain.data(), ia.data(), meas.data(), T.data());
  std::vector<int32_t> s_edge, s_lo, s_hi, first;
  pgo::support_sort(n, E, ia.data(), ib.data(), sel.data(), &s_edge, &s_lo, &s_hi, &first, nullptr);
  std::vector<double> minv(s_edge.size() * P + 1);
  for (size_t r = 0; r < s_edge.size(); ++r) {
    const long e = s_edge[r];
    pgo::support_store(&minv[r * P], pgo::se2_inverse(pgo::support_canonical(ia[e], ib[e], meas[3 * e], meas[3 * e + 1], meas[3 * e + 2])));
  }
  FILE* out = fopen(argv[2], "w");
  if (!out) return 1;
  for (long i = 0; i < n; ++i) fprintf(out, "%.17g %.17g %.17g\n", T[i * P], T[i * P + 1], T[i * P + 2]);
  long n_selected = 0, n_supported = 0, max_pairs = 0;
  long long n_pairs_total = 0;
  for (long e = 0; e < E; ++e) {
    pgo::SupportAcc R = pgo::support_acc_begin();
    if (sel[e]) {
      const int32_t lo = std::min(ia[e], ib[e]), hi = std::max(ia[e], ib[e]);
      int64_t r0, r1;
      pgo::support_range(first.data(), (int32_t)n, lo, (int32_t)window, &r0, &r1);
      R = pgo::support_scan((int32_t)e, lo, hi, pgo::support_canonical(ia[e], ib[e], meas[3 * e], meas[3 * e + 1], meas[3 * e + 2]), r0, r1,
                            s_edge.data(), s_lo.data(), s_hi.data(), minv.data(), T.data(), (int32_t)window, tol_xy * tol_xy, tol_th * tol_th);
      ++n_selected;
      n_supported += R.n_consistent >= min_support;
      n_pairs_total += R.n_pairs;
      max_pairs = std::max<long>(max_pairs, R.n_pairs);
    }
    fprintf(out, "%d %d %d %d %.17g\n", sel[e] ? 1 : 0, R.n_pairs, R.n_consistent, R.best, R.q_min);
  }
  fprintf(out, "%ld %ld %lld %ld\n", n_selected, n_supported, n_pairs_total, max_pairs);
  if (fclose(out) != 0) return 1;
  printf("loop support ok: %ld poses, %ld edges, %ld selected\n", n, E, n_selected);
  return 0;
}
