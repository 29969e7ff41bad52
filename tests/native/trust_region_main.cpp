// The trust-region step policy of csrc/trust_region.h on the host: what pgo_handle::lm_iteration, pgo_batch::iterate and
// k_window_solve decide with, compiled by g++ with AddressSanitizer + UndefinedBehaviorSanitizer.
//     trust_region_main replay IN OUT     replay recorded trajectories (tests/golden/lm_*.json, flattened by the test)
//     trust_region_main drive             the cases the fixtures do not hold, printed as `name value` lines
// IN:  "seq N" then N lines "code rho previous_radius", code: 1 accepted, 0 rejected, -1 invalid, 2 ended on a tolerance (no
//      update).  Each step starts from the RECORDED previous radius (no accumulation); the decrease factor is carried along
//      the sequence.  OUT: the radius after every step, 17 digits.
// Built and run by tests/test_trust_region_host.py.
#include <cstdio>
#include <cstring>

#include "trust_region.h"

static int replay(const char* in_path, const char* out_path) {
  FILE* in = fopen(in_path, "r");
  FILE* out = fopen(out_path, "w");
  if (!in || !out) return 1;
  int n;
  long steps = 0;
  while (fscanf(in, " seq %d", &n) == 1) {
    pgo::TrustRegion T = pgo::tr_begin(0.0);
    for (int i = 0; i < n; ++i) {
      int code;
      double rho, prev;
      if (fscanf(in, "%d %lf %lf", &code, &rho, &prev) != 3) return 1;
      T.radius = prev;
      if (code == 1) pgo::tr_accept(T, rho, 1e16);
      else if (code == 0) pgo::tr_reject(T);
      else if (code == -1) (void)pgo::tr_invalid_step(T);
      fprintf(out, "%.17g\n", T.radius);
      ++steps;
    }
  }
  fclose(in);
  if (fclose(out) != 0) return 1;
  printf("trust region replay ok: %ld steps\n", steps);
  return 0;
}

static int drive() {
  const double DMAX = pgo::TR_DBL_MAX;
  // five invalid steps in a row from radius 1024
  pgo::TrustRegion T = pgo::tr_begin(1024.0);
  for (int k = 1; k <= 5; ++k) {
    const bool usable = pgo::tr_step_usable(k == 2 ? 0.0 : (k == 3 ? -1.0 : NAN), k == 4 ? INFINITY : 1.0);
    const bool failed = usable ? false : pgo::tr_invalid_step(T);
    printf("invalid%d_usable %d\ninvalid%d_failed %d\ninvalid%d_radius %.17g\ninvalid%d_prev_success %d\n", k, (int)usable, k, (int)failed,
           k, T.radius, k, T.prev_success);
  }
  // a usable step ends the run: four invalid, one usable, four invalid again do not fail
  T = pgo::tr_begin(1.0);
  int failures = 0;
  for (int k = 0; k < 9; ++k) {
    if (k == 4) {
      failures += pgo::tr_step_usable(1.0, 1.0) ? 0 : 100;
      pgo::tr_valid_step(T);
    } else if (!pgo::tr_step_usable(-1.0, 1.0)) {
      failures += pgo::tr_invalid_step(T) ? 1 : 0;
    }
  }
  printf("run_reset_failures %d\n", failures);
  // a rejection after an acceptance starts again at factor 2
  T = pgo::tr_begin(100.0);
  pgo::tr_reject(T);
  pgo::tr_reject(T);
  printf("reject2_radius %.17g\nreject2_factor %.17g\n", T.radius, T.decrease_factor);
  pgo::tr_accept(T, 0.5, 1e16);   // rho = 1/2: 1 - (2 rho - 1)^3 = 1, the radius stays
  printf("accept_half_radius %.17g\naccept_factor %.17g\naccept_prev_success %d\n", T.radius, T.decrease_factor, T.prev_success);
  pgo::tr_reject(T);
  printf("reject_after_accept_radius %.17g\nreject_after_accept_factor %.17g\nreject_prev_success %d\n", T.radius, T.decrease_factor,
         T.prev_success);
  // the accept rule: growth capped at 3, and at max_radius
  T = pgo::tr_begin(10.0);
  pgo::tr_accept(T, 1.0, 1e16);
  printf("accept_one_radius %.17g\n", T.radius);
  pgo::tr_accept(T, 1.0, 50.0);
  printf("accept_capped_radius %.17g\n", T.radius);
  T = pgo::tr_begin(10.0);
  pgo::tr_accept(T, 0.25, 1e16);   // 1 - (-1/2)^3 = 9/8
  printf("accept_quarter_radius %.17g\n", T.radius);
  // tolerances: ptol is tested first
  printf("tol_both %d\ntol_ptol %d\ntol_ftol %d\ntol_none %d\n", pgo::tr_tolerance_reached(1e-9, 1.0, 1e-8, 1e-9, 1.0, 1e-6),
         pgo::tr_tolerance_reached(1e-9, 1.0, 1e-8, 1.0, 1.0, 1e-6), pgo::tr_tolerance_reached(1.0, 1.0, 1e-8, -1e-9, 1.0, 1e-6),
         pgo::tr_tolerance_reached(1.0, 1.0, 1e-8, 1.0, 1.0, 1e-6));
  // the stops before a step, in their order
  T = pgo::tr_begin(1.0);
  printf("stop_none %d\n", pgo::tr_stop_before_step(T, 3, 50, 1.0, 1e-10, 1e-32));
  printf("stop_iters %d\n", pgo::tr_stop_before_step(T, 50, 50, 0.0, 1e-10, 1e-32));
  printf("stop_gtol %d\n", pgo::tr_stop_before_step(T, 3, 50, 1e-10, 1e-10, 1e-32));
  T.radius = 1e-33;
  printf("stop_gtol_before_radius %d\n", pgo::tr_stop_before_step(T, 3, 50, 0.0, 1e-10, 1e-32));
  printf("stop_min_radius %d\n", pgo::tr_stop_before_step(T, 3, 50, 1.0, 1e-10, 1e-32));
  T = pgo::tr_begin(1.0);
  pgo::tr_reject(T);   // gtol is tested only after a successful step
  printf("stop_gtol_after_reject %d\n", pgo::tr_stop_before_step(T, 3, 50, 0.0, 1e-10, 1e-32));
  // rho
  printf("rho_plain %.17g\n", pgo::tr_rho(1.0, 3.0, 4.0));
  printf("rho_dbl_max_is_minus_dbl_max %d\n", (int)(pgo::tr_rho(DMAX, 1.0 - DMAX, 1.0) == -DMAX));
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 4 && !strcmp(argv[1], "replay")) return replay(argv[2], argv[3]);
  if (argc >= 2 && !strcmp(argv[1], "drive")) return drive();
  return 2;
}
