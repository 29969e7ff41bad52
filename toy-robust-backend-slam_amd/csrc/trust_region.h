#pragma once
// The step policy of Ceres' TrustRegionMinimizer + LevenbergMarquardtStrategy: ONE statement of the decisions,
// taken on the host by pgo_handle::lm_iteration / lm_iteration_tail and per problem by pgo_batch::iterate, on the device by
// k_window_solve (wavefront-uniform), and replayed on the CPU by tests/native/trust_region_main.cpp.  The callers keep their
// I/O, records, launches and iteration counters; where they differ on purpose is noted at the call sites.
#include <hip/hip_runtime.h>

#include <cmath>

#include "pgo.h"

namespace pgo {

constexpr double TR_DBL_MAX = 1.7976931348623157e308;   // the cost of a candidate that could not be evaluated

struct TrustRegion {
  double radius, decrease_factor;
  int invalid_run, prev_success;   // invalid steps in a row; the previous step was accepted (or there was none yet)
};
__host__ __device__ __forceinline__ TrustRegion tr_begin(double radius0) { return TrustRegion{radius0, 2.0, 0, 1}; }

// FinalizeIterationAndCheckIfMinimizerCanContinue, before a step: the PGO_TERM_* that ends the solve, or 0.
// iter: iterations done so far; gmax: gradient max-norm at the current point.
__host__ __device__ __forceinline__ int tr_stop_before_step(const TrustRegion& T, int iter, int max_iters, double gmax, double gtol,
                                                            double min_radius) {
  if (iter >= max_iters) return PGO_TERM_NO_CONVERGENCE;
  if (T.prev_success && gmax <= gtol) return PGO_TERM_CONVERGENCE_GTOL;
  return T.radius < min_radius ? PGO_TERM_MIN_RADIUS : 0;
}
// HandleUnsuccessfulStep / LevenbergMarquardtStrategy::StepRejected
__host__ __device__ __forceinline__ void tr_reject(TrustRegion& T) {
  T.radius /= T.decrease_factor;
  T.decrease_factor *= 2.0;
  T.prev_success = 0;
}
// is the linear solve's step usable: model decrease -(J d).(r + J d / 2) finite and > 0, |d|^2 finite?
__host__ __device__ __forceinline__ bool tr_step_usable(double model, double step2) {
  return std::isfinite(model) && std::isfinite(step2) && model > 0.0;
}
// a usable step ends the run of invalid ones
__host__ __device__ __forceinline__ void tr_valid_step(TrustRegion& T) { T.invalid_run = 0; }
// HandleInvalidStep: true on the fifth in a row (max_num_consecutive_invalid_steps: the solve has failed, nothing else
// changes), otherwise the radius shrinks as after a rejected step
__host__ __device__ __forceinline__ bool tr_invalid_step(TrustRegion& T) {
  if (++T.invalid_run >= 5) return true;
  tr_reject(T);
  return false;
}
// ParameterToleranceReached, then FunctionToleranceReached, on the candidate: PGO_TERM_CONVERGENCE_PTOL / _FTOL or 0
__host__ __device__ __forceinline__ int tr_tolerance_reached(double step_norm, double x_norm, double ptol, double cost_change,
                                                             double cost, double ftol) {
  if (step_norm <= ptol * (x_norm + ptol)) return PGO_TERM_CONVERGENCE_PTOL;
  return fabs(cost_change) <= ftol * cost ? PGO_TERM_CONVERGENCE_FTOL : 0;
}
// relative decrease; a candidate without a cost (TR_DBL_MAX) can never be accepted
__host__ __device__ __forceinline__ double tr_rho(double cand_cost, double cost_change, double model) {
  return (cand_cost >= TR_DBL_MAX) ? -TR_DBL_MAX : cost_change / model;
}
// HandleSuccessfulStep / LevenbergMarquardtStrategy::StepAccepted(rho)
__host__ __device__ __forceinline__ void tr_accept(TrustRegion& T, double rho, double max_radius) {
  const double t = 2.0 * rho - 1.0;
  T.radius = fmin(max_radius, T.radius / fmax(1.0 / 3.0, 1.0 - t * t * t));
  T.decrease_factor = 2.0;
  T.prev_success = 1;
}

}  // namespace pgo
