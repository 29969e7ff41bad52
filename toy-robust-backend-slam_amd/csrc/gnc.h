#pragma once
// Graduated non-convexity with the truncated-least-squares surrogate (GNC-TLS; Yang, Antonante, Tzoumas, Carlone, "Graduated
// Non-Convexity for Robust Spatial Perception", RA-L 2020, eqs. (13)-(14) and remark 5): ONE statement of the weight update and
// of the first control parameter, in plain doubles -- evaluated by k_gnc_update on the device (gnc.hip.h), by pgo_gnc_weight_eval
// and the outer loop on the host (solver_gnc.hip), by the C++ mirror (host/) and by the stand-alone program tests/native/gnc_main.cpp.
//   c2 = cbar^2: the squared residual above which an edge is an outlier;  s = |e|^2 of the plain residual;  mu > 0 grows from
//   mu0 (the surrogate is convex in the limit mu -> 0) by a constant factor per round (the surrogate tends to TLS).
#include <hip/hip_runtime.h>

#include <cmath>

namespace pgo {

// the first mu: every selected residual lies inside the upper threshold, so that no weight starts at 0.  Valid only for
// 2 rmax2 > c2 -- otherwise every residual is an inlier already and there is nothing to graduate.
__host__ __device__ inline double gnc_mu0(double c2, double rmax2) { return c2 / (2.0 * rmax2 - c2); }

// the TLS weight: 1 up to mu / (mu + 1) c2, 0 from (mu + 1) / mu c2, sqrt(c2 mu (mu + 1) / s) - mu between.  A non-finite s
// (an edge that cannot be evaluated) is an outlier: weight 0.
__host__ __device__ inline double gnc_tls_weight(double c2, double mu, double s) {
  if (!(s - s == 0.0)) return 0.0;   // NaN, +-inf (no isfinite: one spelling for host and device)
  const double lo = mu / (mu + 1.0) * c2, hi = (mu + 1.0) / mu * c2;
  if (s <= lo) return 1.0;
  if (s >= hi) return 0.0;
  // (between the thresholds the expression lies in [0, 1] up to the rounding of the subtraction, ~ulp(mu): clamped, so that a
  // weight is always one pgo_set_edge_weights takes)
  return fmin(1.0, fmax(0.0, sqrt(c2 * mu * (mu + 1.0) / s) - mu));
}

}  // namespace pgo
