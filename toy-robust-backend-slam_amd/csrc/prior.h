#pragma once
// The absolute pose prior (include/pgo.h, "pose priors"): ONE statement of the unary SE(2) factor, evaluated on the device by
// k_prior_eval (prior.hip.h) and on the host by pgo_prior_eval and tests/native/prior_main.cpp.  Plain doubles and
// compile-time indices only: a lane-dependent index goes through scratch.
//   d    = (x - zx, y - zy, remainder(t - zt, 2 pi))      the IEEE remainder: d_theta in [-pi, pi]; d d / d pose = I
//   q    = Lambda d,   chi2 = max(0, d'q)                  (Lambda positive SEMI-definite: rounding may leave d'q at -1e-17)
//   cost = 1/2 rho(chi2);  with the corrector the rows are scaled by sqrt(rho'): J'J = rho' Lambda, J'r = rho' q
// Lambda is given as I11 I12 I13 I22 I23 I33, the order of the edges' information matrices.
#include <hip/hip_runtime.h>

#include <cmath>

#include "loss.h"

namespace pgo {

constexpr double PRIOR_TWO_PI = 6.283185307179586476925286766559;
// An information matrix is accepted when its smallest eigenvalue is >= -PRIOR_PSD_RTOL x its largest absolute eigenvalue
// (what forming Q Omega Q' or summing outer products in floating point leaves of an exact zero), and counts as positive
// DEFINITE -- a gauge, for the calls that need one -- when its smallest eigenvalue is > +PRIOR_PSD_RTOL x the largest.
constexpr double PRIOR_PSD_RTOL = 1e-12;

__host__ __device__ __forceinline__ void prior_residual(double x, double y, double t, double zx, double zy, double zt, double& d0,
                                                        double& d1, double& d2) {
  d0 = x - zx;
  d1 = y - zy;
  d2 = remainder(t - zt, PRIOR_TWO_PI);
}

// q = Lambda d; returns chi2 = max(0, d'q)
__host__ __device__ __forceinline__ double prior_chi2(double l00, double l01, double l02, double l11, double l12, double l22, double d0,
                                                      double d1, double d2, double& q0, double& q1, double& q2) {
  q0 = l00 * d0 + l01 * d1 + l02 * d2;
  q1 = l01 * d0 + l11 * d1 + l12 * d2;
  q2 = l02 * d0 + l12 * d1 + l22 * d2;
  const double s = d0 * q0 + d1 * q1 + d2 * q2;
  return s < 0.0 ? 0.0 : s;
}

// the whole factor at one pose: d, q = Lambda d, chi2 and rho[0..2] of the loss at chi2
__host__ __device__ __forceinline__ void prior_eval(const LossClass& loss, double x, double y, double t, double zx, double zy, double zt,
                                                    double l00, double l01, double l02, double l11, double l12, double l22, double& d0,
                                                    double& d1, double& d2, double& q0, double& q1, double& q2, double& chi2,
                                                    double rho[3]) {
  prior_residual(x, y, t, zx, zy, zt, d0, d1, d2);
  chi2 = prior_chi2(l00, l01, l02, l11, l12, l22, d0, d1, d2, q0, q1, q2);
  loss_rho(loss, chi2, rho);
}

// ---- host only: what pgo_set_priors checks of an information matrix
// eigenvalues of the symmetric 3x3 matrix m = (00 01 02 11 12 22) by cyclic Jacobi rotations on the matrix scaled to unit
// largest entry; ev is NOT sorted.  A zero matrix gives zeros.
inline void prior_sym3_eigenvalues(const double m[6], double ev[3]) {
  double big = 0.0;
  for (int k = 0; k < 6; ++k) big = std::fmax(big, std::fabs(m[k]));
  if (!(big > 0.0)) {
    ev[0] = ev[1] = ev[2] = 0.0;
    return;
  }
  double a[3][3] = {{m[0] / big, m[1] / big, m[2] / big}, {m[1] / big, m[3] / big, m[4] / big}, {m[2] / big, m[4] / big, m[5] / big}};
  for (int sweep = 0; sweep < 64; ++sweep) {
    const double off = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
    if (off < 1e-300) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        if (a[p][q] == 0.0) continue;
        const double theta = (a[q][q] - a[p][p]) / (2.0 * a[p][q]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; ++k) {   // A <- A G
          const double akp = a[k][p], akq = a[k][q];
          a[k][p] = c * akp - s * akq;
          a[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 3; ++k) {   // A <- G' A
          const double apk = a[p][k], aqk = a[q][k];
          a[p][k] = c * apk - s * aqk;
          a[q][k] = s * apk + c * aqk;
        }
      }
  }
  for (int k = 0; k < 3; ++k) ev[k] = a[k][k] * big;
}

enum PriorInfoClass { PRIOR_INFO_NOT_FINITE = -2, PRIOR_INFO_INDEFINITE = -1, PRIOR_INFO_PSD = 0, PRIOR_INFO_PD = 1 };

inline PriorInfoClass prior_info_class(const double info6[6]) {
  for (int k = 0; k < 6; ++k)
    if (!std::isfinite(info6[k])) return PRIOR_INFO_NOT_FINITE;
  double ev[3];
  prior_sym3_eigenvalues(info6, ev);
  const double lo = std::fmin(ev[0], std::fmin(ev[1], ev[2]));
  const double top = std::fmax(std::fabs(ev[0]), std::fmax(std::fabs(ev[1]), std::fabs(ev[2])));
  if (lo < -PRIOR_PSD_RTOL * top) return PRIOR_INFO_INDEFINITE;
  return lo > PRIOR_PSD_RTOL * top ? PRIOR_INFO_PD : PRIOR_INFO_PSD;
}

}  // namespace pgo
