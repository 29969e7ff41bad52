#pragma once
// The SE(2) edge model (src/ceres_error.cpp of the reference in closed form): ONE statement of the formulas,
// evaluated on the device by k_edge_eval (K1), k_edge_chi2, k_gate_eval and win_edge_eval (k_window_solve), and on the host by
// tests/native/edge_model_main.cpp.  Plain doubles and compile-time indices only: a lane-dependent index goes through scratch.
//   diff = T^-1 (Ta^-1 Tb),  e = (ex, ey, heading(sin delta)),  delta = t2 - t1 - dth
// The heading is the CALLER's: asin(sind) in K1 and the window, asin(clamp(sind, -1, 1)) in the chi2 and gate residuals.
#include <hip/hip_runtime.h>

#include <cmath>

#include "loss.h"

namespace pgo {

// ex, ey and sin delta of one edge at poses (x1, y1, t1), (x2, y2, t2) with measurement (dx, dy, dth).  WITH_JAC: also
// J[18] = [d e / d Pa | d e / d Pb], 3 x 6 row-major, the heading row for asin(sind): g = cos delta / sqrt(1 - sin^2 delta),
// unclamped (not finite at |sin delta| = 1).  J is not touched without WITH_JAC (it may be nullptr).
template <bool WITH_JAC>
__host__ __device__ __forceinline__ void edge_plain(double x1, double y1, double t1, double x2, double y2, double t2, double dx,
                                                    double dy, double dth, double& ex, double& ey, double& sind, double* J) {
  double s1, c1, s2, c2, sd, cd;
  sincos(t1, &s1, &c1);
  sincos(t2, &s2, &c2);
  sincos(dth, &sd, &cd);
  const double Dx = x2 - x1, Dy = y2 - y1;
  const double pa = c1 * Dx + s1 * Dy, pb = -s1 * Dx + c1 * Dy;  // R(t1)' D
  const double ux = pa - dx, uy = pb - dy;
  ex = cd * ux + sd * uy;                                          // R(dth)' u
  ey = -sd * ux + cd * uy;
  const double c21 = c1 * c2 + s1 * s2, s21 = c1 * s2 - s1 * c2;  // R(t2 - t1)
  sind = cd * s21 - sd * c21;
  if (WITH_JAC) {
    const double cosd = cd * c21 + sd * s21;
    const double cm = c1 * cd - s1 * sd, sm = s1 * cd + c1 * sd;  // R(t1 + dth)
    const double g = cosd / sqrt(1.0 - sind * sind);              // d asin(u) = du / sqrt(1-u^2)
    J[0] = -cm;  J[1] = -sm;  J[2] = cd * pb - sd * pa;   J[3] = cm;   J[4] = sm;   J[5] = 0.0;
    J[6] = sm;   J[7] = -cm;  J[8] = -sd * pb - cd * pa;  J[9] = -sm;  J[10] = cm;  J[11] = 0.0;
    J[12] = 0.0; J[13] = 0.0; J[14] = -g;                 J[15] = 0.0; J[16] = 0.0; J[17] = g;
  }
}

// DCS (src/ceres_error.cpp:185-193) on the plain objective: e <- psi e, psi = min(1, sqrt(2 phi / (phi + ex^2 + ey^2))),
// and with WITH_JAC J <- psi J + e dpsi'.  (The chi2 form for information-weighted edges is K1's alone: k_edge_eval.)
template <bool WITH_JAC>
__host__ __device__ __forceinline__ void edge_dcs(double phi, double& ex, double& ey, double& et, double* J) {
  const double res = ex * ex + ey * ey;
  const double psi = sqrt(2.0 * phi / (phi + res));
  if (psi < 1.0) {
    if (WITH_JAC) {
      const double k = -psi / (phi + res);
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const double dpsi = k * (ex * J[c] + ey * J[6 + c]);
        J[c] = psi * J[c] + ex * dpsi;
        J[6 + c] = psi * J[6 + c] + ey * dpsi;
        J[12 + c] = psi * J[12 + c] + et * dpsi;
      }
    }
    ex *= psi;
    ey *= psi;
    et *= psi;
  }
}

// the loss of class k (an edge's flags bits 2-3), picked field by field with selects: a lane-dependent index into an array of
// the classes would go through scratch.  BY VALUE: a reference into a kernel's argument block keeps a copy of it in scratch.
__host__ __device__ __forceinline__ LossClass pick_loss(LossClass l0, LossClass l1, LossClass l2, LossClass l3, unsigned k) {
  LossClass L;
  L.type = k == 0u ? l0.type : k == 1u ? l1.type : k == 2u ? l2.type : l3.type;
  L._pad = 0;
  L.a = k == 0u ? l0.a : k == 1u ? l1.a : k == 2u ? l2.a : l3.a;
  L.b = k == 0u ? l0.b : k == 1u ? l1.b : k == 2u ? l2.b : l3.b;
  L.c = k == 0u ? l0.c : k == 1u ? l1.c : k == 2u ? l2.c : l3.c;
  return L;
}

}  // namespace pgo
