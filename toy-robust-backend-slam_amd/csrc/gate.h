#pragma once
// The 3x3 algebra of the loop-edge gate (include/pgo.h, "edge gate"): ONE statement of the formulas, evaluated by
// k_gate_reduce on the device (covariance.hip.h) and by pgo_gate_evaluate on the host.
//   chi2          = r' Omega r, clamped at 0                       (what pgo_edge_chi2 gives)
//   chi2_marginal = (L'r)' M^-1 (L'r) = r' (P + Omega^-1)^-1 r     Omega = L L', M = I + L' P L
//   info_gain     = 1/2 logdet M      = 1/2 logdet(I + Omega P)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

namespace pgo {

constexpr int GATE_OK = 0, GATE_OMEGA_NOT_PD = 1, GATE_M_NOT_PD = 2;

// (isfinite that is the same statement on both sides)
__host__ __device__ inline bool gate_finite(double x) { return x - x == 0.0; }

// lower Cholesky factor (l00 l10 l11 l20 l21 l22) of the symmetric matrix (w00 w01 w02 w11 w12 w22); false when a pivot
// is not finite and > 0
__host__ __device__ inline bool gate_chol3(const double w[6], double l[6]) {
  if (!(w[0] > 0.0) || !gate_finite(w[0])) return false;
  l[0] = sqrt(w[0]);
  l[1] = w[1] / l[0];
  l[3] = w[2] / l[0];
  const double d1 = w[3] - l[1] * l[1];
  if (!(d1 > 0.0) || !gate_finite(d1)) return false;
  l[2] = sqrt(d1);
  l[4] = (w[4] - l[3] * l[1]) / l[2];
  const double d2 = w[5] - l[3] * l[3] - l[4] * l[4];
  if (!(d2 > 0.0) || !gate_finite(d2)) return false;
  l[5] = sqrt(d2);
  return gate_finite(l[1]) && gate_finite(l[3]) && gate_finite(l[4]);
}

// r: the plain residual; P: row-major 3x3, symmetric; info6: (I11 I12 I13 I22 I23 I33) or nullptr = the identity.
// out = {chi2, chi2_marginal, info_gain}.  GATE_OMEGA_NOT_PD: nothing written; GATE_M_NOT_PD: chi2 alone.
__host__ __device__ inline int gate_evaluate(const double r[3], const double P[9], const double* info6, double out[3]) {
  const double ident[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 1.0};
  const double* w = info6 ? info6 : ident;
  double l[6];
  if (!gate_chol3(w, l)) return GATE_OMEGA_NOT_PD;
  const double m = r[0] * (w[0] * r[0] + w[1] * r[1] + w[2] * r[2]) + r[1] * (w[1] * r[0] + w[3] * r[1] + w[4] * r[2]) +
                   r[2] * (w[2] * r[0] + w[4] * r[1] + w[5] * r[2]);
  out[0] = m < 0.0 ? 0.0 : m;
  // T = P L (columns of L: (l00 l10 l20), (0 l11 l21), (0 0 l22)), then M = I + L' T, lower triangle
  double T[9];
  for (int i = 0; i < 3; ++i) {
    T[3 * i] = P[3 * i] * l[0] + P[3 * i + 1] * l[1] + P[3 * i + 2] * l[3];
    T[3 * i + 1] = P[3 * i + 1] * l[2] + P[3 * i + 2] * l[4];
    T[3 * i + 2] = P[3 * i + 2] * l[5];
  }
  double M[6];   // 00 01 02 11 12 22
  M[0] = 1.0 + (l[0] * T[0] + l[1] * T[3] + l[3] * T[6]);
  M[1] = l[0] * T[1] + l[1] * T[4] + l[3] * T[7];
  M[2] = l[0] * T[2] + l[1] * T[5] + l[3] * T[8];
  M[3] = 1.0 + (l[2] * T[4] + l[4] * T[7]);
  M[4] = l[2] * T[5] + l[4] * T[8];
  M[5] = 1.0 + l[5] * T[8];
  double c[6];
  if (!gate_chol3(M, c)) return GATE_M_NOT_PD;
  // y = C^-1 (L' r): |y|^2 = (L'r)' M^-1 (L'r)
  const double v0 = l[0] * r[0] + l[1] * r[1] + l[3] * r[2], v1 = l[2] * r[1] + l[4] * r[2], v2 = l[5] * r[2];
  const double y0 = v0 / c[0];
  const double y1 = (v1 - c[1] * y0) / c[2];
  const double y2 = (v2 - c[3] * y0 - c[4] * y1) / c[5];
  out[1] = y0 * y0 + y1 * y1 + y2 * y2;
  out[2] = log(c[0]) + log(c[2]) + log(c[5]);   // 1/2 logdet M = sum log diag(C)
  return GATE_OK;
}

}  // namespace pgo
