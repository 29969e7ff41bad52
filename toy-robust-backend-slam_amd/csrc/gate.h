#pragma once
// The 3x3 algebra of the loop-edge gate (include/pgo.h, "edge gate"): ONE statement of the formulas, evaluated by
// k_gate_reduce on the device (covariance.hip.h) and by pgo_gate_evaluate on the host.
//   chi2          = r' Omega r, clamped at 0                       (what pgo_edge_chi2 gives)
//   chi2_marginal = (L'r)' M^-1 (L'r) = r' (P + Omega^-1)^-1 r     Omega = L L', M = I + L' P L
//   info_gain     = 1/2 logdet M      = 1/2 logdet(I + Omega P)
// and of the joint gate ("joint edge gate"): the decision on one candidate, the pivot row and the downdate, evaluated by
// k_gate_joint_step on the device and by the serial loop of pgo_gate_joint_evaluate on the host (below).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "pgo.h"

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
// piv (the joint gate): on GATE_OK the factors the numbers were formed from, for gate_pivot_row.
struct GatePivot {
  double l[6], c[6], y[3];   // Omega = L L', M = C C' (both as gate_chol3 stores them), y = C^-1 L' r
};
__host__ __device__ inline int gate_evaluate(const double r[3], const double P[9], const double* info6, double out[3], GatePivot* piv = nullptr) {
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
  if (piv) {
    for (int i = 0; i < 6; ++i) {
      piv->l[i] = l[i];
      piv->c[i] = c[i];
    }
    piv->y[0] = y0;
    piv->y[1] = y1;
    piv->y[2] = y2;
  }
  return GATE_OK;
}

// ---------------------------------------------------------------- the joint gate (include/pgo.h, "joint edge gate")
// Candidates are decided one after the other on the working state (rho, M), M the joint covariance of the predicted
// residuals; an accepted candidate k conditions the rest on it: with B = M_[:, k] L C^-T,
//   rho_i <- rho_i - B_i y,   M_ij <- M_ij - B_i B_j'   (i, j > k),
// the Schur complement of M_kk + Omega_k^-1.  The three statements below are what k_gate_joint_step runs on the device and
// gate_joint_serial on the host.

// candidate k at the working state: its record from rho_k, M_kk, Omega_k (gate_evaluate), and the decision.  status 1: every
// double NaN, never accepted.  GATE_M_NOT_PD: chi2_cond and info_gain_cond NaN, not accepted (the caller names the candidate).
// force: -1 = the two tests, 0 = reject, 1 = accept.  piv is filled when the candidate is accepted.
__host__ __device__ inline int gate_joint_decide(const double rho[3], const double Mkk[9], const double* info6, int status, int force,
                                                 double chi2_gate, double min_info_gain, pgo_gate_joint_result* o, GatePivot* piv) {
  const double nan = NAN;
  o->status = status;
  o->accepted = 0;
  if (status) {
    for (int i = 0; i < 3; ++i) o->r_cond[i] = nan;
    for (int i = 0; i < 9; ++i) o->P_cond[i] = nan;
    o->chi2_cond = o->info_gain_cond = nan;
    return GATE_OK;
  }
  for (int i = 0; i < 3; ++i) o->r_cond[i] = rho[i];
  for (int i = 0; i < 9; ++i) o->P_cond[i] = Mkk[i];
  double res[3] = {nan, nan, nan};
  const int st = gate_evaluate(rho, Mkk, info6, res, piv);
  o->chi2_cond = res[1];
  o->info_gain_cond = res[2];
  if (st != GATE_OK) return st;
  o->accepted = force >= 0 ? (force == 1) : (res[1] <= chi2_gate && res[2] >= min_info_gain);
  return GATE_OK;
}

// row p of B from the row m = M[p][3k .. 3k + 2]:  b C' = m L
__host__ __device__ inline void gate_pivot_row(const GatePivot& v, const double m[3], double b[3]) {
  const double t0 = m[0] * v.l[0] + m[1] * v.l[1] + m[2] * v.l[3], t1 = m[1] * v.l[2] + m[2] * v.l[4], t2 = m[2] * v.l[5];
  b[0] = t0 / v.c[0];
  b[1] = (t1 - v.c[1] * b[0]) / v.c[2];
  b[2] = (t2 - v.c[3] * b[0] - v.c[4] * b[1]) / v.c[5];
}

// one entry of the downdate: m - b_p . b_q (symmetric in p, q: M stays exactly symmetric), and rho_p - b_p . y
__host__ __device__ inline double gate_downdate(double m, const double bp[3], const double bq[3]) {
  return m - (bp[0] * bq[0] + bp[1] * bq[1] + bp[2] * bq[2]);
}

// The serial loop (pgo_gate_joint_evaluate).  rho (3n) and M (3n x 3n row-major, symmetric) are the working state and are
// overwritten; B: 9n doubles of scratch.  Returns GATE_OK, or the first failing status with *bad = its candidate.
inline int gate_joint_serial(int n, double* rho, double* M, const double* info6, const int32_t* status, const int8_t* force, double chi2_gate,
                             double min_info_gain, pgo_gate_joint_result* joint, double* B, int* bad) {
  const int64_t W = 3 * (int64_t)n;
  for (int k = 0; k < n; ++k) {
    double Mkk[9];
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) Mkk[3 * a + b] = M[(3 * k + a) * W + 3 * k + b];
    GatePivot piv;
    const int st = gate_joint_decide(rho + 3 * k, Mkk, info6 ? info6 + 6 * (int64_t)k : nullptr, status ? status[k] : 0, force ? force[k] : -1,
                                     chi2_gate, min_info_gain, &joint[k], &piv);
    if (st != GATE_OK) {
      *bad = k;
      return st;
    }
    if (!joint[k].accepted) continue;
    for (int64_t p = 3 * (k + 1); p < W; ++p) gate_pivot_row(piv, M + p * W + 3 * k, B + 3 * p);
    for (int64_t p = 3 * (k + 1); p < W; ++p) {
      rho[p] = gate_downdate(rho[p], B + 3 * p, piv.y);
      for (int64_t q = 3 * (k + 1); q < W; ++q) M[p * W + q] = gate_downdate(M[p * W + q], B + 3 * p, B + 3 * q);
    }
  }
  return GATE_OK;
}

// n_accepted and the two sums over the accepted candidates, in candidate order
inline void gate_joint_summarise(int n, const pgo_gate_joint_result* joint, pgo_gate_joint_summary* sum) {
  sum->n_accepted = 0;
  sum->_pad = 0;
  sum->chi2_joint = sum->info_gain_joint = 0.0;
  for (int k = 0; k < n; ++k)
    if (joint[k].accepted) {
      ++sum->n_accepted;
      sum->chi2_joint += joint[k].chi2_cond;
      sum->info_gain_joint += joint[k].info_gain_cond;
    }
}

}  // namespace pgo
