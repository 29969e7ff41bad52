// Absolute pose priors on the device (include/pgo.h, "pose priors"; the model: prior.h).  The priors of a handle are kept
// sorted by internal row -- row [n] | caller's position [n] | mean planes [3][n] | information planes [6][n] -- so that both
// kernels walk the pose vector, the scales and the diagonal planes forwards.
//   k_prior_eval<WITH_JAC>   one lane per prior: cost partials per workgroup (they join K1's in eval_enqueue's reduction), the
//                            `bad` flag, and with the Jacobian the UNSCALED rho' Lambda | rho' Lambda d into a per-prior record
//                            [9][n] -- K2 runs later, and again after the Jacobi scales change
//   k_prior_add              after k_assemble: hd_i += S_i (rho' Lambda) S_i, gs_i += S_i (rho' Lambda d) with the CURRENT scales;
//                            rows are unique (at most one prior per pose): plain read-modify-writes, no atomics, the result is
//                            bitwise reproducible and independent of the grid.  The scaled block also goes into the dense planes
//                            the direct solve's k_dlr_setup adds to T's diagonal (nullptr on handles that never solve directly).
// Algorithmic bytes per prior: eval 4 + 24 + 24 + 48 read, 72 written with the Jacobian; add 4 + 72 + 24 read, 72 read and 72
// written in hd / gs (+ 48 written with the dense planes).
#pragma once
#include "kernels.hip.h"
#include "prior.h"

namespace pgo {
namespace dev {

constexpr int PRIOR_REC = 9;   // planes of the per-prior record: rho' Lambda (00 01 02 11 12 22) | rho' Lambda d (3)

struct PriorArgs {
  const double* poses;    // [.. x 3] global pose positions (internal numbering)
  const int32_t* row;     // [n] global row of each prior, ascending
  const double* mean;     // [3][n]
  const double* info;     // [6][n]
  double* rec;            // [PRIOR_REC][n], written WITH_JAC only
  int32_t n;
  int32_t apply_loss;
  LossClass loss;         // ONE loss for all priors of the handle
  // pgo_get_prior_residuals: the plain residual and chi2 in the CALLER's order; nullptr in the LM loop
  const int32_t* order;   // [n] caller's position of each sorted prior
  double* d_out;          // [n x 3]
  double* chi2_out;       // [n]
};

template <bool WITH_JAC>
__global__ __launch_bounds__(WG) void k_prior_eval(PriorArgs A, double* __restrict__ cost_part, int* __restrict__ bad) {
  __shared__ double red[8];
  const int64_t n = A.n;
  double cost = 0.0;
  for (int64_t k = (int64_t)blockIdx.x * WG + threadIdx.x; k < n; k += (int64_t)gridDim.x * WG) {
    const int64_t r = A.row[k];
    const double x = A.poses[3 * r], y = A.poses[3 * r + 1], t = A.poses[3 * r + 2];
    const double l00 = A.info[k], l01 = A.info[n + k], l02 = A.info[2 * n + k], l11 = A.info[3 * n + k], l12 = A.info[4 * n + k],
                 l22 = A.info[5 * n + k];
    double d0, d1, d2, q0, q1, q2, chi2, rho[3];
    prior_eval(A.loss, x, y, t, A.mean[k], A.mean[n + k], A.mean[2 * n + k], l00, l01, l02, l11, l12, l22, d0, d1, d2, q0, q1, q2, chi2,
               rho);   // (prior.h)
    cost += 0.5 * rho[0];
    const double w = A.apply_loss ? rho[1] : 1.0;   // the corrector: rows scaled by sqrt(rho')
    bool finite = isfinite(chi2) && isfinite(rho[0]) && isfinite(w);
    if (WITH_JAC) {
      const double g0 = w * q0, g1 = w * q1, g2 = w * q2;
      finite = finite && isfinite(g0) && isfinite(g1) && isfinite(g2);
      A.rec[k] = w * l00;
      A.rec[n + k] = w * l01;
      A.rec[2 * n + k] = w * l02;
      A.rec[3 * n + k] = w * l11;
      A.rec[4 * n + k] = w * l12;
      A.rec[5 * n + k] = w * l22;
      A.rec[6 * n + k] = g0;
      A.rec[7 * n + k] = g1;
      A.rec[8 * n + k] = g2;
    }
    if (!finite) atomicOr(bad, 1);
    if (A.d_out) {
      const int64_t c = A.order[k];
      A.d_out[3 * c] = d0;
      A.d_out[3 * c + 1] = d1;
      A.d_out[3 * c + 2] = d2;
      A.chi2_out[c] = chi2;
    }
  }
  // wave shuffle, then LDS, in a fixed order (block_sum_bcast): the partial depends on the priors and the grid only
  const double tot = block_sum_bcast(cost, red);
  if (threadIdx.x == 0) cost_part[blockIdx.x] = tot;
}

struct PriorAddArgs {
  const int32_t* row;     // [n] global rows, ascending and unique
  const double* rec;      // [PRIOR_REC][n] of k_prior_eval<true>
  const double* scale;    // [.. x 3] Jacobi column scales by global row (0 on a constant pose: it receives exactly nothing)
  double* hd;             // [6][n_loc]
  double* gs;             // [n_loc x 3]
  double* dense;          // [6][n_loc] the scaled blocks alone, for k_dlr_setup; nullptr = not kept
  int32_t n, n_loc, lo;
};

template <int PGO_UNIT_ = 0>   // (a template so that only the translation units that launch it carry it)
__global__ __launch_bounds__(WG) void k_prior_add(PriorAddArgs A) {
  const int64_t n = A.n, nl = A.n_loc;
  for (int64_t k = (int64_t)blockIdx.x * WG + threadIdx.x; k < n; k += (int64_t)gridDim.x * WG) {
    const int64_t g = A.row[k], r = g - A.lo;
    const double s0 = A.scale[3 * g], s1 = A.scale[3 * g + 1], s2 = A.scale[3 * g + 2];
    const double h00 = s0 * A.rec[k] * s0, h01 = s0 * A.rec[n + k] * s1, h02 = s0 * A.rec[2 * n + k] * s2;
    const double h11 = s1 * A.rec[3 * n + k] * s1, h12 = s1 * A.rec[4 * n + k] * s2, h22 = s2 * A.rec[5 * n + k] * s2;
    const double g0 = s0 * A.rec[6 * n + k], g1 = s1 * A.rec[7 * n + k], g2 = s2 * A.rec[8 * n + k];
    A.hd[r] += h00;
    A.hd[nl + r] += h01;
    A.hd[2 * nl + r] += h02;
    A.hd[3 * nl + r] += h11;
    A.hd[4 * nl + r] += h12;
    A.hd[5 * nl + r] += h22;
    A.gs[3 * r] += g0;
    A.gs[3 * r + 1] += g1;
    A.gs[3 * r + 2] += g2;
    if (A.dense) {
      A.dense[r] = h00;
      A.dense[nl + r] = h01;
      A.dense[2 * nl + r] = h02;
      A.dense[3 * nl + r] = h11;
      A.dense[4 * nl + r] = h12;
      A.dense[5 * nl + r] = h22;
    }
  }
}

}  // namespace dev
}  // namespace pgo
