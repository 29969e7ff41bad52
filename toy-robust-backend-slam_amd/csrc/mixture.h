#pragma once
// Max-mixture edges (Olson & Agarwal, "Inference on networks of mixtures for robust robot mapping", RSS 2012 / IJRR 2013): ONE
// statement of a component's negative log-likelihood and of the selection among an edge's components, in plain doubles --
// evaluated by k_mix_select on the device (mixture.hip.h), by pgo_mixture_eval / pgo_mixture_plan and pgo_set_mixtures on the
// host (solver_mixture.hip), and by the stand-alone program tests/native/mixture_main.cpp.
//   component k of an edge: a mean m_k, a mixing weight pi_k > 0 (relative), an information scale w_k in (0, 1] -- in the
//   handle's unit-information objective its information is w_k I, so its normaliser is pi_k w_k^(3/2) and
//     c_k = -log(pi_k) - 1.5 log(w_k)                                  (mix_const; once, on the host)
//     q_k(x) = w_k 1/2 rho(s_k(x)) + c_k                               (mix_q)
//   with s_k the plain |e|^2 of edge_plain<false> (edge_model.h) for the measurement m_k, heading asin(sin delta), and rho the
//   loss of the edge's class.  A component whose s_k is not finite cannot be evaluated: its q_k is NaN whatever the loss (Tukey
//   is bounded and would otherwise hide it).
//   selection: k* = argmin q_k over the finite q_k, ties to the lowest index (MixPick); none finite: k = -1.
#include <hip/hip_runtime.h>

#include <cmath>

#include "loss.h"

namespace pgo {

constexpr int MIX_MAX_COMPONENTS = 8;   // PGO_MIX_MAX_COMPONENTS

// one component as k_mix_select reads it: three 16-byte loads
struct alignas(16) MixComp {
  double mx, my, mt;   // the mean
  double w;            // the information scale, in (0, 1]
  double c;            // mix_const(pi, w)
  double _pad;
};

__host__ __device__ inline bool mix_finite(double v) { return v - v == 0.0; }   // (no isfinite: one spelling for host and device)

inline double mix_const(double pi, double w) { return -std::log(pi) - 1.5 * std::log(w); }

__host__ __device__ inline double mix_q(const LossClass& L, double w, double c, double s) {
  if (!mix_finite(s)) return s - s;   // NaN
  double rho[3];
  loss_rho(L, s, rho);
  return w * (0.5 * rho[0]) + c;
}

// the running selection over an edge's components, taken in index order
struct MixPick {
  int k;                    // the best component so far; -1: none finite yet
  double q_best, q_second;  // +inf until a first / a second finite q
};

__host__ __device__ inline MixPick mix_pick_begin() {
  MixPick P;
  P.k = -1;
  P.q_best = P.q_second = HUGE_VAL;
  return P;
}

// strict comparisons: an equal q leaves the lower index in place
__host__ __device__ inline void mix_pick_take(MixPick& P, int k, double q) {
  if (!mix_finite(q)) return;
  if (P.k < 0 || q < P.q_best) {
    P.q_second = P.q_best;
    P.q_best = q;
    P.k = k;
  } else if (q < P.q_second) {
    P.q_second = q;
  }
}

// what a select reports per edge: q_best and the margin to the runner-up (+inf with one finite component; an edge that was not
// evaluated -- inactive, or without a finite component -- reports NaN for both)
__host__ __device__ inline double mix_pick_margin(const MixPick& P) { return P.k < 0 ? P.q_best - P.q_best : P.q_second - P.q_best; }
__host__ __device__ inline double mix_pick_best(const MixPick& P) { return P.k < 0 ? P.q_best - P.q_best : P.q_best; }

}  // namespace pgo
