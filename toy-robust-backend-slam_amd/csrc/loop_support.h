#pragma once
// Loop edges judged by odometry cycle consistency (include/pgo.h, "loop support"): ONE statement of the
// trajectory, of the cycle error of a pair of loops and of the per-edge record, evaluated on the host by pgo_loop_support_plan
// (serially, in the caller's order), on the device by the kernels of loop_support.hip.h (fixed trees), and by
// tests/native/loop_support_main.cpp.  Plain doubles only; the SE(2) operations are those of coarsen.h.
//   Z_i        the chain edge of the pair (i, i + 1) as a motion from i to i + 1            (coarsen_chain_motion)
//   T_0        = (0, 0, 0),  T_{i+1} = T_i o Z_i            angles plain sums; the rotation is carried as (cos, sin)
//   O(p, q)    = T_p^-1 o T_q
//   loop e = (a, b, m):  lo = min(a, b), hi = max(a, b), M_e = m if a < b else m^-1
//   Err(e, f)  = M_e o O(hi_e, hi_f) o M_f^-1 o O(lo_f, lo_e)
//              = (((H_e o T_hi_f) o M_f^-1) o T_lo_f^-1) o T_lo_e,   H_e = M_e o T_hi_e^-1     <- the association evaluated
//   q(e, f)    = max((Err.x^2 + Err.y^2) / (tol_xy^2 (2 + L)), wrap(Err.th)^2 / (tol_th^2 (2 + L))),  L = |lo_e - lo_f| + |hi_e - hi_f|
// A pose is stored as 5 doubles (x, y, theta, cos, sin): a lookup costs no sincos.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <vector>

#include "coarsen.h"

namespace pgo {

constexpr int SUPPORT_POSE = 5;   // doubles per stored SE(2) element

__host__ __device__ __forceinline__ Se2 support_load(const double* p) { return Se2{p[0], p[1], p[2], p[3], p[4]}; }
__host__ __device__ __forceinline__ void support_store(double* p, const Se2& A) {
  p[0] = A.x;
  p[1] = A.y;
  p[2] = A.th;
  p[3] = A.c;
  p[4] = A.s;
}

// M_e of the loop (a, b, m)
__host__ __device__ __forceinline__ Se2 support_canonical(int32_t a, int32_t b, double mx, double my, double mt) {
  return coarsen_chain_motion(mx, my, mt, !(a < b));
}
// H_e = M_e o T_hi_e^-1: what a loop brings to every pair it is the first member of
__host__ __device__ __forceinline__ Se2 support_head(const Se2& Me, const Se2& Thi) { return se2_compose(Me, se2_inverse(Thi)); }
// Err(e, f), four compositions left to right
__host__ __device__ __forceinline__ Se2 support_cycle(const Se2& He, const Se2& Thi_f, const Se2& Minv_f, const Se2& Tlo_f, const Se2& Tlo_e) {
  return se2_compose(se2_compose(se2_compose(se2_compose(He, Thi_f), Minv_f), se2_inverse(Tlo_f)), Tlo_e);
}
// q(e, f); txy2 = tol_xy^2, tth2 = tol_th^2.  A part that is not finite makes q not finite.
__host__ __device__ __forceinline__ double support_q(const Se2& Err, int32_t L, double txy2, double tth2) {
  const double w = coarsen_wrap(Err.th), n = 2.0 + (double)L;
  const double qa = (Err.x * Err.x + Err.y * Err.y) / (txy2 * n), qb = (w * w) / (tth2 * n);
  if (!(std::isfinite(qa) && std::isfinite(qb))) return qa + qb;   // (inf or NaN)
  return qa >= qb ? qa : qb;
}

// what a loop gathers over its neighbours: integer counts and a minimum with an index tie-break -- any scan order gives the same
struct SupportAcc {
  int32_t n_pairs, n_consistent, best;
  double q_min;
};
__host__ __device__ __forceinline__ SupportAcc support_acc_begin() { return SupportAcc{0, 0, -1, -1.0}; }
__host__ __device__ __forceinline__ void support_accumulate(SupportAcc& R, double q, int32_t f) {
  ++R.n_pairs;
  if (!std::isfinite(q)) return;
  if (q <= 1.0) ++R.n_consistent;
  if (R.best < 0 || q < R.q_min || (q == R.q_min && f < R.best)) {
    R.q_min = q;
    R.best = f;
  }
}
__host__ __device__ __forceinline__ int32_t support_absdiff(int32_t a, int32_t b) { return a > b ? a - b : b - a; }

// One loop e against the candidates [r0, r1) of the table sorted by (lo, edge): s_edge / s_lo / s_hi per slot, minv the M_f^-1
// (SUPPORT_POSE doubles per slot), T the trajectory (SUPPORT_POSE doubles per pose).
__host__ __device__ __forceinline__ SupportAcc support_scan(int32_t e, int32_t lo_e, int32_t hi_e, const Se2& Me, int64_t r0, int64_t r1,
                                                            const int32_t* s_edge, const int32_t* s_lo, const int32_t* s_hi, const double* minv,
                                                            const double* T, int32_t window, double txy2, double tth2) {
  const Se2 He = support_head(Me, support_load(T + (int64_t)SUPPORT_POSE * hi_e));
  const Se2 Tlo_e = support_load(T + (int64_t)SUPPORT_POSE * lo_e);
  SupportAcc R = support_acc_begin();
  for (int64_t r = r0; r < r1; ++r) {
    const int32_t f = s_edge[r], hi_f = s_hi[r];
    const int32_t dh = support_absdiff(hi_e, hi_f);
    if (f == e || dh > window) continue;
    const int32_t lo_f = s_lo[r];
    const Se2 Err = support_cycle(He, support_load(T + (int64_t)SUPPORT_POSE * hi_f), support_load(minv + SUPPORT_POSE * r),
                                  support_load(T + (int64_t)SUPPORT_POSE * lo_f), Tlo_e);
    support_accumulate(R, support_q(Err, support_absdiff(lo_e, lo_f) + dh, txy2, tth2), f);
  }
  return R;
}

// ------------------------------------------------------------------ the serial evaluation and the tables (host)
// chain[i] (i < N - 1): the edge joining poses i and i + 1.  T: N x SUPPORT_POSE, folded left to right.
inline void support_trajectory_serial(int64_t N, const int32_t* chain, const int32_t* ia, const double* meas, double* T) {
  Se2 A = se2_identity();
  for (int64_t i = 0; i < N; ++i) {
    support_store(T + SUPPORT_POSE * i, A);
    if (i + 1 < N) {
      const int64_t e = chain[i];
      A = se2_compose(A, coarsen_chain_motion(meas[3 * e], meas[3 * e + 1], meas[3 * e + 2], ia[e] != (int32_t)i));
    }
  }
}

// The selected loops sorted by (lo, edge index) -- a counting sort over lo, stable in the edge index -- and first[p] (N + 1
// entries): the slots [first[p], first[p + 1]) hold the loops with lo = p, so that the loops with lo in [p, q] are the slots
// [first[p], first[q + 1]).  slot_of (E entries, optional): the slot of a selected edge, -1 for every other edge.
inline void support_sort(int64_t N, int64_t E, const int32_t* ia, const int32_t* ib, const uint8_t* selected, std::vector<int32_t>* s_edge,
                         std::vector<int32_t>* s_lo, std::vector<int32_t>* s_hi, std::vector<int32_t>* first, std::vector<int32_t>* slot_of) {
  first->assign((size_t)(N + 1), 0);
  for (int64_t e = 0; e < E; ++e)
    if (selected[e]) ++(*first)[(size_t)(ia[e] < ib[e] ? ia[e] : ib[e]) + 1];
  for (int64_t p = 0; p < N; ++p) (*first)[p + 1] += (*first)[p];
  const int64_t n = (*first)[N];
  s_edge->assign((size_t)n, 0);
  s_lo->assign((size_t)n, 0);
  s_hi->assign((size_t)n, 0);
  if (slot_of) slot_of->assign((size_t)E, -1);
  std::vector<int32_t> next(first->begin(), first->end() - 1);
  for (int64_t e = 0; e < E; ++e) {
    if (!selected[e]) continue;
    const int32_t lo = ia[e] < ib[e] ? ia[e] : ib[e], hi = ia[e] < ib[e] ? ib[e] : ia[e];
    const int32_t r = next[lo]++;
    (*s_edge)[r] = (int32_t)e;
    (*s_lo)[r] = lo;
    (*s_hi)[r] = hi;
    if (slot_of) (*slot_of)[e] = r;
  }
}
// the candidate slots of a loop with that lo
__host__ __device__ __forceinline__ void support_range(const int32_t* first, int32_t n_poses, int32_t lo, int32_t window, int64_t* r0, int64_t* r1) {
  const int32_t p = lo - window > 0 ? lo - window : 0, q = lo + window < n_poses - 1 ? lo + window : n_poses - 1;
  *r0 = first[p];
  *r1 = first[q + 1];
}

}  // namespace pgo
