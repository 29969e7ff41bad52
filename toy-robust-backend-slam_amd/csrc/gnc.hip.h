#pragma once
// The GNC-TLS weight update on the device (include/pgo.h, "graduated non-convexity").  Launched by solver_gnc.hip only.
//
// k_gnc_update: one lane per edge of the CALLER's numbering, workgroups of 256 lanes walking chunks of 256 edges (the local
// edge behind caller's edge j comes from a table; a handle with pose_ordering 1 keeps its edges in another order).  A selected
// edge gets its plain |e|^2 from edge_plain<false> (edge_model.h) with K1's heading asin(sin delta) -- the s_plain of
// k_edge_weights, before DCS and any loss -- and the weight gnc_tls_weight(c2, mu, s) (gnc.h) in the handle's plane; every other
// edge keeps its weight.  Chunk c leaves its partials -- max s, sum w s, the counts of selected, 0 < w < 1, w = 0 and non-finite
// s -- at slot c, whatever workgroup took it, and ONE workgroup (k_gnc_fold) folds the slots in fixed order: lane l takes slots
// l, l + 256, ..., then the lane tree of block_sum_bcast.  No atomics: two calls are bitwise equal, and neither the grid nor the
// internal pose ordering plays a part.  61 B read (+ 8 B written) per selected edge, 1 B per other edge.
#include <hip/hip_runtime.h>

#include "edge_model.h"
#include "gnc.h"
#include "kernels.hip.h"

namespace pgo {
namespace dev {

constexpr int GNC_NPART = 6;   // partial arrays per chunk: max s | sum w s | selected | 0 < w < 1 | w = 0 | non-finite s

struct GncArgs {
  EdgeArgs E;               // the handle's edge arrays and current poses (local edge order)
  const int32_t* loc;       // [n] caller's edge -> local edge
  const uint8_t* select;    // [n] caller's order: 1 = the edge takes part (resolved on the host: selected AND active)
  double* w;                // [n_local] the plane (nullptr: no plane yet and nothing to write -- every weight reads as 1)
  int32_t n, n_chunks;
  int32_t mode;             // 0: measure only (weights untouched);  1: w <- gnc_tls_weight;  2: w <- 1 on the selected edges
  int32_t _pad;
  double c2, mu;
  double* part;             // [GNC_NPART][n_chunks]
  pgo_gnc_stats* out;
};

template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_gnc_update(GncArgs A) {
  __shared__ double red[8];
  for (int c = blockIdx.x; c < A.n_chunks; c += gridDim.x) {
    const int64_t j = (int64_t)c * WG + threadIdx.x;
    double smax = -1.0, wsum = 0.0, nsel = 0.0, nmid = 0.0, nzero = 0.0, nbad = 0.0;
    if (j < A.n && A.select[j]) {
      const int64_t e = A.loc[j];
      const int a = A.E.ia[e], b = A.E.ib[e];
      const double dx = A.E.mx[e], dy = A.E.my[e], dth = A.E.mt[e];
      const double* pa = A.E.poses + 3 * (int64_t)a;
      const double* pb = A.E.poses + 3 * (int64_t)b;
      double ex, ey, sind;
      edge_plain<false>(pa[0], pa[1], pa[2], pb[0], pb[1], pb[2], dx, dy, dth, ex, ey, sind, nullptr);   // (edge_model.h)
      const double et = asin(sind);
      const double s = ex * ex + ey * ey + et * et;
      double w = A.w ? A.w[e] : 1.0;
      if (A.mode == 1) w = gnc_tls_weight(A.c2, A.mu, s);
      else if (A.mode == 2) w = 1.0;
      if (A.mode != 0) A.w[e] = w;
      const bool fin = isfinite(s);
      nsel = 1.0;
      if (fin) {
        smax = s;
        wsum = w * s;
      } else {
        nbad = 1.0;
      }
      if (w > 0.0 && w < 1.0) nmid = 1.0;
      if (w == 0.0) nzero = 1.0;
    }
    const int64_t nc = A.n_chunks;
    // (counts are sums of 0 / 1 in doubles: exact)
    const double v0 = block_max_bcast(smax, red), v1 = block_sum_bcast(wsum, red), v2 = block_sum_bcast(nsel, red),
                 v3 = block_sum_bcast(nmid, red), v4 = block_sum_bcast(nzero, red), v5 = block_sum_bcast(nbad, red);
    if (threadIdx.x == 0) {
      A.part[c] = v0;
      A.part[nc + c] = v1;
      A.part[2 * nc + c] = v2;
      A.part[3 * nc + c] = v3;
      A.part[4 * nc + c] = v4;
      A.part[5 * nc + c] = v5;
    }
  }
}

// ONE workgroup: slots l, l + 256, ... in order, then the lane tree
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_gnc_fold(GncArgs A) {
  __shared__ double red[8];
  const int nc = A.n_chunks;
  double v[GNC_NPART];
  v[0] = -1.0;
#pragma unroll
  for (int q = 1; q < GNC_NPART; ++q) v[q] = 0.0;
  for (int i = threadIdx.x; i < nc; i += WG) {
    v[0] = fmax(v[0], A.part[i]);
#pragma unroll
    for (int q = 1; q < GNC_NPART; ++q) v[q] += A.part[(int64_t)q * nc + i];
  }
  v[0] = block_max_bcast(v[0], red);
#pragma unroll
  for (int q = 1; q < GNC_NPART; ++q) v[q] = block_sum_bcast(v[q], red);
  if (threadIdx.x == 0) {
    pgo_gnc_stats S;
    S.s_max = v[0];
    S.weighted_sum = v[1];
    S.n_selected = (int32_t)v[2];
    S.n_nonbinary = (int32_t)v[3];
    S.n_zero = (int32_t)v[4];
    S.n_nonfinite = (int32_t)v[5];
    *A.out = S;
  }
}

}  // namespace dev
}  // namespace pgo
