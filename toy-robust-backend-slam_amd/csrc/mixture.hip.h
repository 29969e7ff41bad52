#pragma once
// The max-mixture selection on the device (include/pgo.h, "max-mixture edges").  Launched by solver_mixture.hip only.
//
// k_mix_select: one lane per MIXTURE edge, in the caller's mixture order, workgroups of 256 lanes walking chunks of 256 mixture
// edges (the local edge behind mixture edge j comes from a table resolved when the mixtures were set; a handle with
// pose_ordering 1 keeps its edges in another order).  An active edge gathers its endpoints and poses once, then walks its
// components in index order: three 16-byte loads per component, s_k from edge_plain<false> (edge_model.h) with K1's heading
// asin(sin delta), q_k = mix_q (mixture.h) under the loss of the edge's class, the running pick and the best component's record
// in eight registers -- no lane-indexed local array.  It writes the chosen index, q_best and the margin per mixture edge; with `apply` also the chosen
// mean into the measurement planes, w_k* into the weight plane and the index into the selection array.  An inactive edge, or one
// without a finite component, keeps its selection and its planes.  Chunk c leaves its partials -- changed, non-finite, inactive,
// sum c_k*, sum q_k*, and the edges per chosen index -- at slot c, whatever workgroup took it, and ONE workgroup (k_mix_fold)
// folds the slots in the fixed order of k_gnc_fold.  No atomics: two calls are bitwise equal, and neither the grid nor the
// internal orderings play a part.  Per mixture edge: 4 + 8 + 1 + 4 B tables, 8 B endpoints, 48 B poses, 48 B per component read;
// 20 B written, + 36 B with apply (mx, my, mt, w, the selection).
#include <hip/hip_runtime.h>

#include "edge_model.h"
#include "kernels.hip.h"
#include "mixture.h"

namespace pgo {
namespace dev {

constexpr int MIX_NPART = 5 + MIX_MAX_COMPONENTS;   // per chunk: changed | non-finite | inactive | sum c | sum q | count[8]

struct MixtureArgs {
  EdgeArgs E;               // the handle's edge arrays, current poses and loss classes (local edge order)
  double *mx, *my, *mt;     // the measurement planes again, writable (apply)
  double* w;                // [n_local] the weight plane (apply; nullptr without)
  const int32_t* loc;       // [n] mixture edge -> local edge
  const int32_t* ptr;       // [n + 1] its components
  const MixComp* comp;
  int32_t* sel;             // [n] the applied selection (-1: none yet); written with apply
  int32_t* chosen;          // [n] out
  double* q;                // [2 n] out: q_best, margin
  int32_t n, n_chunks;
  int32_t apply, _pad;
  double* part;             // [MIX_NPART][n_chunks]
  pgo_mix_stats* out;
};

template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_mix_select(MixtureArgs A) {
  __shared__ double red[8];
  for (int c = blockIdx.x; c < A.n_chunks; c += gridDim.x) {
    const int64_t j = (int64_t)c * WG + threadIdx.x;
    double nchg = 0.0, nbad = 0.0, noff = 0.0, csum = 0.0, qsum = 0.0;
    int kcount = -1;   // the index this lane counts under (-1: none)
    if (j < A.n) {
      const int64_t e = A.loc[j];
      const unsigned fl = A.E.flags[e];
      const int prev = A.sel[j];
      int kst = prev;
      double qb = __builtin_nan(""), qm = qb;
      if (fl & EDGE_INACTIVE) {
        noff = 1.0;
      } else {
        const int a = A.E.ia[e], b = A.E.ib[e];
        const double* pa = A.E.poses + 3 * (int64_t)a;
        const double* pb = A.E.poses + 3 * (int64_t)b;
        const double x1 = pa[0], y1 = pa[1], t1 = pa[2], x2 = pb[0], y2 = pb[1], t2 = pb[2];
        const LossClass L = pick_loss(A.E.loss0, A.E.loss1, A.E.loss2, A.E.loss3, (fl >> 2) & 3u);
        const int k0 = A.ptr[j], k1 = A.ptr[j + 1];
        MixPick P = mix_pick_begin();
        double bx = 0.0, by = 0.0, bt = 0.0, bw = 1.0, bc = 0.0;   // the best component's record, kept as the pick moves
        for (int k = k0; k < k1; ++k) {
          const double2* rec = reinterpret_cast<const double2*>(A.comp + k);
          const double2 r0 = rec[0], r1 = rec[1], r2 = rec[2];   // mx my | mt w | c pad
          double ex, ey, sind;
          edge_plain<false>(x1, y1, t1, x2, y2, t2, r0.x, r0.y, r1.x, ex, ey, sind, nullptr);   // (edge_model.h)
          const double et = asin(sind);
          const double s = ex * ex + ey * ey + et * et;
          const double q = mix_q(L, r1.y, r2.x, s);
          const int before = P.k;
          mix_pick_take(P, k - k0, q);
          if (P.k != before) {
            bx = r0.x; by = r0.y; bt = r1.x; bw = r1.y; bc = r2.x;
          }
        }
        if (P.k < 0) {
          nbad = 1.0;
        } else {
          kst = P.k;
          kcount = P.k;
          qb = mix_pick_best(P);
          qm = mix_pick_margin(P);
          csum = bc;
          qsum = qb;
          if (kst != prev) nchg = 1.0;
          if (A.apply) {
            A.mx[e] = bx;
            A.my[e] = by;
            A.mt[e] = bt;
            A.w[e] = bw;
            A.sel[j] = kst;
          }
        }
      }
      A.chosen[j] = kst;
      A.q[2 * j] = qb;
      A.q[2 * j + 1] = qm;
    }
    const int64_t nc = A.n_chunks;
    // (counts are sums of 0 / 1 in doubles: exact)
    const double v0 = block_sum_bcast(nchg, red), v1 = block_sum_bcast(nbad, red), v2 = block_sum_bcast(noff, red),
                 v3 = block_sum_bcast(csum, red), v4 = block_sum_bcast(qsum, red);
    if (threadIdx.x == 0) {
      A.part[c] = v0;
      A.part[nc + c] = v1;
      A.part[2 * nc + c] = v2;
      A.part[3 * nc + c] = v3;
      A.part[4 * nc + c] = v4;
    }
#pragma unroll
    for (int i = 0; i < MIX_MAX_COMPONENTS; ++i) {
      const double vi = block_sum_bcast(kcount == i ? 1.0 : 0.0, red);
      if (threadIdx.x == 0) A.part[(5 + i) * nc + c] = vi;
    }
  }
}

// ONE workgroup: slots l, l + 256, ... in order, then the lane tree
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_mix_fold(MixtureArgs A) {
  __shared__ double red[8];
  const int nc = A.n_chunks;
  double v[MIX_NPART];
#pragma unroll
  for (int i = 0; i < MIX_NPART; ++i) v[i] = 0.0;
  for (int s = threadIdx.x; s < nc; s += WG) {
#pragma unroll
    for (int i = 0; i < MIX_NPART; ++i) v[i] += A.part[(int64_t)i * nc + s];
  }
#pragma unroll
  for (int i = 0; i < MIX_NPART; ++i) v[i] = block_sum_bcast(v[i], red);
  if (threadIdx.x == 0) {
    pgo_mix_stats S;
    S.n_mix = A.n;
    S.n_changed = (int32_t)v[0];
    S.n_nonfinite = (int32_t)v[1];
    S.n_inactive = (int32_t)v[2];
    S.offset = v[3];
    S.mix_cost = v[4];
#pragma unroll
    for (int i = 0; i < MIX_MAX_COMPONENTS; ++i) S.count[i] = (int32_t)v[5 + i];
    *A.out = S;
  }
}

}  // namespace dev
}  // namespace pgo
