#pragma once
// Loop support kernels (include/pgo.h, "loop support"; loop_support.h is the one statement).  Launched by solver_support.hip
// only.  Everything walks the CALLER's numbering through tables the host built once per handle (the chain and edge tables of
// pgo_coarsen) or once per selection (the sorted loops); no atomics, every composition and every total runs in a fixed tree:
// two calls are bitwise equal, the internal pose ordering plays no part, and neither does the grid.
//   k_support_segments  one wavefront per segment of SUPPORT_SEG poses: 4 consecutive chain motions per lane folded serially, a
//                       log-step scan over the lanes (the tree of k_chain_compose) -> C_i in T, the segment's end in Cend
//   k_support_keys      ONE workgroup: lane l folds its run of consecutive segment ends, the runs are scanned (wavefront tree,
//                       then the four wavefront totals in order), every lane writes the Tkey of its run
//   k_support_traj      one lane per pose: T_i = Tkey_k o C_i, in place
//   k_support_prepare   one lane per sorted loop: M_f^-1 of the table
//   k_loop_support      one lane per sorted loop (neighbouring lanes share their candidates): the loop's range of the table,
//                       |hi - hi_e| <= window, the cycle (four compositions), counts and (q_min, best) -> the slot's result
//   k_support_finish    one lane per edge of the caller's order: the record, the weight (apply), per-chunk totals
//   k_support_fold      ONE workgroup: the chunk totals in fixed order (counts as doubles: exact)
#include <hip/hip_runtime.h>

#include "coarsen.hip.h"
#include "loop_support.h"
#include "kernels.hip.h"

namespace pgo {
namespace dev {

constexpr int SUPPORT_SEG = 256;    // poses per segment of the trajectory scan: 64 lanes x SUPPORT_Q
constexpr int SUPPORT_Q = 4;
constexpr int SUPPORT_NPART = 4;    // partial arrays per chunk: selected | supported | pairs | max pairs

struct SupportTrajArgs {
  const double *mx, *my, *mt;   // the handle's measurements (local edge order)
  const int32_t* chain;         // [n - 1] (local edge << 1) | reversed
  int32_t n, n_seg;
  double* T;                    // [n x SUPPORT_POSE]
  double* Cend;                 // [n_seg x SUPPORT_POSE] (the last one is not written)
  double* Tkey;                 // [n_seg x SUPPORT_POSE]
};

template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_support_segments(SupportTrajArgs A) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = A.n;
  for (int64_t k = (int64_t)blockIdx.x * (WG / 64) + wave; k < A.n_seg; k += (int64_t)gridDim.x * (WG / 64)) {
    const int64_t base = k * SUPPORT_SEG;
    Se2 loc[SUPPORT_Q];
    Se2 acc = se2_identity();
#pragma unroll
    for (int q = 0; q < SUPPORT_Q; ++q) {
      const int64_t i = base + lane * SUPPORT_Q + q;
      if (i + 1 < n) {
        const int32_t ce = A.chain[i];
        const int32_t e = ce >> 1;
        acc = se2_compose(acc, coarsen_chain_motion(A.mx[e], A.my[e], A.mt[e], (ce & 1) != 0));
      }
      loc[q] = acc;
    }
    Se2 inc = acc;   // inclusive scan of the lane totals, fixed tree
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const Se2 up = se2_shfl_up(inc, off);
      if (lane >= off) inc = se2_compose(up, inc);
    }
    Se2 pre = se2_shfl_up(inc, 1);
    if (lane == 0) pre = se2_identity();
#pragma unroll
    for (int q = 0; q < SUPPORT_Q; ++q) {
      const int j = lane * SUPPORT_Q + q;
      const int64_t i = base + j;
      if (i + 1 < n) {
        const Se2 R = se2_compose(pre, loc[q]);
        if (j + 1 < SUPPORT_SEG) support_store(A.T + SUPPORT_POSE * (i + 1), R);
        else support_store(A.Cend + SUPPORT_POSE * k, R);
      }
    }
    if (lane == 0) support_store(A.T + SUPPORT_POSE * base, se2_identity());
  }
}

// Tkey_0 = identity, Tkey_{k+1} = Tkey_k o Cend_k.  (n_seg <= 2^31 / 256: a run is short)
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_support_keys(SupportTrajArgs A) {
  __shared__ double wtot[WG / 64][SUPPORT_POSE];
  __shared__ double incl[WG][SUPPORT_POSE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ns = A.n_seg, per = (ns + WG - 1) / WG;
  const int lo = min(ns, (int)threadIdx.x * per), hi = min(ns, lo + per);
  Se2 run = se2_identity();
  for (int k = lo; k < hi; ++k)
    if (k + 1 < ns) run = se2_compose(run, support_load(A.Cend + SUPPORT_POSE * (int64_t)k));
  Se2 inc = run;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const Se2 up = se2_shfl_up(inc, off);
    if (lane >= off) inc = se2_compose(up, inc);
  }
  if (lane == 63) support_store(wtot[wave], inc);
  __syncthreads();
  if (wave > 0) {
    Se2 before = support_load(wtot[0]);
    for (int w = 1; w < wave; ++w) before = se2_compose(before, support_load(wtot[w]));
    inc = se2_compose(before, inc);
  }
  support_store(incl[threadIdx.x], inc);
  __syncthreads();
  Se2 pre = threadIdx.x == 0 ? se2_identity() : support_load(incl[threadIdx.x - 1]);
  for (int k = lo; k < hi; ++k) {
    support_store(A.Tkey + SUPPORT_POSE * (int64_t)k, pre);
    if (k + 1 < ns) pre = se2_compose(pre, support_load(A.Cend + SUPPORT_POSE * (int64_t)k));
  }
}

template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_support_traj(SupportTrajArgs A) {
  for (int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * WG) {
    double* t = A.T + SUPPORT_POSE * i;
    support_store(t, se2_compose(support_load(A.Tkey + SUPPORT_POSE * (i / SUPPORT_SEG)), support_load(t)));
  }
}

struct SupportArgs {
  const double *mx, *my, *mt;   // the handle's measurements (local edge order)
  const int32_t* eloc;          // [n_edges] caller's edge -> local edge (-1: a chain edge, never selected)
  const int32_t *ea, *eb;       // [n_edges] caller's endpoints
  const double* T;              // [n x SUPPORT_POSE]
  // the table of the selection, sorted by (lo, edge)
  const int32_t *s_edge, *s_lo, *s_hi;   // [n_sel]
  const int32_t* first;         // [n + 1]
  const int32_t* slot_of;       // [n_edges] -1: not selected
  double* minv;                 // [n_sel x SUPPORT_POSE]
  int32_t n, n_edges, n_sel, n_chunks;
  int32_t window, min_support, apply, _pad;
  double txy2, tth2;
  // results per slot, then per edge
  int32_t* r_cnt;               // [n_sel x 3] n_pairs | n_consistent | best
  double* r_q;                  // [n_sel]
  pgo_loop_support_record* out;        // [n_edges]
  double* w;                    // the weight plane (apply), local edge order
  double* part;                 // [SUPPORT_NPART][n_chunks]
  pgo_loop_support_stats* stats;
};

// M_e of the caller's edge e, from the measurement the handle holds
__device__ __forceinline__ Se2 support_loop_motion(const double* mx, const double* my, const double* mt, const int32_t* eloc, const int32_t* ea,
                                                   const int32_t* eb, int32_t e) {
  const int64_t l = eloc[e];
  return support_canonical(ea[e], eb[e], mx[l], my[l], mt[l]);
}

template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_support_prepare(SupportArgs A) {
  for (int64_t r = (int64_t)blockIdx.x * WG + threadIdx.x; r < A.n_sel; r += (int64_t)gridDim.x * WG)
    support_store(A.minv + SUPPORT_POSE * r, se2_inverse(support_loop_motion(A.mx, A.my, A.mt, A.eloc, A.ea, A.eb, A.s_edge[r])));
}

template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_loop_support(SupportArgs A) {
  for (int64_t r = (int64_t)blockIdx.x * WG + threadIdx.x; r < A.n_sel; r += (int64_t)gridDim.x * WG) {
    const int32_t e = A.s_edge[r], lo = A.s_lo[r], hi = A.s_hi[r];
    const Se2 Me = support_loop_motion(A.mx, A.my, A.mt, A.eloc, A.ea, A.eb, e);
    int64_t r0, r1;
    support_range(A.first, A.n, lo, A.window, &r0, &r1);
    const SupportAcc R = support_scan(e, lo, hi, Me, r0, r1, A.s_edge, A.s_lo, A.s_hi, A.minv, A.T, A.window, A.txy2, A.tth2);
    A.r_cnt[3 * r] = R.n_pairs;
    A.r_cnt[3 * r + 1] = R.n_consistent;
    A.r_cnt[3 * r + 2] = R.best;
    A.r_q[r] = R.q_min;
  }
}

template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_support_finish(SupportArgs A) {
  __shared__ double red[8];
  for (int c = blockIdx.x; c < A.n_chunks; c += gridDim.x) {
    const int64_t e = (int64_t)c * WG + threadIdx.x;
    double nsel = 0.0, nsup = 0.0, npair = 0.0, mpair = 0.0;
    if (e < A.n_edges) {
      const int64_t r = A.slot_of[e];
      pgo_loop_support_record O;
      O.selected = 0;
      O.n_pairs = 0;
      O.n_consistent = 0;
      O.best = -1;
      O.q_min = -1.0;
      if (r >= 0) {
        O.selected = 1;
        O.n_pairs = A.r_cnt[3 * r];
        O.n_consistent = A.r_cnt[3 * r + 1];
        O.best = A.r_cnt[3 * r + 2];
        O.q_min = A.r_q[r];
        const bool ok = O.n_consistent >= A.min_support;
        if (A.apply) A.w[A.eloc[e]] = ok ? 1.0 : 0.0;
        nsel = 1.0;
        nsup = ok ? 1.0 : 0.0;
        npair = (double)O.n_pairs;
        mpair = npair;
      }
      A.out[e] = O;
    }
    const int64_t nc = A.n_chunks;
    // (counts are sums of small integers in doubles: exact)
    const double v0 = block_sum_bcast(nsel, red), v1 = block_sum_bcast(nsup, red), v2 = block_sum_bcast(npair, red), v3 = block_max_bcast(mpair, red);
    if (threadIdx.x == 0) {
      A.part[c] = v0;
      A.part[nc + c] = v1;
      A.part[2 * nc + c] = v2;
      A.part[3 * nc + c] = v3;
    }
  }
}

// ONE workgroup: slots l, l + 256, ... in order, then the lane tree
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_support_fold(SupportArgs A) {
  __shared__ double red[8];
  const int nc = A.n_chunks;
  double v[SUPPORT_NPART] = {0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < nc; i += WG) {
#pragma unroll
    for (int q = 0; q < 3; ++q) v[q] += A.part[(int64_t)q * nc + i];
    v[3] = fmax(v[3], A.part[(int64_t)3 * nc + i]);
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) v[q] = block_sum_bcast(v[q], red);
  v[3] = block_max_bcast(v[3], red);
  if (threadIdx.x == 0) {
    pgo_loop_support_stats S;
    S.n_pairs_total = (int64_t)v[2];
    S.n_selected = (int32_t)v[0];
    S.n_supported = (int32_t)v[1];
    S.max_pairs = (int32_t)v[3];
    S._pad = 0;
    *A.stats = S;
  }
}

}  // namespace dev
}  // namespace pgo
