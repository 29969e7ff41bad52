#pragma once
// Coarsening and prolongation kernels (include/pgo.h, "hierarchical initialisation"; coarsen.h is the one statement of the
// operators).  Launched by solver_coarsen.hip only.  Everything walks the CALLER's numbering through tables the host built
// once per handle; no atomics, every composition runs in a fixed tree: two calls are bitwise equal, the internal pose ordering
// plays no part, and neither does the grid.
//   k_chain_compose<Q>   one wavefront per segment: Q consecutive chain motions per lane folded serially, a log-step scan over
//                        the lanes, then the lane's own prefixes -> C, Cend, the K - 1 composite edges and the key poses
//   k_coarsen_count      per chunk of COARSEN_CHUNK fine edges: how many are kept
//   k_coarsen_scan       ONE workgroup: exclusive scan of the chunk counts
//   k_coarsen_edges      one lane per fine edge: C_a o m o C_b^-1 of every kept edge to its slot (stable)
//   k_prolong            one lane per fine pose, written through perm into the pose buffer
//   k_chain_compose_info<Q>, k_coarsen_edges_info    the siblings of pgo_coarsen_info: pairs (motion, covariance), the same trees
#include <hip/hip_runtime.h>

#include "coarsen.h"
#include "kernels.hip.h"

namespace pgo {
namespace dev {

constexpr int COARSEN_CHUNK = WG;       // fine edges per chunk: one per lane
constexpr int COARSEN_MAX_Q = 4;        // chain motions per lane: stride <= 64 COARSEN_MAX_Q

struct CoarsenArgs {
  // the handle's edges (local order) and poses (internal numbering)
  const double *mx, *my, *mt;
  const double* poses;
  const int32_t* perm;        // caller's pose -> internal position; nullptr = the identity
  // tables in the caller's numbering
  const int32_t* chain;       // [n - 1] (local edge << 1) | reversed
  const int32_t* ea;          // [n_edges] caller's endpoints
  const int32_t* eb;
  const int32_t* eloc;        // [n_edges] local edge, -1 for a chain edge
  const uint8_t* ekind;       // [n_edges]
  int32_t n, n_edges, stride, n_key;
  int32_t n_chunks, _pad;
  // composites kept in the handle
  double* C;                  // [n x 3]
  double* Cend;               // [(n_key - 1) x 3]
  // scan scratch and outputs
  int32_t* cnt;               // [n_chunks] kept edges per chunk
  int32_t* off;               // [n_chunks] exclusive scan
  double* o_key;              // [n_key x 3] the current poses at the key poses
  double* o_meas;             // [n_out x 3]
  int32_t *o_ia, *o_ib, *o_origin;
  uint8_t* o_kind;
};

__device__ __forceinline__ Se2 se2_shfl_up(const Se2& A, int off) {
  Se2 R;
  R.x = __shfl_up(A.x, off, 64);
  R.y = __shfl_up(A.y, off, 64);
  R.th = __shfl_up(A.th, off, 64);
  R.c = __shfl_up(A.c, off, 64);
  R.s = __shfl_up(A.s, off, 64);
  return R;
}

// Segment k holds the motions Z_{kS + j}, j < S; the inclusive scan at j is C_{kS + j + 1}, or Cend_k at j = S - 1.
template <int Q>
__global__ __launch_bounds__(WG) void k_chain_compose(CoarsenArgs A) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t S = A.stride, n = A.n;
  for (int64_t k = (int64_t)blockIdx.x * (WG / 64) + wave; k < A.n_key; k += (int64_t)gridDim.x * (WG / 64)) {
    const int64_t base = k * S;
    Se2 loc[Q];
    Se2 acc = se2_identity();
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int64_t j = (int64_t)lane * Q + q, i = base + j;
      if (j < S && i + 1 < n) {
        const int32_t ce = A.chain[i];
        const int32_t e = ce >> 1;
        acc = se2_compose(acc, coarsen_chain_motion(A.mx[e], A.my[e], A.mt[e], (ce & 1) != 0));
      }
      loc[q] = acc;
    }
    // inclusive scan of the lane totals, fixed tree
    Se2 inc = acc;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const Se2 up = se2_shfl_up(inc, off);
      if (lane >= off) inc = se2_compose(up, inc);
    }
    Se2 pre = se2_shfl_up(inc, 1);
    if (lane == 0) pre = se2_identity();
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int64_t j = (int64_t)lane * Q + q, i = base + j;
      if (j < S && i + 1 < n) {
        const Se2 R = se2_compose(pre, loc[q]);
        if (j + 1 < S) {
          A.C[3 * (i + 1)] = R.x;
          A.C[3 * (i + 1) + 1] = R.y;
          A.C[3 * (i + 1) + 2] = R.th;
        } else {   // the segment's closing composite: kept, and the coarse odometry edge (k, k + 1)
          A.Cend[3 * k] = R.x;
          A.Cend[3 * k + 1] = R.y;
          A.Cend[3 * k + 2] = R.th;
          A.o_meas[3 * k] = R.x;
          A.o_meas[3 * k + 1] = R.y;
          A.o_meas[3 * k + 2] = coarsen_wrap(R.th);
          A.o_ia[k] = (int32_t)k;
          A.o_ib[k] = (int32_t)k + 1;
          A.o_origin[k] = -1;
          A.o_kind[k] = 0;
        }
      }
    }
    if (lane == 0) {
      A.C[3 * base] = 0.0;
      A.C[3 * base + 1] = 0.0;
      A.C[3 * base + 2] = 0.0;
      const double* p = A.poses + 3 * (int64_t)(A.perm ? A.perm[base] : (int32_t)base);
      A.o_key[3 * k] = p[0];
      A.o_key[3 * k + 1] = p[1];
      A.o_key[3 * k + 2] = p[2];
    }
  }
}

// (pointers BY VALUE: a reference into a kernel's argument block keeps a copy of it in scratch)
__device__ __forceinline__ bool coarsen_keeps(const int32_t* eloc, const int32_t* ea, const int32_t* eb, int64_t e, int32_t n_edges,
                                              int32_t stride) {
  return e < n_edges && eloc[e] >= 0 && ea[e] / stride != eb[e] / stride;
}

// the workgroup's count of `flag` (broadcast) and this lane's rank among the set lanes below it.  sh: >= WG / 64 + 1 ints
__device__ __forceinline__ int block_rank(bool flag, int* total, int* sh) {
  const unsigned long long m = __ballot(flag);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int below = __popcll(m & ((1ull << lane) - 1ull));
  __syncthreads();
  if (lane == 0) sh[w] = __popcll(m);
  __syncthreads();
  int base = 0, all = 0;
#pragma unroll
  for (int q = 0; q < WG / 64; ++q) {
    if (q < w) base += sh[q];
    all += sh[q];
  }
  *total = all;
  return base + below;
}

template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_coarsen_count(CoarsenArgs A) {
  __shared__ int sh[WG / 64 + 1];
  for (int c = blockIdx.x; c < A.n_chunks; c += gridDim.x) {
    const int64_t e = (int64_t)c * COARSEN_CHUNK + threadIdx.x;
    int total;
    (void)block_rank(coarsen_keeps(A.eloc, A.ea, A.eb, e, A.n_edges, A.stride), &total, sh);
    if (threadIdx.x == 0) A.cnt[c] = total;
  }
}

// ONE workgroup: lane l sums its run of ceil(n_chunks / WG) consecutive counts, the runs are scanned through LDS, and every
// lane writes its run's offsets (integers: exact in any order)
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_coarsen_scan(CoarsenArgs A) {
  __shared__ int run[WG];
  const int nc = A.n_chunks, per = (nc + WG - 1) / WG;
  const int lo = min(nc, (int)threadIdx.x * per), hi = min(nc, lo + per);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += A.cnt[i];
  run[threadIdx.x] = s;
  __syncthreads();
  int before = 0;
  for (int q = 0; q < (int)threadIdx.x; ++q) before += run[q];
  for (int i = lo; i < hi; ++i) {
    A.off[i] = before;
    before += A.cnt[i];
  }
}

template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_coarsen_edges(CoarsenArgs A) {
  __shared__ int sh[WG / 64 + 1];
  const int32_t S = A.stride;
  for (int c = blockIdx.x; c < A.n_chunks; c += gridDim.x) {
    const int64_t e = (int64_t)c * COARSEN_CHUNK + threadIdx.x;
    const bool keep = coarsen_keeps(A.eloc, A.ea, A.eb, e, A.n_edges, S);
    int total;
    const int rank = block_rank(keep, &total, sh);
    if (keep) {
      const int32_t a = A.ea[e], b = A.eb[e], l = A.eloc[e];
      const int64_t slot = (int64_t)(A.n_key - 1) + A.off[c] + rank;
      const Se2 Ca = se2_make(A.C[3 * (int64_t)a], A.C[3 * (int64_t)a + 1], A.C[3 * (int64_t)a + 2]);
      const Se2 Cb = se2_make(A.C[3 * (int64_t)b], A.C[3 * (int64_t)b + 1], A.C[3 * (int64_t)b + 2]);
      double m[3];
      coarsen_transport(Ca, A.mx[l], A.my[l], A.mt[l], Cb, m);
      A.o_meas[3 * slot] = m[0];
      A.o_meas[3 * slot + 1] = m[1];
      A.o_meas[3 * slot + 2] = m[2];
      A.o_ia[slot] = a / S;
      A.o_ib[slot] = b / S;
      A.o_origin[slot] = (int32_t)e;
      A.o_kind[slot] = A.ekind[e];
    }
  }
}

// ------------------------------------------------------------------ the same with information (pgo_coarsen_info)
// Siblings of k_chain_compose and k_coarsen_edges that carry pairs (motion, covariance; coarsen.h): the same trees, the same
// slots (k_coarsen_count / k_coarsen_scan as they stand).  The host has refused an information matrix that is not positive
// definite before they are launched.
struct CoarsenInfoArgs {
  CoarsenArgs a;
  const double* info;         // six planes over the local edges (plane c of local edge k at c n_local + k); nullptr = unit
  int64_t n_local;
  double* Ccov;               // [n x 6]
  double* Cendcov;            // [(n_key - 1) x 6]
  double* o_cov;              // [n_out x 6]
  double* o_info;             // [n_out x 6]
};

__device__ __forceinline__ Se2Cov pair_shfl_up(const Se2Cov& A, int off) {
  Se2Cov R;
  R.m = se2_shfl_up(A.m, off);
#pragma unroll
  for (int c = 0; c < 6; ++c) R.v[c] = __shfl_up(A.v[c], off, 64);
  return R;
}

// local edge l's information from the planes into w (zeros without planes: not read then)
__device__ __forceinline__ void info_planes_load(const double* info, int64_t n_local, int32_t l, double w[6]) {
#pragma unroll
  for (int c = 0; c < 6; ++c) w[c] = info ? info[c * n_local + l] : 0.0;
}

// Z_i as a pair (pointers BY VALUE, as coarsen_keeps)
__device__ __forceinline__ Se2Cov chain_pair_load(const int32_t* chain, const double* mx, const double* my, const double* mt,
                                                  const double* info, int64_t n_local, int64_t i) {
  const int32_t ce = chain[i];
  const int32_t e = ce >> 1;
  double w[6];
  Se2Cov Z;
  info_planes_load(info, n_local, e, w);
  if (!coarsen_chain_pair_w(mx[e], my[e], mt[e], info != nullptr, w, (ce & 1) != 0, &Z)) Z = pair_identity();
  return Z;
}

__device__ __forceinline__ void store6(double* dst, const double v[6]) {
#pragma unroll
  for (int c = 0; c < 6; ++c) dst[c] = v[c];
}

// k_chain_compose<Q> on pairs.  The lane's Q local prefixes are not kept across the scan: the write-out pass folds the lane's
// motions again (the same operations in the same order, so the same bits) -- Q pairs of 11 doubles do not fit the registers --,
// and neither fold is unrolled: the register count is that of Q = 1.
template <int Q>
__global__ __launch_bounds__(WG) void k_chain_compose_info(CoarsenInfoArgs AI) {
  const CoarsenArgs& A = AI.a;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t S = A.stride, n = A.n;
  for (int64_t k = (int64_t)blockIdx.x * (WG / 64) + wave; k < A.n_key; k += (int64_t)gridDim.x * (WG / 64)) {
    const int64_t base = k * S;
    Se2Cov acc = pair_identity();
#pragma unroll 1
    for (int q = 0; q < Q; ++q) {
      const int64_t j = (int64_t)lane * Q + q, i = base + j;
      if (j < S && i + 1 < n) acc = pair_compose(acc, chain_pair_load(A.chain, A.mx, A.my, A.mt, AI.info, AI.n_local, i));
    }
    // inclusive scan of the lane totals, fixed tree
    Se2Cov inc = acc;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const Se2Cov up = pair_shfl_up(inc, off);
      if (lane >= off) inc = pair_compose(up, inc);
    }
    Se2Cov pre = pair_shfl_up(inc, 1);
    if (lane == 0) pre = pair_identity();
    acc = pair_identity();
#pragma unroll 1
    for (int q = 0; q < Q; ++q) {
      const int64_t j = (int64_t)lane * Q + q, i = base + j;
      if (j < S && i + 1 < n) {
        acc = pair_compose(acc, chain_pair_load(A.chain, A.mx, A.my, A.mt, AI.info, AI.n_local, i));
        const Se2Cov R = pair_compose(pre, acc);
        if (j + 1 < S) {
          A.C[3 * (i + 1)] = R.m.x;
          A.C[3 * (i + 1) + 1] = R.m.y;
          A.C[3 * (i + 1) + 2] = R.m.th;
          store6(AI.Ccov + 6 * (i + 1), R.v);
        } else {   // the segment's closing composite: kept, and the coarse odometry edge (k, k + 1)
          A.Cend[3 * k] = R.m.x;
          A.Cend[3 * k + 1] = R.m.y;
          A.Cend[3 * k + 2] = R.m.th;
          store6(AI.Cendcov + 6 * k, R.v);
          A.o_meas[3 * k] = R.m.x;
          A.o_meas[3 * k + 1] = R.m.y;
          A.o_meas[3 * k + 2] = coarsen_wrap(R.m.th);
          double w[6];
          coarsen_info_of(R.v, w);
          store6(AI.o_cov + 6 * k, R.v);
          store6(AI.o_info + 6 * k, w);
          A.o_ia[k] = (int32_t)k;
          A.o_ib[k] = (int32_t)k + 1;
          A.o_origin[k] = -1;
          A.o_kind[k] = 0;
        }
      }
    }
    if (lane == 0) {
      A.C[3 * base] = 0.0;
      A.C[3 * base + 1] = 0.0;
      A.C[3 * base + 2] = 0.0;
      const Se2Cov I = pair_identity();
      store6(AI.Ccov + 6 * base, I.v);
      const double* p = A.poses + 3 * (int64_t)(A.perm ? A.perm[base] : (int32_t)base);
      A.o_key[3 * k] = p[0];
      A.o_key[3 * k + 1] = p[1];
      A.o_key[3 * k + 2] = p[2];
    }
  }
}

template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_coarsen_edges_info(CoarsenInfoArgs AI) {
  __shared__ int sh[WG / 64 + 1];
  const CoarsenArgs& A = AI.a;
  const int32_t S = A.stride;
  for (int c = blockIdx.x; c < A.n_chunks; c += gridDim.x) {
    const int64_t e = (int64_t)c * COARSEN_CHUNK + threadIdx.x;
    const bool keep = coarsen_keeps(A.eloc, A.ea, A.eb, e, A.n_edges, S);
    int total;
    const int rank = block_rank(keep, &total, sh);
    if (keep) {
      const int32_t a = A.ea[e], b = A.eb[e], l = A.eloc[e];
      const int64_t slot = (int64_t)(A.n_key - 1) + A.off[c] + rank;
      Se2Cov Ca, Cb;
      Ca.m = se2_make(A.C[3 * (int64_t)a], A.C[3 * (int64_t)a + 1], A.C[3 * (int64_t)a + 2]);
      Cb.m = se2_make(A.C[3 * (int64_t)b], A.C[3 * (int64_t)b + 1], A.C[3 * (int64_t)b + 2]);
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        Ca.v[q] = AI.Ccov[6 * (int64_t)a + q];
        Cb.v[q] = AI.Ccov[6 * (int64_t)b + q];
      }
      double w[6], m[3] = {0.0, 0.0, 0.0}, cov[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, inf[6];
      info_planes_load(AI.info, AI.n_local, l, w);
      (void)coarsen_transport_pair_w(Ca, A.mx[l], A.my[l], A.mt[l], AI.info != nullptr, w, Cb, m, cov);
      coarsen_info_of(cov, inf);
      A.o_meas[3 * slot] = m[0];
      A.o_meas[3 * slot + 1] = m[1];
      A.o_meas[3 * slot + 2] = m[2];
      store6(AI.o_cov + 6 * slot, cov);
      store6(AI.o_info + 6 * slot, inf);
      A.o_ia[slot] = a / S;
      A.o_ib[slot] = b / S;
      A.o_origin[slot] = (int32_t)e;
      A.o_kind[slot] = A.ekind[e];
    }
  }
}

struct ProlongArgs {
  const double* X;            // [n_key x 3] coarse poses
  const double* C;            // [n x 3]
  const double* Cend;         // [(n_key - 1) x 3]
  const int32_t* perm;        // caller's pose -> internal position; nullptr = the identity
  const uint8_t* constant;    // [n] internal numbering: the resolved constant poses of an active set, or nullptr
  double* poses;              // the handle's poses, internal numbering
  int32_t n, stride, n_key, fixed_internal;   // fixed_internal: opt.fixed_pose in the internal numbering, -1 = none
};

template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_prolong(ProlongArgs A) {
  for (int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * WG) {
    const int32_t row = A.perm ? A.perm[i] : (int32_t)i;
    if (row == A.fixed_internal || (A.constant && A.constant[row])) continue;
    const int64_t k = i / A.stride;
    const bool has_next = k < A.n_key - 1;
    double out[3];
    coarsen_prolong_pose(A.X + 3 * k, has_next ? A.X + 3 * (k + 1) : nullptr, A.C + 3 * i, has_next ? A.Cend + 3 * k : nullptr, has_next,
                         (int32_t)(i - k * A.stride), A.stride, out);
    A.poses[3 * (int64_t)row] = out[0];
    A.poses[3 * (int64_t)row + 1] = out[1];
    A.poses[3 * (int64_t)row + 2] = out[2];
  }
}

}  // namespace dev
}  // namespace pgo
