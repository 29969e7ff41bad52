#pragma once
// Scoring kernels (include/pgo.h, "scoring"): the trajectory error of the handle's poses against a reference, and the
// per-edge weights of the robust machinery.  Launched by solver_score.hip only.
//
// Trajectory error.  Workgroups of 256 lanes walk the CALLER's numbering in chunks of SCORE_CHUNK poses (the estimate is
// gathered through perm); chunk c leaves its partial sums at slot c of the partials arrays, whatever workgroup took it, and
// ONE workgroup folds the slots in fixed order (lane l adds slots l, l + 256, ..., then the lane tree of block_sum_bcast).
// The sums behind the alignment (centroids, centred moments) are compensated (TrajAcc) through the same tree.
// No atomics; the maxima carry their index and ties go to the smaller one.  Hence two calls are bitwise equal, the internal
// pose ordering plays no part, and neither does the grid.
//   k_traj_centroid -> k_traj_fold<0>   counted poses, sums of p and q          -> centroids
//   k_traj_moments  -> k_traj_fold<1>   centred moments a, b                    -> phi, t      (both passes: align = 1 only)
//   k_traj_errors   -> k_traj_fold<2>   ATE / RPE terms, the per-pose array     -> pgo_traj_error
#include <hip/hip_runtime.h>

#include "edge_model.h"
#include "kernels.hip.h"
#include "traj_error.h"

namespace pgo {
namespace dev {

constexpr int SCORE_CHUNK = PGO_SCORE_POSES_PER_WG;   // poses per chunk: SCORE_CHUNK / WG per lane
static_assert(SCORE_CHUNK % WG == 0, "a chunk is a whole number of poses per lane");
constexpr int SCORE_NSUM = 9;    // partial-sum arrays: the error pass fills 7 (n, t2, t1, r2, np, pt2, pr2: traj_error.h, TrajSums), the
                                 // centroid pass 9 (count, then s | c of four compensated sums), the moment pass 4 (s | c of a, b)
constexpr int SCORE_NERR = 7;
constexpr int SCORE_NMAX = 4;    // partial maxima: tmax, rmax, ptmax, prmax
constexpr int SCORE_NIDX = 3;    // partial indices: of tmax, of ptmax, the smallest counted pose that is not finite
constexpr int SCORE_STATE = 16;  // doubles: [0] count, [1..4] centroids pbar, qbar, [5..9] phi, c, s, tx, ty

struct TrajArgs {
  const double* est;       // the handle's poses, internal numbering
  const int32_t* perm;     // caller's pose -> internal position; nullptr = the identity
  const double* ref;       // [n x 3] caller's numbering
  const uint8_t* mask;     // [n] or nullptr
  int32_t n, n_chunks;
  int32_t delta;           // RPE pairs (i, i + delta); 0 = none
  int32_t _pad;
  double* psum;            // [SCORE_NSUM][n_chunks] partial sums
  double* pmax;            // [SCORE_NMAX][n_chunks]
  int32_t* pidx;           // [SCORE_NIDX][n_chunks]
  double* state;           // [SCORE_STATE]
  double* per_pose;        // [n x 2] or nullptr
  pgo_traj_error* out;     // followed by one int32: the smallest counted pose that is not finite, or -1
};

// maximum over the workgroup with its index (ties: the smaller index), broadcast.  sh: >= 5 doubles, shi: >= 5 ints
__device__ __forceinline__ void block_argmax_bcast(double& v, int32_t& i, double* sh, int32_t* shi) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double v2 = __shfl_down(v, off, 64);
    const int32_t i2 = __shfl_down(i, off, 64);
    traj_take_max(v, i, v2, i2);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) {
    sh[w] = v;
    shi[w] = i;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double bv = sh[0];
    int32_t bi = shi[0];
    for (int k = 1; k < WG / 64; ++k) traj_take_max(bv, bi, sh[k], shi[k]);
    sh[4] = bv;
    shi[4] = bi;
  }
  __syncthreads();
  v = sh[4];
  i = shi[4];
}
// a compensated sum (traj_error.h, TrajAcc) over the workgroup in the fixed tree of block_sum_bcast, broadcast.  sh: >= 10 doubles
__device__ __forceinline__ TrajAcc block_acc_bcast(TrajAcc A, double* sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double s2 = __shfl_down(A.s, off, 64), c2 = __shfl_down(A.c, off, 64);
    traj_acc_merge(A, s2, c2);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) {
    sh[2 * w] = A.s;
    sh[2 * w + 1] = A.c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    TrajAcc lo = {sh[0], sh[1]}, hi = {sh[4], sh[5]};
    traj_acc_merge(lo, sh[2], sh[3]);
    traj_acc_merge(hi, sh[6], sh[7]);
    traj_acc_merge(lo, hi.s, hi.c);
    sh[8] = lo.s;
    sh[9] = lo.c;
  }
  __syncthreads();
  return TrajAcc{sh[8], sh[9]};
}
// the smallest index >= 0 over the workgroup (-1: none), broadcast
__device__ __forceinline__ int32_t block_min_index_bcast(int32_t i, int32_t* shi) {
  unsigned u = (unsigned)i;   // -1 -> the largest unsigned value
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) u = min(u, (unsigned)__shfl_down((int)u, off, 64));
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) shi[w] = (int32_t)u;
  __syncthreads();
  if (threadIdx.x == 0) shi[4] = (int32_t)min(min((unsigned)shi[0], (unsigned)shi[1]), min((unsigned)shi[2], (unsigned)shi[3]));
  __syncthreads();
  return shi[4];
}

// (pointers BY VALUE: a reference into a kernel's argument block keeps a copy of it in scratch)
__device__ __forceinline__ bool traj_counted(const uint8_t* mask, int64_t i) { return !mask || mask[i]; }
__device__ __forceinline__ const double* traj_est(const double* est, const int32_t* perm, int64_t i) {
  return est + 3 * (int64_t)(perm ? perm[i] : (int32_t)i);
}

// pass 1: count and sums of the counted translations, per chunk
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_traj_centroid(TrajArgs A) {
  __shared__ double red[12];
  for (int c = blockIdx.x; c < A.n_chunks; c += gridDim.x) {
    double cnt = 0.0;
    TrajAcc spx = {0.0, 0.0}, spy = {0.0, 0.0}, sqx = {0.0, 0.0}, sqy = {0.0, 0.0};
    for (int k = 0; k < SCORE_CHUNK / WG; ++k) {
      const int64_t i = (int64_t)c * SCORE_CHUNK + k * WG + threadIdx.x;
      if (i < A.n && traj_counted(A.mask, i)) {
        const double* p = traj_est(A.est, A.perm, i);
        cnt += 1.0;
        traj_acc_add(spx, p[0]);
        traj_acc_add(spy, p[1]);
        traj_acc_add(sqx, A.ref[3 * i]);
        traj_acc_add(sqy, A.ref[3 * i + 1]);
      }
    }
    cnt = block_sum_bcast(cnt, red);   // (a count: exact)
    spx = block_acc_bcast(spx, red);
    spy = block_acc_bcast(spy, red);
    sqx = block_acc_bcast(sqx, red);
    sqy = block_acc_bcast(sqy, red);
    if (threadIdx.x == 0) {
      const int64_t nc = A.n_chunks;
      A.psum[c] = cnt;
      A.psum[nc + c] = spx.s;
      A.psum[2 * nc + c] = spx.c;
      A.psum[3 * nc + c] = spy.s;
      A.psum[4 * nc + c] = spy.c;
      A.psum[5 * nc + c] = sqx.s;
      A.psum[6 * nc + c] = sqx.c;
      A.psum[7 * nc + c] = sqy.s;
      A.psum[8 * nc + c] = sqy.c;
    }
  }
}

// pass 2: the centred moments about the centroids of pass 1, per chunk
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_traj_moments(TrajArgs A) {
  __shared__ double red[12];
  const double pbx = A.state[1], pby = A.state[2], qbx = A.state[3], qby = A.state[4];
  for (int c = blockIdx.x; c < A.n_chunks; c += gridDim.x) {
    TrajAcc a = {0.0, 0.0}, b = {0.0, 0.0};
    for (int k = 0; k < SCORE_CHUNK / WG; ++k) {
      const int64_t i = (int64_t)c * SCORE_CHUNK + k * WG + threadIdx.x;
      if (i < A.n && traj_counted(A.mask, i)) {
        const double* p = traj_est(A.est, A.perm, i);
        double ai, bi;
        traj_moment_terms(p[0], p[1], A.ref[3 * i], A.ref[3 * i + 1], pbx, pby, qbx, qby, ai, bi);
        traj_acc_add(a, ai);
        traj_acc_add(b, bi);
      }
    }
    a = block_acc_bcast(a, red);
    b = block_acc_bcast(b, red);
    if (threadIdx.x == 0) {
      const int64_t nc = A.n_chunks;
      A.psum[c] = a.s;
      A.psum[nc + c] = a.c;
      A.psum[2 * nc + c] = b.s;
      A.psum[3 * nc + c] = b.c;
    }
  }
}

// pass 3: the ATE terms of every counted pose and the RPE terms of every counted pair (i, i + delta), per chunk
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_traj_errors(TrajArgs A) {
  __shared__ double red[8];
  __shared__ int32_t redi[8];
  TrajAlign T;
  T.phi = A.state[5];
  T.c = A.state[6];
  T.s = A.state[7];
  T.tx = A.state[8];
  T.ty = A.state[9];
  for (int c = blockIdx.x; c < A.n_chunks; c += gridDim.x) {
    double s[SCORE_NERR];
#pragma unroll
    for (int q = 0; q < SCORE_NERR; ++q) s[q] = 0.0;
    double tmax = -1.0, rmax = -1.0, ptmax = -1.0, prmax = -1.0;
    int32_t tmax_i = -1, ptmax_i = -1, bad_i = -1;
    for (int k = 0; k < SCORE_CHUNK / WG; ++k) {
      const int64_t i = (int64_t)c * SCORE_CHUNK + k * WG + threadIdx.x;
      if (i >= A.n) continue;
      double t2 = 0.0, rot = 0.0;
      if (traj_counted(A.mask, i)) {
        const double* p = traj_est(A.est, A.perm, i);
        const double px = p[0], py = p[1], pt = p[2], qx = A.ref[3 * i], qy = A.ref[3 * i + 1], qt = A.ref[3 * i + 2];
        if (!(isfinite(px) && isfinite(py) && isfinite(pt) && isfinite(qx) && isfinite(qy) && isfinite(qt)) && bad_i < 0)
          bad_i = (int32_t)i;   // (i grows with k: the lane's smallest)
        traj_pose_error(T, px, py, pt, qx, qy, qt, t2, rot);
        s[0] += 1.0;
        s[1] += t2;
        s[2] += sqrt(t2);
        s[3] += rot * rot;
        traj_take_max(tmax, tmax_i, t2, (int32_t)i);
        rmax = fmax(rmax, rot);
        const int64_t j = i + (int64_t)A.delta;
        if (A.delta > 0 && j < A.n && traj_counted(A.mask, j)) {
          const double* pj = traj_est(A.est, A.perm, j);
          double p2, prot;
          traj_pair_error(px, py, pt, pj[0], pj[1], pj[2], qx, qy, qt, A.ref[3 * j], A.ref[3 * j + 1], A.ref[3 * j + 2], p2, prot);
          s[4] += 1.0;
          s[5] += p2;
          s[6] += prot * prot;
          traj_take_max(ptmax, ptmax_i, p2, (int32_t)i);
          prmax = fmax(prmax, prot);
        }
      }
      if (A.per_pose) {
        A.per_pose[2 * i] = sqrt(t2);
        A.per_pose[2 * i + 1] = rot;
      }
    }
    const int64_t nc = A.n_chunks;
#pragma unroll
    for (int q = 0; q < SCORE_NERR; ++q) {
      const double v = block_sum_bcast(s[q], red);
      if (threadIdx.x == 0) A.psum[q * nc + c] = v;
    }
    block_argmax_bcast(tmax, tmax_i, red, redi);
    block_argmax_bcast(ptmax, ptmax_i, red, redi);
    rmax = block_max_bcast(rmax, red);
    prmax = block_max_bcast(prmax, red);
    bad_i = block_min_index_bcast(bad_i, redi);
    if (threadIdx.x == 0) {
      A.pmax[c] = tmax;
      A.pmax[nc + c] = rmax;
      A.pmax[2 * nc + c] = ptmax;
      A.pmax[3 * nc + c] = prmax;
      A.pidx[c] = tmax_i;
      A.pidx[nc + c] = ptmax_i;
      A.pidx[2 * nc + c] = bad_i;
    }
  }
}

// slots l, l + 256, ... in order, then the lane tree
__device__ __forceinline__ double fold_sum(const double* part, int n, double* sh) {
  double v = 0.0;
  for (int i = threadIdx.x; i < n; i += WG) v += part[i];
  return block_sum_bcast(v, sh);
}
__device__ __forceinline__ double fold_acc(const double* ps, const double* pc, int n, double* sh) {
  TrajAcc A = {0.0, 0.0};
  for (int i = threadIdx.x; i < n; i += WG) traj_acc_merge(A, ps[i], pc[i]);
  return traj_acc_value(block_acc_bcast(A, sh));
}
__device__ __forceinline__ double fold_max(const double* part, int n, double* sh) {
  double v = -1.0;
  for (int i = threadIdx.x; i < n; i += WG) v = fmax(v, part[i]);
  return block_max_bcast(v, sh);
}
__device__ __forceinline__ void fold_argmax(const double* part, const int32_t* idx, int n, double& v, int32_t& vi, double* sh, int32_t* shi) {
  v = -1.0;
  vi = -1;
  for (int i = threadIdx.x; i < n; i += WG) traj_take_max(v, vi, part[i], idx[i]);
  block_argmax_bcast(v, vi, sh, shi);
}

// ONE workgroup.  STAGE 0: centroids from the partials of k_traj_centroid; 1: phi and t from those of k_traj_moments;
// 2: the result record from those of k_traj_errors.
template <int STAGE>
__global__ __launch_bounds__(WG) void k_traj_fold(TrajArgs A) {
  __shared__ double red[12];
  __shared__ int32_t redi[8];
  const int nc = A.n_chunks;
  const int64_t ncl = nc;
  if (STAGE == 0) {
    const double cnt = fold_sum(A.psum, nc, red), spx = fold_acc(A.psum + ncl, A.psum + 2 * ncl, nc, red),
                 spy = fold_acc(A.psum + 3 * ncl, A.psum + 4 * ncl, nc, red), sqx = fold_acc(A.psum + 5 * ncl, A.psum + 6 * ncl, nc, red),
                 sqy = fold_acc(A.psum + 7 * ncl, A.psum + 8 * ncl, nc, red);
    if (threadIdx.x == 0) {
      const bool any = cnt > 0.0;
      A.state[0] = cnt;
      A.state[1] = any ? spx / cnt : 0.0;
      A.state[2] = any ? spy / cnt : 0.0;
      A.state[3] = any ? sqx / cnt : 0.0;
      A.state[4] = any ? sqy / cnt : 0.0;
    }
  } else if (STAGE == 1) {
    const double a = fold_acc(A.psum, A.psum + ncl, nc, red), b = fold_acc(A.psum + 2 * ncl, A.psum + 3 * ncl, nc, red);
    if (threadIdx.x == 0) {
      TrajAlign T = traj_identity();
      if (A.state[0] > 0.0) T = traj_align_from_moments(a, b, A.state[1], A.state[2], A.state[3], A.state[4]);
      A.state[5] = T.phi;
      A.state[6] = T.c;
      A.state[7] = T.s;
      A.state[8] = T.tx;
      A.state[9] = T.ty;
    }
  } else {
    TrajSums S;
    S.n = fold_sum(A.psum, nc, red);
    S.t2 = fold_sum(A.psum + ncl, nc, red);
    S.t1 = fold_sum(A.psum + 2 * ncl, nc, red);
    S.r2 = fold_sum(A.psum + 3 * ncl, nc, red);
    S.np = fold_sum(A.psum + 4 * ncl, nc, red);
    S.pt2 = fold_sum(A.psum + 5 * ncl, nc, red);
    S.pr2 = fold_sum(A.psum + 6 * ncl, nc, red);
    fold_argmax(A.pmax, A.pidx, nc, S.tmax, S.tmax_i, red, redi);
    S.rmax = fold_max(A.pmax + ncl, nc, red);
    fold_argmax(A.pmax + 2 * ncl, A.pidx + ncl, nc, S.ptmax, S.ptmax_i, red, redi);
    S.prmax = fold_max(A.pmax + 3 * ncl, nc, red);
    int32_t bad = -1;
    for (int i = threadIdx.x; i < nc; i += WG) bad = (int32_t)min((unsigned)bad, (unsigned)A.pidx[2 * ncl + i]);
    bad = block_min_index_bcast(bad, redi);
    if (threadIdx.x == 0) {
      TrajAlign T;
      T.phi = A.state[5];
      T.c = A.state[6];
      T.s = A.state[7];
      T.tx = A.state[8];
      T.ty = A.state[9];
      traj_finish(S, T, A.out);
      *reinterpret_cast<int32_t*>(A.out + 1) = bad;
    }
  }
}

// ------------------------------------------------------------------ per-edge weights
// One lane per edge: the plain residual (edge_plain<false>, K1's heading asin(sin delta)), the DCS factor psi of edge_dcs on
// the edges METHOD 1 applies it to (flags bit 0), the loss of the edge's class at the scaled residual (loss.h) -- the
// arithmetic of K1's plain path, without its Jacobian.  Inactive edges are computed too.  57 B read + 48 B written per edge.
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_edge_weights(EdgeArgs A, int32_t dcs, const int32_t* __restrict__ orig_edge,
                                                    pgo_edge_weight* __restrict__ out) {
  const int64_t ne = A.n_edges;
  for (int64_t e = (int64_t)blockIdx.x * WG + threadIdx.x; e < ne; e += (int64_t)gridDim.x * WG) {
    const int a = A.ia[e], b = A.ib[e];
    const double dx = A.mx[e], dy = A.my[e], dth = A.mt[e];
    const unsigned fl = A.flags[e];
    const double x1 = A.poses[3 * (int64_t)a], y1 = A.poses[3 * (int64_t)a + 1], t1 = A.poses[3 * (int64_t)a + 2];
    const double x2 = A.poses[3 * (int64_t)b], y2 = A.poses[3 * (int64_t)b + 1], t2 = A.poses[3 * (int64_t)b + 2];
    double ex, ey, sind;
    edge_plain<false>(x1, y1, t1, x2, y2, t2, dx, dy, dth, ex, ey, sind, nullptr);   // (edge_model.h)
    double et = asin(sind);
    pgo_edge_weight W;
    W.s_plain = ex * ex + ey * ey + et * et;
    W.scale = 1.0;
    if (dcs && (fl & 1u)) {   // psi of edge_dcs
      const double res = ex * ex + ey * ey;
      const double psi = sqrt(2.0 * A.phi / (A.phi + res));
      if (psi < 1.0) {
        W.scale = psi;
        ex *= psi;
        ey *= psi;
        et *= psi;
      }
    }
    const double s = ex * ex + ey * ey + et * et;   // = scale^2 s_plain, in K1's arithmetic
    double rho[3];
    loss_rho(pick_loss(A.loss0, A.loss1, A.loss2, A.loss3, (fl >> 2) & 3u), s, rho);
    W.rho1 = rho[1];
    W.weight = W.scale * W.scale * rho[1];
    W.cost = 0.5 * rho[0];
    if (A.w) {   // pgo_set_edge_weights: the edge counts w times that (weight * s_plain stays |r|^2 of pgo_eval's r)
      const double w = A.w[e];
      W.weight *= w;
      W.cost *= w;
    }
    if (!isfinite(s)) W.s_plain = W.scale = W.rho1 = W.weight = W.cost = __builtin_nan("");
    W.active = (fl & EDGE_INACTIVE) ? 0 : 1;
    W._pad = 0;
    out[orig_edge[e]] = W;
  }
}

}  // namespace dev
}  // namespace pgo
