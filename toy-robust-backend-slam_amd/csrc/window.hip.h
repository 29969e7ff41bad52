// One workgroup solves one WINDOW: the whole Ceres LM loop of a tiny sub-problem of the handle's graph in a single launch.
//
// Why: the reference's layer managers solve a local window after every accepted loop edge (SimpleLayerManagerV2::
// optimize_local_window, src/simple_layer_manager.cpp:500-565; SimpleLayerManager::optimize_layer_local,
// src/layer_manager.cpp:137-179): 42 poses, 41 edges, one constant pose, 1-2 LM iterations, exact linear solve.  Through
// pgo_set_active + pgo_solve such a window costs E lanes of K1, N-row vector kernels and ~ten launches with host round trips
// per LM iteration; here the window is COMPACTED -- its poses and edges are addressed through host-built lists -- and
// everything (evaluate, assemble, dense Cholesky, candidate, accept / reject, termination tests) runs in LDS and registers
// of one workgroup, grid = number of windows.
//
// Layout of a window with np listed poses (n3 = 3 np unknowns, the constant ones kept as decoupled identity rows) and ne edges:
//   LDS   Hp   packed lower triangle of S J'J S + D'D, row-major: (i, j <= i) at i (i + 1) / 2 + j     n3 (n3 + 1) / 2 doubles
//         xs, cs, sc, gv, zv   poses, candidate (y on the way), Jacobi scales, gradient J'r, right-hand side / z / delta    5 n3
//         red  reduction scratch                                                                                          16
//   64 poses: 18528 + 960 + 16 doubles = 156,032 bytes of the 163,840 a workgroup may have; the launch asks for what the
//   largest window of the call needs (42 poses: 69,176 bytes).  At 396 VGPRs a CU holds one workgroup whatever the LDS.
//   regs  lane e < ne holds its edge: measurement, flags, residual (3) and Jacobian (18) at the current point and at the candidate
//   HBM   rec  the same 21 doubles per edge (structure of arrays per window), read by the assembly lanes: L2-resident scratch
// Determinism: one lane per edge / per pose row / per 3x3 block, every sum in the order of the window's own lists or by the
// fixed lane tree of block_sum_bcast; no atomics.  The handle's internal numbering only enters through the gather indices.
#pragma once
#include "kernels.hip.h"
#include "trust_region.h"

namespace pgo {
namespace dev {

constexpr int WIN_WG = 256;          // one lane per edge: PGO_WINDOW_MAX_EDGES
constexpr int WIN_REC = 21;          // J (3 x 6 row-major: [d e / d Pa | d e / d Pb]) then r (3), after DCS and the loss corrector
static_assert(PGO_WINDOW_MAX_EDGES == WIN_WG, "one lane per edge");
static_assert(PGO_WINDOW_MAX_POSES <= 255 && 3 * PGO_WINDOW_MAX_POSES <= WIN_WG - 1, "one lane per unknown plus the right-hand side's lane");

struct WinDesc {
  int32_t pose0, np;      // its poses: pidx[pose0 .. pose0 + np)
  int32_t edge0, ne;      // its edges: eloc / eab [edge0 .. edge0 + ne)
  int32_t anchor;         // list position of the constant pose
  int32_t blk0, nblk;     // its 3x3 blocks: blk[blk0 .. blk0 + nblk); block p < np is the diagonal block of pose p
  int32_t _pad;
};
struct WinArgs {
  const WinDesc* win;
  const int32_t* pidx;      // listed pose -> row of the handle's pose array
  const int32_t* eloc;      // listed edge -> local edge of the handle
  const int32_t* eab;       // listed edge -> list positions of its endpoints, a | b << 8
  const int32_t* blk;       // block -> list positions p | q << 8, p >= q
  const int32_t* blk_ptr;   // block -> its contributions ent[blk_ptr[b] .. blk_ptr[b + 1]), in edge-list order
  const int32_t* ent;       // contribution: listed edge << 1 | side of p (0: p is Edge::a)
  double* poses;            // the handle's poses (written only with commit)
  const double* mx;
  const double* my;
  const double* mt;
  const uint8_t* flags;
  double phi;
  LossClass loss0, loss1, loss2, loss3;
  int32_t max_iters, jacobi_scaling, commit, n3cap;
  double ftol, gtol, ptol, radius0, max_radius, min_radius, min_relative_decrease, min_lm_diagonal, max_lm_diagonal;
  double* rec;              // WIN_REC doubles per listed edge
  double* poses_out;        // 3 per listed pose
  pgo_window_result* results;
  pgo_iter_record* records; // (max_iters + 1) per window, or nullptr
};

// LDS doubles a window of n3 unknowns needs
__host__ __device__ constexpr int64_t win_lds_doubles(int64_t n3) { return n3 * (n3 + 1) / 2 + 5 * n3 + 16; }

__device__ __forceinline__ int win_tri(int i, int j) { return ((i * (i + 1)) >> 1) + j; }   // j <= i

// One residual block on the plain objective (edge_model.h: no information weighting, no switch): DCS when flags bit 0 says
// so, the corrector of the class's loss.  r, J: what Ceres' ResidualBlock::Evaluate hands the minimiser.
// cost = 1/2 rho(|e|^2), NaN when |e|^2 is not finite; jac_finite = every entry of the corrected Jacobian is finite.
__device__ __forceinline__ void win_edge_eval(const double* __restrict__ Pa, const double* __restrict__ Pb, double dx, double dy,
                                              double dth, unsigned fl, double phi, const LossClass& L, double (&r)[3],
                                              double (&J)[18], double& cost, bool& jac_finite) {
  double ex, ey, sind;
  edge_plain<true>(Pa[0], Pa[1], Pa[2], Pb[0], Pb[1], Pb[2], dx, dy, dth, ex, ey, sind, J);
  double et = asin(sind);
  if (fl & 1u) edge_dcs<true>(phi, ex, ey, et, J);
  const double s = ex * ex + ey * ey + et * et;
  double rho[3];
  loss_rho(L, s, rho);
  const double sc = sqrt(rho[1]);   // the corrector of a loss with rho'' <= 0, as in k_edge_eval
  bool fin = true;
#pragma unroll
  for (int c = 0; c < 18; ++c) {
    J[c] *= sc;
    fin = fin && isfinite(J[c]);
  }
  r[0] = sc * ex;
  r[1] = sc * ey;
  r[2] = sc * et;
  jac_finite = fin;
  cost = isfinite(s) ? 0.5 * rho[0] : __builtin_nan("");
}

// the lane's record to the scratch: value c of listed edge e at rec[c * ne + e]
__device__ __forceinline__ void win_store_rec(double* rec, int ne, int e, const double (&r)[3], const double (&J)[18]) {
#pragma unroll
  for (int c = 0; c < 18; ++c) rec[c * ne + e] = J[c];
#pragma unroll
  for (int c = 0; c < 3; ++c) rec[(18 + c) * ne + e] = r[c];
}

// lane p < np: diagonal of J'J and gradient J'r of pose p from the records, in the order of its contribution list;
// SCALES: also the Jacobi scales 1 / (1 + sqrt(diag)) (0 on a constant pose)
template <bool SCALES>
__device__ __forceinline__ void win_gradient(const WinArgs& A, const WinDesc& W, const double* rec, int jacobi,
                                             double* __restrict__ sc, double* __restrict__ gv) {
  const int p = threadIdx.x;
  if (p >= W.np) return;
  const int e0 = A.blk_ptr[W.blk0 + p], e1 = A.blk_ptr[W.blk0 + p + 1];
  const bool constant = p == W.anchor || e0 == e1;
  double d[3] = {0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
  for (int k = e0; k < e1; ++k) {
    const int en = A.ent[k], e = en >> 1, s = en & 1;
    const double r0 = rec[18 * W.ne + e], r1 = rec[19 * W.ne + e], r2 = rec[20 * W.ne + e];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double j0 = rec[(3 * s + c) * W.ne + e], j1 = rec[(6 + 3 * s + c) * W.ne + e], j2 = rec[(12 + 3 * s + c) * W.ne + e];
      d[c] += j0 * j0 + j1 * j1 + j2 * j2;
      g[c] += j0 * r0 + j1 * r1 + j2 * r2;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (SCALES) sc[3 * p + c] = constant ? 0.0 : (jacobi ? 1.0 / (1.0 + sqrt(d[c])) : 1.0);
    gv[3 * p + c] = constant ? 0.0 : g[c];
  }
}

template <int PGO_UNIT_ = 0>   // (a template so that only the translation unit that launches it carries it)
__global__ __launch_bounds__(WIN_WG) void k_window_solve(WinArgs A) {
  extern __shared__ __attribute__((aligned(16))) double win_lds[];
  const WinDesc W = A.win[blockIdx.x];
  const int tid = threadIdx.x, np = W.np, ne = W.ne, n3 = 3 * np;
  double* __restrict__ Hp = win_lds;
  double* __restrict__ xs = Hp + (((int64_t)A.n3cap * (A.n3cap + 1)) >> 1);
  double* __restrict__ cs = xs + A.n3cap;
  double* __restrict__ sc = cs + A.n3cap;
  double* __restrict__ gv = sc + A.n3cap;
  double* __restrict__ zv = gv + A.n3cap;
  double* red = zv + A.n3cap;
  double* rec = A.rec + (int64_t)W.edge0 * WIN_REC;   // (written and read by different lanes: no __restrict__)

  // ---- gather: poses through the translation list, the lane's edge from the handle's arrays (read in place)
  int my_row = 0;
  if (tid < n3) {
    my_row = A.pidx[W.pose0 + tid / 3];
    xs[tid] = A.poses[3 * (int64_t)my_row + tid % 3];
  }
  const bool is_edge = tid < ne;
  double dx = 0.0, dy = 0.0, dth = 0.0;
  unsigned fl = 0u;
  int pa = 0, pb = 0;
  if (is_edge) {
    const int k = A.eloc[W.edge0 + tid], ab = A.eab[W.edge0 + tid];
    dx = A.mx[k];
    dy = A.my[k];
    dth = A.mt[k];
    fl = A.flags[k];
    pa = ab & 255;
    pb = ab >> 8;
  }
  const LossClass L = pick_loss(A.loss0, A.loss1, A.loss2, A.loss3, (fl >> 2) & 3u);
  __syncthreads();

  // ---- the initial point
  double r[3] = {0.0, 0.0, 0.0}, J[18], rc[3] = {0.0, 0.0, 0.0}, Jc[18];
#pragma unroll
  for (int c = 0; c < 18; ++c) J[c] = Jc[c] = 0.0;
  double ecost = 0.0;
  if (is_edge) {
    bool jf;
    win_edge_eval(xs + 3 * pa, xs + 3 * pb, dx, dy, dth, fl, A.phi, L, r, J, ecost, jf);
    if (!jf) ecost = __builtin_nan("");
    win_store_rec(rec, ne, tid, r, J);
  }
  double cost = block_sum_bcast(ecost, red);   // (its barriers also order the records before the reads below)
  win_gradient<true>(A, W, rec, A.jacobi_scaling, sc, gv);
  __syncthreads();
  const bool is_row = tid < n3;
  const bool is_free = is_row && sc[is_row ? tid : 0] > 0.0;
  double gmax = block_max_bcast(is_free ? fabs(gv[tid]) : 0.0, red);
  double x_norm = sqrt(block_sum_bcast(is_free ? xs[tid] * xs[tid] : 0.0, red));
  const double initial_cost = cost;
  TrustRegion T = tr_begin(A.radius0);   // (wavefront-uniform scalars; handed to trust_region.h by reference: registers)
  int iter = 0, successful = 0, termination = 0, n_rec = 0;
  pgo_iter_record* recs = A.records ? A.records + (int64_t)blockIdx.x * (A.max_iters + 1) : nullptr;
  auto push = [&](int it, int ok, double c, double dc, double gm, double sn, double rd, double rad) {
    if (recs && tid == 0) {
      pgo_iter_record R;
      R.iter = it;
      R.step_ok = ok;
      R.cost = c;
      R.cost_change = dc;
      R.gradient_max_norm = gm;
      R.step_norm = sn;
      R.relative_decrease = rd;
      R.radius = rad;
      R.pcg_iters = 0;
      R._pad = 0;
      R.pcg_rel_residual = 0.0;
      R.seconds = 0.0;
      recs[n_rec] = R;
    }
    ++n_rec;
  };
  push(0, 1, cost, 0.0, gmax, 0.0, 0.0, T.radius);
  if (!isfinite(cost)) termination = PGO_TERM_FAILURE;   // "Residual and Jacobian evaluation failed" at the initial point

  // ---- TrustRegionMinimizer + LevenbergMarquardtStrategy: the decisions are trust_region.h's, scalar-uniform
  while (!termination) {
    termination = tr_stop_before_step(T, iter, A.max_iters, gmax, A.gtol, A.min_radius);
    if (termination) break;
    ++iter;
    // S J'J S (every 3x3 block summed by one lane in list order), right-hand side S J'r
    const int ntri = (n3 * (n3 + 1)) >> 1;
    for (int i = tid; i < ntri; i += WIN_WG) Hp[i] = 0.0;
    if (is_row) zv[tid] = sc[tid] * gv[tid];
    __syncthreads();
    for (int b = tid; b < W.nblk; b += WIN_WG) {
      const int pq = A.blk[W.blk0 + b], p = pq & 255, q = pq >> 8;
      const int e0 = A.blk_ptr[W.blk0 + b], e1 = A.blk_ptr[W.blk0 + b + 1];
      double h[9];
#pragma unroll
      for (int c = 0; c < 9; ++c) h[c] = 0.0;
      for (int k = e0; k < e1; ++k) {
        const int en = A.ent[k], e = en >> 1, sp = en & 1, sq = (p == q) ? sp : 1 - sp;
        double jp[9], jq[9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            jp[3 * i + c] = rec[(6 * i + 3 * sp + c) * ne + e];
            jq[3 * i + c] = rec[(6 * i + 3 * sq + c) * ne + e];
          }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int c = 0; c < 3; ++c) h[3 * a + c] += jp[a] * jq[c] + jp[3 + a] * jq[3 + c] + jp[6 + a] * jq[6 + c];
      }
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int c = 0; c < 3; ++c)
          if (p != q || c <= a) Hp[win_tri(3 * p + a, 3 * q + c)] = sc[3 * p + a] * sc[3 * q + c] * h[3 * a + c];
    }
    __syncthreads();
    // D'D = clip(diag) / radius; a constant pose is a decoupled identity row (k_prepare)
    if (is_row) {
      const int dd = win_tri(tid, tid);
      const double hii = Hp[dd];
      Hp[dd] = hii + (is_free ? fmin(fmax(hii, A.min_lm_diagonal), A.max_lm_diagonal) / T.radius : 1.0);
    }
    __syncthreads();
    // dense Cholesky by 3x3 block columns, right-looking; the right-hand side rides along as one more row (lane 255), so
    // that zv leaves as z = L^-1 S J'r
    bool lost = false;
    for (int kb = 0; kb < np; ++kb) {
      const int k = 3 * kb;
      const double a00 = Hp[win_tri(k, k)], a10 = Hp[win_tri(k + 1, k)], a11 = Hp[win_tri(k + 1, k + 1)];
      const double a20 = Hp[win_tri(k + 2, k)], a21 = Hp[win_tri(k + 2, k + 1)], a22 = Hp[win_tri(k + 2, k + 2)];
      const double l00 = sqrt(a00), l10 = a10 / l00, l20 = a20 / l00;
      const double t11 = a11 - l10 * l10, l11 = sqrt(t11), l21 = (a21 - l20 * l10) / l11;
      const double t22 = a22 - l20 * l20 - l21 * l21, l22 = sqrt(t22);
      if (!(a00 > 0.0) || !(t11 > 0.0) || !(t22 > 0.0)) {   // a lost pivot (uniform: every lane read the same block)
        lost = true;
        break;
      }
      const int i = k + 3 + tid;
      if (i < n3) {
        const int o = win_tri(i, k);
        const double w0 = Hp[o] / l00, w1 = (Hp[o + 1] - w0 * l10) / l11, w2 = (Hp[o + 2] - w0 * l20 - w1 * l21) / l22;
        Hp[o] = w0;
        Hp[o + 1] = w1;
        Hp[o + 2] = w2;
      }
      if (tid == WIN_WG - 1) {
        const double w0 = zv[k] / l00, w1 = (zv[k + 1] - w0 * l10) / l11, w2 = (zv[k + 2] - w0 * l20 - w1 * l21) / l22;
        zv[k] = w0;
        zv[k + 1] = w1;
        zv[k + 2] = w2;
      }
      __syncthreads();
      if (tid == 0) {   // (nothing below reads the diagonal block)
        Hp[win_tri(k, k)] = l00;
        Hp[win_tri(k + 1, k)] = l10;
        Hp[win_tri(k + 1, k + 1)] = l11;
        Hp[win_tri(k + 2, k)] = l20;
        Hp[win_tri(k + 2, k + 1)] = l21;
        Hp[win_tri(k + 2, k + 2)] = l22;
      }
      const int mb = np - kb - 1, npair = (mb * (mb + 1)) >> 1;
      for (int t = tid; t < npair; t += WIN_WG) {
        int ri = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
        while (((ri * (ri + 1)) >> 1) > t) --ri;
        while ((((ri + 1) * (ri + 2)) >> 1) <= t) ++ri;
        const int rj = t - ((ri * (ri + 1)) >> 1);
        const int bi = 3 * (kb + 1 + ri), bj = 3 * (kb + 1 + rj);
        double li[9], lj[9];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            li[3 * a + c] = Hp[win_tri(bi + a, k + c)];
            lj[3 * a + c] = Hp[win_tri(bj + a, k + c)];
          }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int c = 0; c < 3; ++c)
            if (ri != rj || c <= a)
              Hp[win_tri(bi + a, bj + c)] -= li[3 * a] * lj[3 * c] + li[3 * a + 1] * lj[3 * c + 1] + li[3 * a + 2] * lj[3 * c + 2];
      }
      if (i < n3) {
        const int o = win_tri(i, k);
        zv[i] -= Hp[o] * zv[k] + Hp[o + 1] * zv[k + 1] + Hp[o + 2] * zv[k + 2];
      }
      __syncthreads();
    }
    // L' y = z by block rows from the bottom; y lands in cs
    if (!lost) {
      for (int kb = np - 1; kb >= 0; --kb) {
        const int k = 3 * kb;
        const double l00 = Hp[win_tri(k, k)], l10 = Hp[win_tri(k + 1, k)], l11 = Hp[win_tri(k + 1, k + 1)];
        const double l20 = Hp[win_tri(k + 2, k)], l21 = Hp[win_tri(k + 2, k + 1)], l22 = Hp[win_tri(k + 2, k + 2)];
        const double y2 = zv[k + 2] / l22, y1 = (zv[k + 1] - l21 * y2) / l11, y0 = (zv[k] - l10 * y1 - l20 * y2) / l00;
        if (tid == 0) {
          cs[k] = y0;
          cs[k + 1] = y1;
          cs[k + 2] = y2;
        }
        if (tid < k) zv[tid] -= Hp[win_tri(k, tid)] * y0 + Hp[win_tri(k + 1, tid)] * y1 + Hp[win_tri(k + 2, tid)] * y2;
        __syncthreads();
      }
    }
    // step delta = -S y (kept in zv), candidate, |delta|^2; model decrease -(J delta).(r + J delta / 2): no D term
    double dl = 0.0;
    if (is_row) {
      dl = (is_free && !lost) ? -sc[tid] * cs[tid] : 0.0;
      zv[tid] = dl;
    }
    __syncthreads();   // (every lane has read y from cs)
    if (is_row) cs[tid] = xs[tid] + dl;
    const double step2 = block_sum_bcast(dl * dl, red);
    double me = 0.0;
    if (is_edge) {
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double m = J[6 * i] * zv[3 * pa] + J[6 * i + 1] * zv[3 * pa + 1] + J[6 * i + 2] * zv[3 * pa + 2] +
                         J[6 * i + 3] * zv[3 * pb] + J[6 * i + 4] * zv[3 * pb + 1] + J[6 * i + 5] * zv[3 * pb + 2];
        me -= m * (r[i] + 0.5 * m);
      }
    }
    const double model = block_sum_bcast(me, red);
    if (lost || !tr_step_usable(model, step2)) {   // invalid step
      if (tr_invalid_step(T)) {
        termination = PGO_TERM_FAILURE;
        --iter;   // as pgo_batch::iterate: the failed iteration is not counted (pgo_handle counts it)
        break;
      }
      push(iter, -1, cost, 0.0, gmax, 0.0, 0.0, T.radius);
      continue;
    }
    tr_valid_step(T);
    // the candidate: cost, and its Jacobian for the case that it is accepted
    double ccost = 0.0;
    bool jf = true;
    if (is_edge) win_edge_eval(cs + 3 * pa, cs + 3 * pb, dx, dy, dth, fl, A.phi, L, rc, Jc, ccost, jf);
    double cand_cost = block_sum_bcast(ccost, red);
    if (!isfinite(cand_cost)) cand_cost = TR_DBL_MAX;
    const double step_norm = sqrt(step2), cost_change = cost - cand_cost;
    termination = tr_tolerance_reached(step_norm, x_norm, A.ptol, cost_change, cost, A.ftol);
    if (termination) {
      push(iter, 0, cost, cost_change, gmax, step_norm, 0.0, T.radius);
      break;
    }
    const double rho = tr_rho(cand_cost, cost_change, model);
    if (rho > A.min_relative_decrease) {   // HandleSuccessfulStep
      // the radius is updated BEFORE the bad-Jacobian test, whose record carries the new radius (pgo_handle updates it only
      // after the accepted point has been re-linearised, and records the old radius on a failure there)
      tr_accept(T, rho, A.max_radius);
      ++successful;
      const double bad_jac = block_max_bcast(jf ? 0.0 : 1.0, red);
      if (bad_jac > 0.0) {   // non-finite Jacobian at an accepted point (the asin' singularity)
        termination = PGO_TERM_FAILURE;
        push(iter, 1, cost, cost_change, gmax, step_norm, rho, T.radius);
        break;
      }
      if (is_row) xs[tid] = cs[tid];
      if (is_edge) {
#pragma unroll
        for (int c = 0; c < 18; ++c) J[c] = Jc[c];
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c] = rc[c];
        win_store_rec(rec, ne, tid, r, J);
      }
      cost = cand_cost;
      __syncthreads();
      win_gradient<false>(A, W, rec, 0, sc, gv);
      __syncthreads();
      gmax = block_max_bcast(is_free ? fabs(gv[tid]) : 0.0, red);
      x_norm = sqrt(block_sum_bcast(is_free ? xs[tid] * xs[tid] : 0.0, red));
      push(iter, 1, cost, cost_change, gmax, step_norm, rho, T.radius);
    } else {   // HandleUnsuccessfulStep
      tr_reject(T);
      push(iter, 0, cand_cost, cost_change, gmax, step_norm, rho, T.radius);
    }
  }

  // ---- results: a failed window comes back unchanged
  const bool failed = termination == PGO_TERM_FAILURE;
  if (is_row) {
    const double v = failed ? A.poses[3 * (int64_t)my_row + tid % 3] : xs[tid];
    A.poses_out[3 * (int64_t)W.pose0 + tid] = v;
    if (A.commit && !failed) A.poses[3 * (int64_t)my_row + tid % 3] = v;
  }
  if (tid == 0) {
    pgo_window_result R;
    R.termination = termination;
    R.iterations = iter;
    R.successful_steps = successful;
    R.n_records = n_rec;
    R.initial_cost = initial_cost;
    R.final_cost = cost;
    A.results[blockIdx.x] = R;
  }
}

}  // namespace dev
}  // namespace pgo
