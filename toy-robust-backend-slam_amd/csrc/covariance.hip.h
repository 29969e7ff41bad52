#pragma once
// Kernels of pgo_pose_covariance and pgo_edge_gate (solver_covariance.hip): PCG on m right-hand sides at once for the
// undamped, Jacobi-scaled normal equations A X = B (B = S E: unit vectors; B = S J': the sparse columns of the gate).  Vectors are column-major panels [m][3N] in the internal pose order (column c at c * ld).
// Every column has its own scalars (CovCol) and stops on its own; a stopped column is frozen by the `done` mask.  Every
// reduction is a fixed-order sum of per-workgroup partials (no atomics): the results are bitwise reproducible.
#include "pgo.h"
#include "gate.h"
#include "kernels.hip.h"

namespace pgo {
namespace dev {

constexpr int COV_MAX_COLS = 48;   // 3 x 16 poses per pass
constexpr int COV_MC = 24;         // columns per sweep of k_spmm: 3 x 24 accumulators per lane

struct CovCol {        // per-column PCG scalars (device memory)
  double rz;           // r.z
  double bb;           // b.b
  double tol2;         // rtol^2 b.b
  double rr;           // r.r after the latest update
  double alpha, beta;
  int32_t done;        // 0 = running, 1 = converged, 2 = breakdown (p'Ap <= 0 or not finite), 3 = r.z <= 0 or not finite
  int32_t iters;
};

// Y = A P on the columns [c0, c0 + nc) of the panels, A = H + diag(d2) (H: hd planes + off-diagonal blocks of the row's
// incidences).  One row per lane: the row's off-diagonal blocks (72 B + the 4 B column index) are read ONCE per sweep and
// applied to all nc columns held in registers.  part[c * gridDim.x + block] = partial of p_c . y_c.
struct SpmmArgs {
  const int32_t* inc_ptr;
  const int32_t* inc_col;
  const double* hoff;
  const double* hd;        // 6 planes [n]
  const double* d2;        // [n x 3]
  int32_t n;
  int32_t c0, nc;
  int64_t ld;
  const double* p;
  double* y;
  double* part;
};

template <int MC>
__global__ __launch_bounds__(WG) void k_spmm(SpmmArgs A) {
  __shared__ double red[8];
  const int64_t n = A.n;
  double dot[MC];
#pragma unroll
  for (int c = 0; c < MC; ++c) dot[c] = 0.0;
  for (int row = blockIdx.x * WG + threadIdx.x; row < A.n; row += gridDim.x * WG) {
    const double a00 = A.hd[row] + A.d2[3 * (int64_t)row], a01 = A.hd[n + row], a02 = A.hd[2 * n + row],
                 a11 = A.hd[3 * n + row] + A.d2[3 * (int64_t)row + 1], a12 = A.hd[4 * n + row],
                 a22 = A.hd[5 * n + row] + A.d2[3 * (int64_t)row + 2];
    double acc[MC][3];
#pragma unroll
    for (int c = 0; c < MC; ++c) {
      acc[c][0] = acc[c][1] = acc[c][2] = 0.0;
      if (c < A.nc) {
        const double* pc = A.p + (A.c0 + c) * A.ld + 3 * (int64_t)row;
        const double p0 = pc[0], p1 = pc[1], p2 = pc[2];
        acc[c][0] = a00 * p0 + a01 * p1 + a02 * p2;
        acc[c][1] = a01 * p0 + a11 * p1 + a12 * p2;
        acc[c][2] = a02 * p0 + a12 * p1 + a22 * p2;
      }
    }
    const int q1 = A.inc_ptr[row + 1];
    for (int q = A.inc_ptr[row]; q < q1; ++q) {
      const int64_t col = A.inc_col[q];
      double h[9];
      hoff_load(A.hoff, q, h);
#pragma unroll
      for (int c = 0; c < MC; ++c) {
        if (c < A.nc) {
          const double* pc = A.p + (A.c0 + c) * A.ld + 3 * col;
          const double p0 = pc[0], p1 = pc[1], p2 = pc[2];
          acc[c][0] += h[0] * p0 + h[1] * p1 + h[2] * p2;
          acc[c][1] += h[3] * p0 + h[4] * p1 + h[5] * p2;
          acc[c][2] += h[6] * p0 + h[7] * p1 + h[8] * p2;
        }
      }
    }
#pragma unroll
    for (int c = 0; c < MC; ++c) {
      if (c < A.nc) {
        const int64_t o = (A.c0 + c) * A.ld + 3 * (int64_t)row;
        const double* pc = A.p + o;
        double* yc = A.y + o;
        yc[0] = acc[c][0];
        yc[1] = acc[c][1];
        yc[2] = acc[c][2];
        dot[c] += pc[0] * acc[c][0] + pc[1] * acc[c][1] + pc[2] * acc[c][2];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < MC; ++c) {
    if (c < A.nc) {
      const double s = block_sum_bcast(dot[c], red);
      if (threadIdx.x == 0) A.part[(int64_t)(A.c0 + c) * gridDim.x + blockIdx.x] = s;
    }
  }
}

// One candidate of pgo_edge_gate as k_gate_eval leaves it, a 64-byte-aligned record: the plain residual, its Jacobian
// [d r/d Pa | d r/d Pb] (3x6 row-major), the internal rows 3 a, 3 b of its endpoints, status 1 = r or J not finite, and
// nonzero = some entry of S J' is not 0 (an endpoint is not constant)
struct alignas(64) GateRec {
  double J[18];
  double r[3];
  int32_t ra, rb;
  int32_t status, nonzero;
};

// The right-hand sides of a pass, as functors: column(c) = what column c needs, at(col, i) = its entry in row i.
// RhsUnit: column c is S e_k with k = rows[c] (the internal row of pose component c) -- pgo_pose_covariance.
struct RhsUnit {
  const int32_t* __restrict__ rows;
  const double* __restrict__ scale;
  struct Col {
    int64_t k;
  };
  __device__ __forceinline__ Col column(int c) const { return Col{rows[c]}; }
  __device__ __forceinline__ double at(const Col& q, int64_t i) const { return (i == q.k) ? scale[i] : 0.0; }
};
// RhsSparse: column 3 j + c is S J_c' of the pass's j-th candidate (record cand[j]): scale[i] J[c][i - ra] on the rows
// ra .. ra + 2, the b half on rb .. rb + 2 (a != b) -- pgo_edge_gate.
struct RhsSparse {
  const GateRec* __restrict__ rec;
  const int32_t* __restrict__ cand;
  const double* __restrict__ scale;
  struct Col {
    int64_t ra, rb;
    const double* j;
  };
  __device__ __forceinline__ Col column(int c) const {
    const GateRec& g = rec[cand[c / 3]];
    return Col{g.ra, g.rb, g.J + 6 * (c % 3)};
  }
  __device__ __forceinline__ double at(const Col& q, int64_t i) const {
    const int64_t da = i - q.ra, db = i - q.rb;
    if (da >= 0 && da < 3) return scale[i] * q.j[da];
    if (db >= 0 && db < 3) return scale[i] * q.j[3 + db];
    return 0.0;
  }
};

// Right-hand sides and start: X = 0, R = B, P = 0.  Grid (g, m).  part_bb[c * g + block].
template <class RHS>
__global__ __launch_bounds__(WG) void k_cov_rhs(int64_t n3, int64_t ld, RHS B, double* __restrict__ x, double* __restrict__ r, double* __restrict__ p,
                                                double* __restrict__ part_bb) {
  __shared__ double red[8];
  const int c = blockIdx.y;
  const typename RHS::Col q = B.column(c);
  double bb = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x; i < n3; i += (int64_t)gridDim.x * WG) {
    const double b = B.at(q, i);
    x[c * ld + i] = 0.0;
    p[c * ld + i] = 0.0;
    r[c * ld + i] = b;
    bb += b * b;
  }
  bb = block_sum_bcast(bb, red);
  if (threadIdx.x == 0) part_bb[(int64_t)c * gridDim.x + blockIdx.x] = bb;
}

// partials of r_c . z_c (grid (g, m)); frozen columns write 0
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_cov_dot(int64_t n3, int64_t ld, const double* __restrict__ r, const double* __restrict__ z,
                                                const CovCol* __restrict__ cs, double* __restrict__ part) {
  __shared__ double red[8];
  const int c = blockIdx.y;
  double s = 0.0;
  if (!cs[c].done)
    for (int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x; i < n3; i += (int64_t)gridDim.x * WG) s += r[c * ld + i] * z[c * ld + i];
  s = block_sum_bcast(s, red);
  if (threadIdx.x == 0) part[(int64_t)c * gridDim.x + blockIdx.x] = s;
}

// start of the solve, one workgroup per column: b.b, r.z, tolerance; a zero right-hand side (the constant pose) is done at once
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_cov_start(CovCol* __restrict__ cs, const double* __restrict__ part_bb, const double* __restrict__ part_rz,
                                                  int g, double rtol) {
  __shared__ double red[8];
  const int c = blockIdx.x;
  const double bb = sum_partials_bcast(part_bb + (int64_t)c * g, g, red);
  const double rz = sum_partials_bcast(part_rz + (int64_t)c * g, g, red);
  if (threadIdx.x == 0) {
    CovCol s;
    s.rz = rz;
    s.bb = bb;
    s.tol2 = rtol * rtol * bb;
    s.rr = bb;
    s.alpha = s.beta = 0.0;
    s.iters = 0;
    s.done = (bb == 0.0) ? 1 : ((rz > 0.0 && isfinite(rz)) ? 0 : 3);
    cs[c] = s;
  }
}

// alpha_c = r.z / p'Ap, one workgroup per column (the product's partials in fixed order)
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_cov_alpha(CovCol* __restrict__ cs, const double* __restrict__ part_pap, int g) {
  __shared__ double red[8];
  const int c = blockIdx.x;
  if (cs[c].done) return;
  const double pap = sum_partials_bcast(part_pap + (int64_t)c * g, g, red);
  if (threadIdx.x == 0) {
    if (pap > 0.0 && isfinite(pap)) cs[c].alpha = cs[c].rz / pap;
    else cs[c].done = 2;
  }
}

// x += alpha p, r -= alpha A p, partials of r.r (grid (g, m)); frozen columns write 0
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_cov_update1(int64_t n3, int64_t ld, const CovCol* __restrict__ cs, double* __restrict__ x, double* __restrict__ r,
                                                    const double* __restrict__ p, const double* __restrict__ ap, double* __restrict__ part_rr) {
  __shared__ double red[8];
  const int c = blockIdx.y;
  double rr = 0.0;
  if (!cs[c].done) {
    const double alpha = cs[c].alpha;
    for (int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x; i < n3; i += (int64_t)gridDim.x * WG) {
      const int64_t o = c * ld + i;
      x[o] += alpha * p[o];
      const double ri = r[o] - alpha * ap[o];
      r[o] = ri;
      rr += ri * ri;
    }
  }
  rr = block_sum_bcast(rr, red);
  if (threadIdx.x == 0) part_rr[(int64_t)c * gridDim.x + blockIdx.x] = rr;
}

// after the preconditioner: the iteration is booked, convergence tested on r.r, beta = r.z_new / r.z (one workgroup per column)
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_cov_beta(CovCol* __restrict__ cs, const double* __restrict__ part_rr, const double* __restrict__ part_rz, int g) {
  __shared__ double red[8];
  const int c = blockIdx.x;
  if (cs[c].done) return;
  const double rr = sum_partials_bcast(part_rr + (int64_t)c * g, g, red);
  const double rz = sum_partials_bcast(part_rz + (int64_t)c * g, g, red);
  if (threadIdx.x == 0) {
    CovCol s = cs[c];
    s.iters += 1;
    s.rr = rr;
    if (rr <= s.tol2) s.done = 1;
    else if (!(rz > 0.0 && isfinite(rz))) s.done = 3;
    else {
      s.beta = rz / s.rz;
      s.rz = rz;
    }
    cs[c] = s;
  }
}

// p = z + beta p (grid (g, m)); frozen columns keep theirs
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_cov_pupdate(int64_t n3, int64_t ld, const CovCol* __restrict__ cs, const double* __restrict__ z, double* __restrict__ p) {
  const int c = blockIdx.y;
  if (cs[c].done) return;
  const double beta = cs[c].beta;
  for (int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x; i < n3; i += (int64_t)gridDim.x * WG) p[c * ld + i] = z[c * ld + i] + beta * p[c * ld + i];
}

// true residual R = B - A X of every column after the product A X (k_spmm into y): partials of |r|^2 (grid (g, m))
template <class RHS>
__global__ __launch_bounds__(WG) void k_cov_resid(int64_t n3, int64_t ld, RHS B, const double* __restrict__ ax, double* __restrict__ part) {
  __shared__ double red[8];
  const int c = blockIdx.y;
  const typename RHS::Col q = B.column(c);
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x; i < n3; i += (int64_t)gridDim.x * WG) {
    const double d = B.at(q, i) - ax[c * ld + i];
    s += d * d;
  }
  s = block_sum_bcast(s, red);
  if (threadIdx.x == 0) part[(int64_t)c * gridDim.x + blockIdx.x] = s;
}

// residual replacement for the columns of mask: r = B - A X from the product A X in ax (grid (g, m))
template <class RHS>
__global__ __launch_bounds__(WG) void k_cov_replace(int64_t n3, int64_t ld, RHS B, const double* __restrict__ ax, double* __restrict__ r,
                                                    const uint8_t* __restrict__ mask) {
  const int c = blockIdx.y;
  if (!mask[c]) return;
  const typename RHS::Col q = B.column(c);
  for (int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x; i < n3; i += (int64_t)gridDim.x * WG) r[c * ld + i] = B.at(q, i) - ax[c * ld + i];
}

// the columns of mask run again (one thread per column)
template <int PGO_UNIT_ = 0>
__global__ void k_cov_reopen(CovCol* __restrict__ cs, const uint8_t* __restrict__ mask, int m) {
  const int c = threadIdx.x;
  if (c < m && mask[c]) cs[c].done = 0;
}

// restart of the columns of mask from the replaced residual: r.z afresh, beta = 0 (p = z), tolerance and b.b kept
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_cov_restart(CovCol* __restrict__ cs, const double* __restrict__ part_rz, int g, const uint8_t* __restrict__ mask) {
  __shared__ double red[8];
  const int c = blockIdx.x;
  if (!mask[c]) return;
  const double rz = sum_partials_bcast(part_rz + (int64_t)c * g, g, red);
  if (threadIdx.x == 0) {
    cs[c].rz = rz;
    cs[c].beta = 0.0;
    cs[c].done = (rz > 0.0 && isfinite(rz)) ? 0 : 3;
  }
}

// ---- solver = 1 (the handle's direct solve): the column-major panels above meet the row-major panel T [n3][ldt] of the
// chain sweeps (direct.hip.h: one lane per column) in two transposes through a 32 x 33 LDS tile.  Grid (ldt / 32,
// n3 / 32 rounded up), block (32, 8).  Columns whose mask is 0 take no part in a step: their T is 0, their x is left alone.
//   k_cov_to_panel     T[i][c] = r_c[i] for the columns c < m with mask, 0 elsewhere (the padding columns included)
//   k_cov_from_panel   x_c[i] += T[i][c] for the columns c < m with mask
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(256) void k_cov_to_panel(int64_t n3, int64_t ld, int m, const double* __restrict__ r, const uint8_t* __restrict__ mask,
                                                      int64_t ldt, double* __restrict__ T) {
  __shared__ double tile[32][33];
  const int64_t i0 = (int64_t)blockIdx.y * 32;
  const int c0 = blockIdx.x * 32;
  for (int cc = threadIdx.y; cc < 32; cc += 8) {
    const int c = c0 + cc;
    const int64_t i = i0 + threadIdx.x;
    tile[cc][threadIdx.x] = (c < m && i < n3 && mask[c]) ? r[c * ld + i] : 0.0;
  }
  __syncthreads();
  for (int ii = threadIdx.y; ii < 32; ii += 8) {
    const int64_t i = i0 + ii;
    if (i < n3) T[i * ldt + c0 + threadIdx.x] = tile[threadIdx.x][ii];
  }
}

template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(256) void k_cov_from_panel(int64_t n3, int64_t ld, int m, const double* __restrict__ T, int64_t ldt,
                                                        const uint8_t* __restrict__ mask, double* __restrict__ x) {
  __shared__ double tile[32][33];
  const int64_t i0 = (int64_t)blockIdx.y * 32;
  const int c0 = blockIdx.x * 32;
  for (int ii = threadIdx.y; ii < 32; ii += 8) {
    const int64_t i = i0 + ii;
    tile[ii][threadIdx.x] = i < n3 ? T[i * ldt + c0 + threadIdx.x] : 0.0;
  }
  __syncthreads();
  for (int cc = threadIdx.y; cc < 32; cc += 8) {
    const int c = c0 + cc;
    const int64_t i = i0 + threadIdx.x;
    if (c < m && i < n3 && mask[c]) x[c * ld + i] += tile[threadIdx.x][cc];
  }
}

// out[c * n_out + j] = scale[rows_out[j]] * x_c[rows_out[j]]: the requested rows of Sigma's columns (Sigma = S X)
template <int PGO_UNIT_ = 0>
__global__ void k_cov_gather(int m, int64_t ld, const double* __restrict__ x, const double* __restrict__ scale, const int32_t* __restrict__ rows_out,
                             int n_out, double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)m * n_out) return;
  const int c = (int)(t / n_out), j = (int)(t - (int64_t)c * n_out);
  const int64_t k = rows_out[j];
  out[t] = scale[k] * x[c * ld + k];
}

// rows whose diagonal block of A has a non-positive or non-finite diagonal entry (a pose without edges, a NaN pose):
// per workgroup the smallest such row, or n
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_cov_check_rows(int n, const double* __restrict__ hd, const double* __restrict__ d2, int32_t* __restrict__ part) {
  __shared__ int32_t sh[WG];
  const int64_t nn = n;
  int bad = n;
  for (int row = blockIdx.x * WG + threadIdx.x; row < n; row += gridDim.x * WG) {
    const double a0 = hd[row] + d2[3 * (int64_t)row], a1 = hd[3 * nn + row] + d2[3 * (int64_t)row + 1],
                 a2 = hd[5 * nn + row] + d2[3 * (int64_t)row + 2];
    const bool ok = a0 > 0.0 && a1 > 0.0 && a2 > 0.0 && isfinite(a0) && isfinite(a1) && isfinite(a2) && isfinite(hd[nn + row]) &&
                    isfinite(hd[2 * nn + row]) && isfinite(hd[4 * nn + row]);
    if (!ok && row < bad) bad = row;
  }
  sh[threadIdx.x] = bad;
  __syncthreads();
  for (int s = WG / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) sh[threadIdx.x] = min(sh[threadIdx.x], sh[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

// ---------------------------------------------------------------- pgo_edge_gate
// One lane per candidate (a, b, meas) at the current poses: the plain model of edge_model.h -- the residual with the heading
// clamped as in k_edge_chi2, the Jacobian as in K1 (g = cos delta / sqrt(1 - sin^2 delta), unclamped) -- both unscaled.  ia, ib:
// internal pose indices.  flags[k] = status | nonzero << 1 for the host's pass plan.
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_gate_eval(int n, const int32_t* __restrict__ ia, const int32_t* __restrict__ ib, const double* __restrict__ meas,
                                                  const double* __restrict__ poses, const double* __restrict__ scale, GateRec* __restrict__ rec,
                                                  int32_t* __restrict__ flags) {
  const int k = blockIdx.x * WG + threadIdx.x;
  if (k >= n) return;
  const int a = ia[k], b = ib[k];
  const double dx = meas[3 * (int64_t)k], dy = meas[3 * (int64_t)k + 1], dth = meas[3 * (int64_t)k + 2];
  const double x1 = poses[3 * (int64_t)a], y1 = poses[3 * (int64_t)a + 1], t1 = poses[3 * (int64_t)a + 2];
  const double x2 = poses[3 * (int64_t)b], y2 = poses[3 * (int64_t)b + 1], t2 = poses[3 * (int64_t)b + 2];
  GateRec R;
  double ex, ey, sind;
  edge_plain<true>(x1, y1, t1, x2, y2, t2, dx, dy, dth, ex, ey, sind, R.J);   // (edge_model.h)
  const double et = asin(fmin(1.0, fmax(-1.0, sind)));
  R.r[0] = ex;
  R.r[1] = ey;
  R.r[2] = et;
  R.ra = 3 * a;
  R.rb = 3 * b;
  bool finite = isfinite(ex) && isfinite(ey) && isfinite(et);
  bool nz = false;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int d = 0; d < 6; ++d) {
      const double v = R.J[6 * c + d];
      finite = finite && isfinite(v);
      nz = nz || (scale[(d < 3 ? R.ra + d : R.rb + d - 3)] * v != 0.0);
    }
  R.status = finite ? 0 : 1;
  R.nonzero = (finite && nz) ? 1 : 0;
  rec[k] = R;
  flags[k] = R.status | (R.nonzero << 1);
}

// One 3x3 block of J Sigma J', unsymmetrised: P[a][c] = J_g[a] . (S x_c) over the six rows the Jacobian of g touches, x_c =
// x + c ld the three solved columns of ONE candidate (g itself: a diagonal block, k_gate_reduce; another one: a cross block,
// k_gate_cross).  x == nullptr: zeros.  Fixed-order sums.
__device__ __forceinline__ void gate_block(const GateRec& g, const double* __restrict__ x, int64_t ld, const double* __restrict__ scale, double P[9]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double y[6];   // rows ra .. ra + 2, rb .. rb + 2 of column c of Sigma J'
#pragma unroll
    for (int d = 0; d < 6; ++d) {
      const int64_t row = d < 3 ? g.ra + d : g.rb + d - 3;
      y[d] = x ? scale[row] * x[(int64_t)c * ld + row] : 0.0;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double s = 0.0;
#pragma unroll
      for (int d = 0; d < 6; ++d) s += g.J[6 * a + d] * y[d];
      P[3 * a + c] = s;
    }
  }
}

// One lane per candidate of a pass (record cand[j], columns 3 j .. 3 j + 2 of the panel x): the six rows of S X its
// Jacobian touches, P = J (S X) symmetrised, the 3x3 algebra of gate.h, the result record out[cand[j]].  x == nullptr: the
// candidates that took no columns (P = 0: both endpoints constant; status 1: every double NaN).  Fixed-order sums, no
// atomics.  info6: n x 6 in the caller's candidate order, or nullptr = the identity.
template <int PGO_UNIT_ = 0>
__global__ void k_gate_reduce(int k, const int32_t* __restrict__ cand, const GateRec* __restrict__ rec, const double* __restrict__ x, int64_t ld,
                              const double* __restrict__ scale, const double* __restrict__ info6, pgo_edge_gate_result* __restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  const int q = cand[j];
  const GateRec& g = rec[q];
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  pgo_edge_gate_result o;
  o._pad = 0;
  o.status = g.status;
  if (g.status) {
    for (int i = 0; i < 3; ++i) o.r[i] = nan;
    for (int i = 0; i < 18; ++i) o.J[i] = nan;
    for (int i = 0; i < 9; ++i) o.P[i] = nan;
    o.chi2 = o.chi2_marginal = o.info_gain = nan;
    out[q] = o;
    return;
  }
  double P[9];
  gate_block(g, x ? x + (int64_t)3 * j * ld : nullptr, ld, scale, P);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = a + 1; c < 3; ++c) P[3 * a + c] = P[3 * c + a] = 0.5 * (P[3 * a + c] + P[3 * c + a]);
  double res[3] = {nan, nan, nan};
  (void)gate_evaluate(g.r, P, info6 ? info6 + 6 * (int64_t)q : nullptr, res);   // (M not positive definite: NaNs, named by the host)
  for (int i = 0; i < 3; ++i) o.r[i] = g.r[i];
  for (int i = 0; i < 18; ++i) o.J[i] = g.J[i];
  for (int i = 0; i < 9; ++i) o.P[i] = P[i];
  o.chi2 = res[0];
  o.chi2_marginal = res[1];
  o.info_gain = res[2];
  out[q] = o;
}

// ---------------------------------------------------------------- pgo_edge_gate_joint
// After every pass: the blocks of C = [J_q Sigma J_p'] (order W = 3n, the caller's candidate order) between EVERY candidate
// with columns, q = all[0 .. n_all), and the k candidates of the pass, p = cand[j] with the columns 3 j .. 3 j + 2 of the
// panel x.  One lane per pair, neighbours sharing the columns; every entry of C is written by one lane, once per call.
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_gate_cross(int n_all, const int32_t* __restrict__ all, int k, const int32_t* __restrict__ cand,
                                                   const GateRec* __restrict__ rec, const double* __restrict__ x, int64_t ld,
                                                   const double* __restrict__ scale, int64_t W, double* __restrict__ C) {
  const int t = blockIdx.x * WG + threadIdx.x;
  if (t >= n_all * k) return;
  const int j = t / n_all, q = all[t % n_all], p = cand[j];
  double P[9];
  gate_block(rec[q], x + (int64_t)3 * j * ld, ld, scale, P);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c) C[(3 * (int64_t)q + a) * W + 3 * p + c] = P[3 * a + c];
}

// P = 1/2 (C + C'), the diagonal as it stands: a diagonal block comes out bitwise as k_gate_reduce symmetrises its own
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_gate_symmetrise(int64_t W, const double* __restrict__ C, double* __restrict__ P) {
  const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (t >= W * W) return;
  const int64_t i = t / W, j = t % W;
  P[t] = i == j ? C[t] : 0.5 * (C[i * W + j] + C[j * W + i]);
}

// the working state of the elimination: rho <- r, the status of every candidate in the caller's order
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_gate_joint_begin(int n, const GateRec* __restrict__ rec, double* __restrict__ rho, int32_t* __restrict__ status) {
  const int q = blockIdx.x * WG + threadIdx.x;
  if (q >= n) return;
  for (int i = 0; i < 3; ++i) rho[3 * q + i] = rec[q].r[i];
  status[q] = rec[q].status;
}

// The elimination of the joint gate (gate.h: gate_joint_decide, gate_pivot_row, gate_downdate), candidates k0 .. k1 - 1 in
// order.  Every workgroup decides candidate k for itself from (rho_k, M_kk) -- the same numbers, the same decision -- and forms
// all of B in LDS; workgroup 0 writes the record and downdates rho; the rows of the trailing matrix are dealt to the
// workgroups in turn, GATE_JOINT_WG / 256 rows at a time, 256 lanes along a row.  A launch reads row / column block k and
// writes only indices > k, so the workgroups of one launch never meet.  Two admissible shapes from this one body:
//   one launch, ONE workgroup, k0 .. k1 = 0 .. n (the barrier at the end of a step orders it against the next);
//   one launch per candidate (k1 = k0 + 1), any grid.
// Never a grid of several workgroups with k1 > k0 + 1: there is no barrier across workgroups here.  No atomics; every sum in
// fixed order, independent of the grid.
constexpr int GATE_JOINT_WG = 1024;
struct GateJointArgs {
  int n, k0, k1;
  double* M;      // (3n)^2 row-major, symmetric: P on entry
  double* rho;    // 3n
  const double* info6;   // n x 6 or nullptr
  const int32_t* status;
  const int8_t* force;   // n or nullptr
  double chi2_gate, min_info_gain;
  pgo_gate_joint_result* joint;
};
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(GATE_JOINT_WG) void k_gate_joint_step(GateJointArgs A) {
  __shared__ double B[9 * PGO_GATE_JOINT_MAX];
  __shared__ GatePivot piv;
  __shared__ int go;
  const int64_t W = 3 * (int64_t)A.n;
  for (int k = A.k0; k < A.k1; ++k) {
    if (threadIdx.x == 0) {
      double Mkk[9], rk[3];
      for (int a = 0; a < 3; ++a) {
        rk[a] = A.rho[3 * k + a];
        for (int b = 0; b < 3; ++b) Mkk[3 * a + b] = A.M[(3 * (int64_t)k + a) * W + 3 * k + b];
      }
      pgo_gate_joint_result o;
      GatePivot v;
      const int st = gate_joint_decide(rk, Mkk, A.info6 ? A.info6 + 6 * (int64_t)k : nullptr, A.status[k], A.force ? A.force[k] : -1, A.chi2_gate,
                                       A.min_info_gain, &o, &v);
      go = st == GATE_OK && o.accepted;
      if (go) piv = v;
      if (blockIdx.x == 0) A.joint[k] = o;
    }
    __syncthreads();
    const int64_t lo = 3 * (int64_t)(k + 1);
    if (go) {   // (the same for every lane of the workgroup)
      for (int64_t p = lo + threadIdx.x; p < W; p += GATE_JOINT_WG) {
        const double m[3] = {A.M[p * W + 3 * k], A.M[p * W + 3 * k + 1], A.M[p * W + 3 * k + 2]};
        gate_pivot_row(piv, m, &B[3 * p]);
      }
      __syncthreads();
      if (blockIdx.x == 0)
        for (int64_t p = lo + threadIdx.x; p < W; p += GATE_JOINT_WG) A.rho[p] = gate_downdate(A.rho[p], &B[3 * p], piv.y);
      const int lane = threadIdx.x % 256, rl = threadIdx.x / 256, RL = GATE_JOINT_WG / 256;
      for (int64_t p = lo + (int64_t)blockIdx.x * RL + rl; p < W; p += (int64_t)gridDim.x * RL)
        for (int64_t q = lo + lane; q < W; q += 256) A.M[p * W + q] = gate_downdate(A.M[p * W + q], &B[3 * p], &B[3 * q]);
    }
    __syncthreads();
  }
}

}  // namespace dev
}  // namespace pgo
