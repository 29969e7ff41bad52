#pragma once
// Kernels of pgo_pose_covariance (solver_covariance.hip): PCG on m right-hand sides at once for the undamped, Jacobi-scaled
// normal equations A X = S E.  Vectors are column-major panels [m][3N] in the internal pose order (column c at c * ld).
// Every column has its own scalars (CovCol) and stops on its own; a stopped column is frozen by the `done` mask.  Every
// reduction is a fixed-order sum of per-workgroup partials (no atomics): the results are bitwise reproducible.
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

// Right-hand sides and start: column c is S e_k with k = rows[c] (the internal row of pose component c); X = 0, R = B, P = 0.
// Grid (g, m).  part_bb[c * g + block].
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_cov_rhs(int64_t n3, int64_t ld, const int32_t* __restrict__ rows, const double* __restrict__ scale,
                                                double* __restrict__ x, double* __restrict__ r, double* __restrict__ p, double* __restrict__ part_bb) {
  __shared__ double red[8];
  const int c = blockIdx.y;
  const int64_t k = rows[c];
  double bb = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x; i < n3; i += (int64_t)gridDim.x * WG) {
    const double b = (i == k) ? scale[i] : 0.0;
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

// true residual R = S E - A X of every column after the product A X (k_spmm into y): partials of |r|^2 (grid (g, m))
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_cov_resid(int64_t n3, int64_t ld, const int32_t* __restrict__ rows, const double* __restrict__ scale,
                                                  const double* __restrict__ ax, double* __restrict__ part) {
  __shared__ double red[8];
  const int c = blockIdx.y;
  const int64_t k = rows[c];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x; i < n3; i += (int64_t)gridDim.x * WG) {
    const double d = ((i == k) ? scale[i] : 0.0) - ax[c * ld + i];
    s += d * d;
  }
  s = block_sum_bcast(s, red);
  if (threadIdx.x == 0) part[(int64_t)c * gridDim.x + blockIdx.x] = s;
}

// residual replacement for the columns of mask: r = S e - A X from the product A X in ax (grid (g, m))
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_cov_replace(int64_t n3, int64_t ld, const int32_t* __restrict__ rows, const double* __restrict__ scale,
                                                    const double* __restrict__ ax, double* __restrict__ r, const uint8_t* __restrict__ mask) {
  const int c = blockIdx.y;
  if (!mask[c]) return;
  const int64_t k = rows[c];
  for (int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x; i < n3; i += (int64_t)gridDim.x * WG)
    r[c * ld + i] = ((i == k) ? scale[i] : 0.0) - ax[c * ld + i];
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

}  // namespace dev
}  // namespace pgo
