#pragma once
// Kernels of pgo_posterior_sample (solver_covariance.hip): perturb-and-MAP draws delta ~ N(0, (J'J)^-1) -- eps ~ N(0, I) in
// residual space, one triple per edge (sample.h), b = S J' eps in the scaled space of the undamped system, A x = b by the
// covariance session (covariance.hip.h), delta = S x -- and their second moment per pose.
//   k_sample_rhs      b_c = S J' eps_c on the rows, for the columns of a pass: one lane per row walks the row's incidences in
//                     incidence order (K2's order) and regenerates every edge's triple where it is consumed.  No atomics, every
//                     entry one fixed-order sum: bitwise independent of the grid and of the column's place in a pass.
//   k_sample_prior    b_c += S R eps_p on the rows with a pose prior (R R' = rho' Lambda): one lane per prior, rows are unique
//   k_sample_eps      the triples of one sample in the caller's edge order (pgo_debug_sample_rhs)
//   k_sample_accum    one lane per pose: delta = S x for the pass's columns in column order, the six unique entries of
//                     delta delta' added to six accumulator planes; the unscaled column into a staging panel in the caller's numbering
//   k_sample_finish   the planes / (number of samples), expanded to row-major 3x3 blocks in the caller's numbering
// The panel k_sample_rhs writes is the session's dense right-hand side (RhsDense): k_cov_rhs starts the solve from it as it
// does for the other kinds, and the true-residual and replacement steps read it again.
#include "covariance.hip.h"
#include "sample.h"

namespace pgo {
namespace dev {

// RhsDense: column c is the c-th column of a panel of its own, at(col, i) = panel[col * ld + i] -- pgo_posterior_sample.
struct RhsDense {
  const double* __restrict__ panel;
  int64_t ld;
  struct Col {
    const double* p;
  };
  __device__ __forceinline__ Col column(int c) const { return Col{panel + c * ld}; }
  __device__ __forceinline__ double at(const Col& q, int64_t i) const { return q.p[i]; }
};

struct SampleRhsArgs {
  const double* jr;          // K1's records, REC doubles per local edge
  const int32_t* inc_ptr;    // n + 1
  const int32_t* inc_edge;   // (local edge << 1) | side; < 0: a null incidence of a padded tile
  const int32_t* orig;       // local edge -> the caller's edge index (the noise is keyed by it)
  const double* scale;       // [n x 3] Jacobi scales, 0 on a constant pose
  int32_t n;                 // rows
  int32_t m;                 // columns of the pass
  int32_t sample0;           // global sample number of column 0
  uint64_t seed;
  int64_t ld;
  double* b;                 // [m][ld]
};

// Grid (ceil(n / WG), m): one lane per row, one column per blockIdx.y, as k_cov_rhs.  The record of an incidence is read with
// five 16-byte loads (A and g2).  Holding the record in registers for several columns of one launch was compiled too: it costs
// vector registers and, above all, scalar ones (the resource table) -- the kernel is bound by the generator's
// arithmetic, not by the records, which the columns of a launch share through L2.
template <bool UNIT>   // UNIT: the scales replaced by 1 (0 stays 0)
__global__ __launch_bounds__(WG) void k_sample_rhs(SampleRhsArgs A) {
  const int row = blockIdx.x * WG + threadIdx.x, c = blockIdx.y;
  if (row >= A.n) return;
  const uint32_t sample = (uint32_t)(A.sample0 + c);
  double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
  const int q1 = A.inc_ptr[row + 1];
  for (int q = A.inc_ptr[row]; q < q1; ++q) {
    const int ed = A.inc_edge[q];
    if (ed < 0) continue;
    const int e = ed >> 1;
    const double2* rp = reinterpret_cast<const double2*>(A.jr + (int64_t)e * REC);
    double R[10];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const double2 v = rp[k];
      R[2 * k] = v.x;
      R[2 * k + 1] = v.y;
    }
    double z[3];
    sample_triple(A.seed, SAMPLE_STREAM_EDGE, (uint32_t)A.orig[e], sample, z);
    // A' eps on the first endpoint; [-A[:,0] | -A[:,1] | (0, 0, g2)']' eps on the second
    const bool first = (ed & 1) == 0;
    const double t0 = R[0] * z[0] + R[3] * z[1] + R[6] * z[2], t1 = R[1] * z[0] + R[4] * z[1] + R[7] * z[2];
    const double t2 = first ? R[2] * z[0] + R[5] * z[1] + R[8] * z[2] : R[9] * z[2];
    acc0 += first ? t0 : -t0;
    acc1 += first ? t1 : -t1;
    acc2 += t2;
  }
  const double* sc = A.scale + 3 * (int64_t)row;
  double s0 = sc[0], s1 = sc[1], s2 = sc[2];
  if (UNIT) {
    s0 = s0 != 0.0 ? 1.0 : 0.0;
    s1 = s1 != 0.0 ? 1.0 : 0.0;
    s2 = s2 != 0.0 ? 1.0 : 0.0;
  }
  double* o = A.b + c * A.ld + 3 * (int64_t)row;
  o[0] = s0 * acc0;
  o[1] = s1 * acc1;
  o[2] = s2 * acc2;
}

struct SamplePriorArgs {
  const int32_t* row;      // [n] internal rows, ascending and unique
  const int32_t* order;    // [n] the prior's position in the order given to pgo_set_priors (the noise is keyed by it)
  const double* rec;       // [PRIOR_REC][n] of k_prior_eval<true>: rho' Lambda in planes 0 .. 5, what k_prior_add applied
  const double* scale;
  int32_t n, m, sample0, unit;
  uint64_t seed;
  int64_t ld;
  double* b;
};

template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_sample_prior(SamplePriorArgs A) {
  const int64_t n = A.n;
  const int c = blockIdx.y;
  for (int64_t k = (int64_t)blockIdx.x * WG + threadIdx.x; k < n; k += (int64_t)gridDim.x * WG) {
    const double l[6] = {A.rec[k], A.rec[n + k], A.rec[2 * n + k], A.rec[3 * n + k], A.rec[4 * n + k], A.rec[5 * n + k]};
    double R[9], z[3];
    sample_chol3_psd(l, R);
    sample_triple(A.seed, SAMPLE_STREAM_PRIOR, (uint32_t)A.order[k], (uint32_t)(A.sample0 + c), z);
    const int64_t r = A.row[k];
    double s[3] = {A.scale[3 * r], A.scale[3 * r + 1], A.scale[3 * r + 2]};
    if (A.unit)
      for (int a = 0; a < 3; ++a) s[a] = s[a] != 0.0 ? 1.0 : 0.0;
    double* o = A.b + c * A.ld + 3 * r;
    o[0] += s[0] * (R[0] * z[0]);
    o[1] += s[1] * (R[3] * z[0] + R[4] * z[1]);
    o[2] += s[2] * (R[6] * z[0] + R[7] * z[1] + R[8] * z[2]);
  }
}

template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_sample_eps(int64_t n_edges, const int32_t* __restrict__ orig, uint64_t seed, int32_t sample,
                                                   double* __restrict__ eps) {
  for (int64_t e = (int64_t)blockIdx.x * WG + threadIdx.x; e < n_edges; e += (int64_t)gridDim.x * WG) {
    const int64_t o = orig[e];
    double z[3];
    sample_triple(seed, SAMPLE_STREAM_EDGE, (uint32_t)o, (uint32_t)sample, z);
    eps[3 * o] = z[0];
    eps[3 * o + 1] = z[1];
    eps[3 * o + 2] = z[2];
  }
}

// acc: six planes [n] (00 01 02 11 12 22), read and written once per pass; stage (or nullptr): [m][ld] in the caller's
// numbering, inv[row] = the caller's pose of an internal row (nullptr: the identity).  The columns are added in column
// order, the passes come in sample order: every plane entry is one sum in global sample order, whatever the pass width.
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_sample_accum(int32_t n, int32_t m, int64_t ld, const double* __restrict__ x, const double* __restrict__ scale,
                                                     const int32_t* __restrict__ inv, double* __restrict__ acc, double* __restrict__ stage) {
  const int64_t nn = n;
  for (int64_t row = (int64_t)blockIdx.x * WG + threadIdx.x; row < nn; row += (int64_t)gridDim.x * WG) {
    const double s0 = scale[3 * row], s1 = scale[3 * row + 1], s2 = scale[3 * row + 2];
    double a00 = acc[row], a01 = acc[nn + row], a02 = acc[2 * nn + row], a11 = acc[3 * nn + row], a12 = acc[4 * nn + row], a22 = acc[5 * nn + row];
    const int64_t out = 3 * (inv ? (int64_t)inv[row] : row);
    for (int c = 0; c < m; ++c) {
      const double* xc = x + c * ld + 3 * row;
      const double d0 = s0 * xc[0], d1 = s1 * xc[1], d2 = s2 * xc[2];
      a00 += d0 * d0;
      a01 += d0 * d1;
      a02 += d0 * d2;
      a11 += d1 * d1;
      a12 += d1 * d2;
      a22 += d2 * d2;
      if (stage) {
        double* o = stage + c * ld + out;
        o[0] = d0;
        o[1] = d1;
        o[2] = d2;
      }
    }
    acc[row] = a00;
    acc[nn + row] = a01;
    acc[2 * nn + row] = a02;
    acc[3 * nn + row] = a11;
    acc[4 * nn + row] = a12;
    acc[5 * nn + row] = a22;
  }
}

// cov [n x 9] in the caller's numbering: the second moment about the known mean 0 -- the divisor is the number of samples
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_sample_finish(int32_t n, double n_samples, const double* __restrict__ acc, const int32_t* __restrict__ inv,
                                                      double* __restrict__ cov) {
  const int64_t nn = n;
  for (int64_t row = (int64_t)blockIdx.x * WG + threadIdx.x; row < nn; row += (int64_t)gridDim.x * WG) {
    const double c00 = acc[row] / n_samples, c01 = acc[nn + row] / n_samples, c02 = acc[2 * nn + row] / n_samples,
                 c11 = acc[3 * nn + row] / n_samples, c12 = acc[4 * nn + row] / n_samples, c22 = acc[5 * nn + row] / n_samples;
    double* o = cov + 9 * (inv ? (int64_t)inv[row] : row);
    o[0] = c00;
    o[1] = c01;
    o[2] = c02;
    o[3] = c01;
    o[4] = c11;
    o[5] = c12;
    o[6] = c02;
    o[7] = c12;
    o[8] = c22;
  }
}

}  // namespace dev
}  // namespace pgo
