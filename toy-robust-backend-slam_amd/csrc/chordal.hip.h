#pragma once
// Chordal initialisation kernels (include/pgo.h, "chordal initialisation"; chordal.h is the one statement).  Launched by
// solver_chordal.hip only.  Everything walks the CALLER's numbering through tables the host built once per handle (the slot
// table, the edge tables of pgo_coarsen); no atomics, every sum runs in a fixed tree over tiles of 256 rows or chunks of 256
// edges whatever the grid: two calls are bitwise equal, the internal pose ordering plays no part, and neither does the grid.
//   k_chordal_assemble   one lane per row: the row's 16-byte slot values, d (summed in slot order), b, x0, the identity flag
//   k_chordal_spmv       q = H p.  A workgroup takes a tile of 256 rows, each wavefront 64 consecutive rows: their slots are one
//                        contiguous run, which the lanes stride 64 at a time (16-byte value load, 4-byte column load, 16-byte
//                        gather of p[col]); the products go through the wavefront's own LDS row (wave-level synchronisation
//                        only) and the lane of a row adds its slots in slot order.
//                        The tile's partial of Re(p^H q) goes to part[PQ]
//   k_chordal_residual   r = b - q, z = r / d, p = z; the tile's partials of r.z, |r|^2, |b|^2
//   k_chordal_begin      ONE workgroup: folds them into the state; done[0]
//   k_chordal_update     folds part[PQ] (every workgroup the same sum) into alpha; x += alpha p, r -= alpha q, z = r / d; partials
//   k_chordal_direction  folds them into beta and |r|^2; p = z + beta p; workgroup 0 writes the state of the next iteration
//   k_chordal_headings   stage R's result per pose; partials of the degenerate count and of min |z|
//   k_chordal_finish     the poses, the per-edge report, the reject decision; partials of the counts
//   k_chordal_fold       ONE workgroup: the counts in fixed order (as doubles: exact)
//   k_chordal_commit     the poses into the handle's;  k_chordal_apply   0 into the weight plane on the rejected edges
// The state carries rz and done twice, indexed by the iteration's parity: a kernel reads what the previous launch wrote and
// writes the other half, so no launch reads what one of its own workgroups writes.
#include <hip/hip_runtime.h>

#include "chordal.h"
#include "kernels.hip.h"

namespace pgo {
namespace dev {

constexpr int CHORDAL_TILE = WG;     // rows per tile: WG / 64 wavefronts x 64 rows
enum { CH_PQ = 0, CH_RZ, CH_RR, CH_BB, CH_DEG, CH_MAG, CH_NEW, CH_BAD, CHORDAL_NPART };

struct ChordalState {
  double rz[2];
  double rr, bb;
  double n_degenerate, min_mag, n_new, n_bad;
  int32_t done[2];
  int32_t iters, _pad;
};

struct ChordalDevGraph {
  const double *mx, *my, *mt;   // the handle's measurements (local edge order)
  const int32_t* loc;           // [n_edges] caller's edge -> local edge
  const double* poses;          // the handle's poses, internal numbering
  const int32_t* perm;          // caller's pose -> internal position; nullptr = the identity
  const uint8_t* is_const;      // [n] caller's numbering
  const double* T;              // [n x SUPPORT_POSE]
  __host__ __device__ __forceinline__ void meas(int32_t e, double* x, double* y, double* t) const {
    const int64_t l = loc[e];
    *x = mx[l];
    *y = my[l];
    *t = mt[l];
  }
  __host__ __device__ __forceinline__ void pose(int32_t i, double* x, double* y, double* th) const {
    const double* p = poses + 3 * (int64_t)(perm ? perm[i] : i);
    *x = p[0];
    *y = p[1];
    *th = p[2];
  }
  __host__ __device__ __forceinline__ bool constant(int32_t i) const { return is_const[i] != 0; }
  __host__ __device__ __forceinline__ Se2 traj(int32_t i) const { return support_load(T + (int64_t)SUPPORT_POSE * i); }
};

struct ChordalArgs {
  ChordalDevGraph g;
  const int32_t *rp, *col, *se;   // the slot table: [n + 1], [n_slots], [n_slots]
  const int32_t *ea, *eb;         // [n_edges] caller's endpoints
  const int32_t* eloc;            // [n_edges] pgo_coarsen's table: < 0 on a chain edge
  double* u;                      // [n_edges] the call's working weights
  uint8_t* rej;                   // [n_edges] rejected by a round of this call
  Cx *val, *b, *x, *r, *z, *p, *q, *zh;
  double *d, *theta;
  uint8_t* ident;
  double* part;                   // [CHORDAL_NPART][n_part]
  ChordalState* st;
  double *poses_out, *res_out;    // [n x 3], [n_edges x 2]
  double* w;                      // the weight plane (k_chordal_apply), local edge order
  double* h_poses;                // the handle's poses (k_chordal_commit)
  int32_t n, n_edges, n_tiles, n_chunks, n_part, c0, stage, it, reject, _pad;
  double rtol, mag_min, reject_xy, reject_th;
};

template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_chordal_assemble(ChordalArgs A) {
  const ChordalStart S = chordal_start(A.g, A.c0);
  for (int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * WG)
    chordal_row(A.g, S, A.stage, (int32_t)i, A.rp, A.col, A.se, A.u, A.zh, A.val, A.d + i, A.b + i, A.x + i, A.ident + i);
}

// q = H v; part[CH_PQ][tile] = the tile's sum of Re(v_i^H q_i)
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_chordal_spmv(ChordalArgs A, const Cx* __restrict__ v, Cx* __restrict__ q) {
  __shared__ Cx prod[WG / 64][64];
  __shared__ double red[8];
  if (A.st->done[A.it & 1]) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n = A.n;
  for (int tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
    const int64_t t0 = (int64_t)tile * CHORDAL_TILE, r0 = t0 + 64 * wave, row = r0 + lane;
    // a wavefront's LDS row is its own and its pass count is that of its own run: no wavefront waits for another's hub row
    const int64_t s_beg = A.rp[min(r0, n)], s_end = A.rp[min(r0 + 64, n)];
    const int64_t my_lo = row < n ? A.rp[row] : s_end, my_hi = row < n ? A.rp[row + 1] : s_end;
    Cx acc = cx(0.0, 0.0);
    for (int64_t base = s_beg; base < s_end; base += 64) {
      const int64_t s = base + lane;
      if (s < s_end) prod[wave][lane] = cx_mul(A.val[s], v[A.col[s]]);
      wave_lds_sync();
      const int64_t lo = max(my_lo, base), hi = min(my_hi, base + 64);
      for (int64_t k = lo; k < hi; ++k) acc = cx_add(acc, prod[wave][k - base]);
      wave_lds_sync();
    }
    double term = 0.0;
    if (row < n) {
      const Cx vi = v[row], qi = cx_add(cx_scale(A.d[row], vi), acc);
      q[row] = qi;
      term = cx_dot(vi, qi);
    }
    const double sum = block_sum_bcast(term, red);
    if (threadIdx.x == 0) A.part[(int64_t)CH_PQ * A.n_part + tile] = sum;
  }
}

// x, r, z per row and the tile's partials of r.z and |r|^2 (rows that are not identity rows), shared by the two kernels below
__device__ __forceinline__ void chordal_tile_partials(const ChordalArgs& A, int tile, double rz, double rr, double* red) {
  const double s0 = block_sum_bcast(rz, red), s1 = block_sum_bcast(rr, red);
  if (threadIdx.x == 0) {
    A.part[(int64_t)CH_RZ * A.n_part + tile] = s0;
    A.part[(int64_t)CH_RR * A.n_part + tile] = s1;
  }
}

template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_chordal_residual(ChordalArgs A) {
  __shared__ double red[8];
  for (int tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
    const int64_t i = (int64_t)tile * CHORDAL_TILE + threadIdx.x;
    double rz = 0.0, rr = 0.0, bb = 0.0;
    if (i < A.n) {
      const Cx bi = A.b[i], ri = cx_sub(bi, A.q[i]), zi = cx_scale(1.0 / A.d[i], ri);
      A.r[i] = ri;
      A.z[i] = zi;
      A.p[i] = zi;
      rz = cx_dot(ri, zi);
      if (!A.ident[i]) {
        rr = cx_dot(ri, ri);
        bb = cx_dot(bi, bi);
      }
    }
    chordal_tile_partials(A, tile, rz, rr, red);
    const double s2 = block_sum_bcast(bb, red);
    if (threadIdx.x == 0) A.part[(int64_t)CH_BB * A.n_part + tile] = s2;
  }
}

template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_chordal_begin(ChordalArgs A) {
  __shared__ double red[8];
  const double rz = sum_partials_bcast(A.part + (int64_t)CH_RZ * A.n_part, A.n_tiles, red);
  const double rr = sum_partials_bcast(A.part + (int64_t)CH_RR * A.n_part, A.n_tiles, red);
  const double bb = sum_partials_bcast(A.part + (int64_t)CH_BB * A.n_part, A.n_tiles, red);
  if (threadIdx.x == 0) {
    ChordalState& S = *A.st;
    S.rz[0] = rz;
    S.rz[1] = 0.0;
    S.rr = rr;
    S.bb = bb;
    S.done[0] = chordal_converged(rr, bb, A.rtol) ? 1 : 0;
    S.done[1] = 0;
    S.iters = 0;
  }
}

template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_chordal_update(ChordalArgs A) {
  __shared__ double red[8];
  if (A.st->done[A.it & 1]) return;
  const double pq = sum_partials_bcast(A.part + (int64_t)CH_PQ * A.n_part, A.n_tiles, red);
  const double alpha = chordal_ratio(A.st->rz[A.it & 1], pq);
  for (int tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
    const int64_t i = (int64_t)tile * CHORDAL_TILE + threadIdx.x;
    double rz = 0.0, rr = 0.0;
    if (i < A.n) {
      A.x[i] = cx_add(A.x[i], cx_scale(alpha, A.p[i]));
      const Cx ri = cx_sub(A.r[i], cx_scale(alpha, A.q[i])), zi = cx_scale(1.0 / A.d[i], ri);
      A.r[i] = ri;
      A.z[i] = zi;
      rz = cx_dot(ri, zi);
      if (!A.ident[i]) rr = cx_dot(ri, ri);
    }
    chordal_tile_partials(A, tile, rz, rr, red);
  }
}

template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_chordal_direction(ChordalArgs A) {
  __shared__ double red[8];
  const int cur = A.it & 1, nxt = cur ^ 1;
  if (A.st->done[cur]) {
    if (blockIdx.x == 0 && threadIdx.x == 0) A.st->done[nxt] = 1;
    return;
  }
  const double rz_new = sum_partials_bcast(A.part + (int64_t)CH_RZ * A.n_part, A.n_tiles, red);
  const double rr = sum_partials_bcast(A.part + (int64_t)CH_RR * A.n_part, A.n_tiles, red);
  const double beta = chordal_ratio(rz_new, A.st->rz[cur]);
  for (int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * WG) A.p[i] = cx_add(A.z[i], cx_scale(beta, A.p[i]));
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ChordalState& S = *A.st;
    const bool conv = chordal_converged(rr, S.bb, A.rtol);
    S.rz[nxt] = rz_new;
    S.rr = rr;
    S.iters = A.it + 1;
    S.done[nxt] = conv ? 1 : 0;
  }
}

template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_chordal_headings(ChordalArgs A) {
  __shared__ double red[8];
  const ChordalStart S = chordal_start(A.g, A.c0);
  for (int tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
    const int64_t i = (int64_t)tile * CHORDAL_TILE + threadIdx.x;
    double deg = 0.0, neg_mag = -INFINITY;
    if (i < A.n) {
      const ChordalHeading H = chordal_heading(A.g, S, (int32_t)i, A.x[i], A.mag_min);
      A.theta[i] = H.theta;
      A.zh[i] = H.zh;
      deg = (double)H.degenerate;
      if (!A.g.constant((int32_t)i)) neg_mag = H.mag == H.mag ? -H.mag : INFINITY;   // (a NaN magnitude wins the maximum: k_chordal_fold)
    }
    const double s0 = block_sum_bcast(deg, red), s1 = block_max_bcast(neg_mag, red);
    if (threadIdx.x == 0) {
      A.part[(int64_t)CH_DEG * A.n_part + tile] = s0;
      A.part[(int64_t)CH_MAG * A.n_part + tile] = s1;
    }
  }
}

template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_chordal_finish(ChordalArgs A) {
  __shared__ double red[8];
  for (int c = blockIdx.x; c < A.n_part; c += gridDim.x) {
    const int64_t k = (int64_t)c * WG + threadIdx.x;
    double bad = 0.0, fresh = 0.0;
    if (c < A.n_tiles && k < A.n) {
      double* o = A.poses_out + 3 * k;
      if (A.g.constant((int32_t)k)) A.g.pose((int32_t)k, o, o + 1, o + 2);
      else {
        const Cx t = A.x[k];
        o[0] = t.re;
        o[1] = t.im;
        o[2] = A.theta[k];
      }
      bad = coarsen_finite3(o[0], o[1], o[2]) ? 0.0 : 1.0;
    }
    if (c < A.n_chunks && k < A.n_edges) {
      const int32_t a = A.ea[k], b = A.eb[k];
      double mx, my, mt, rxy, rth;
      A.g.meas((int32_t)k, &mx, &my, &mt);
      // (the positions of the constant poses are x0: what stage T's x holds on their identity rows)
      chordal_residual(mx, my, mt, A.theta[a], A.theta[b], A.zh[a], A.x[a], A.x[b], &rxy, &rth);
      A.res_out[2 * k] = rxy;
      A.res_out[2 * k + 1] = rth;
      if (A.reject && chordal_rejects(A.u[k], A.eloc[k] < 0, rxy, rth, A.reject_xy, A.reject_th)) {
        A.u[k] = 0.0;
        A.rej[k] = 1;
        fresh = 1.0;
      }
    }
    const double s0 = block_sum_bcast(bad, red), s1 = block_sum_bcast(fresh, red);
    if (threadIdx.x == 0) {
      A.part[(int64_t)CH_BAD * A.n_part + c] = s0;
      A.part[(int64_t)CH_NEW * A.n_part + c] = s1;
    }
  }
}

// ONE workgroup: slots l, l + 256, ... in order, then the lane tree
template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_chordal_fold(ChordalArgs A) {
  __shared__ double red[8];
  const double deg = sum_partials_bcast(A.part + (int64_t)CH_DEG * A.n_part, A.n_tiles, red);
  const double bad = sum_partials_bcast(A.part + (int64_t)CH_BAD * A.n_part, A.n_part, red);
  const double fresh = sum_partials_bcast(A.part + (int64_t)CH_NEW * A.n_part, A.n_part, red);
  double m = -INFINITY;
  for (int i = threadIdx.x; i < A.n_tiles; i += WG) m = fmax(m, A.part[(int64_t)CH_MAG * A.n_part + i]);
  m = block_max_bcast(m, red);
  if (threadIdx.x == 0) {
    A.st->n_degenerate = deg;
    A.st->min_mag = m == INFINITY ? NAN : -m;   // (some |z| is NaN: so is the minimum, as in chordal_serial)
    A.st->n_new = fresh;
    A.st->n_bad = bad;
  }
}

template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_chordal_commit(ChordalArgs A) {
  for (int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * WG) {
    if (A.g.constant((int32_t)i)) continue;
    double* p = A.h_poses + 3 * (int64_t)(A.g.perm ? A.g.perm[i] : (int32_t)i);
    p[0] = A.poses_out[3 * i];
    p[1] = A.poses_out[3 * i + 1];
    p[2] = A.poses_out[3 * i + 2];
  }
}

template <int PGO_UNIT_ = 0>
__global__ __launch_bounds__(WG) void k_chordal_apply(ChordalArgs A) {
  for (int64_t e = (int64_t)blockIdx.x * WG + threadIdx.x; e < A.n_edges; e += (int64_t)gridDim.x * WG)
    if (A.rej[e]) A.w[A.g.loc[e]] = 0.0;
}

}  // namespace dev
}  // namespace pgo
