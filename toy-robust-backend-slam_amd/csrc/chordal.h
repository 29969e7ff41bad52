#pragma once
// An estimate-free linear start (include/pgo.h, "chordal initialisation"): ONE statement of the two
// Hermitian systems, of the Jacobi-PCG that solves them and of the per-pose and per-edge results, evaluated on the host by
// pgo_chordal_plan (serially, in the caller's order), on the device by the kernels of chordal.hip.h (fixed trees), and by
// tests/native/chordal_main.cpp.  Plain doubles only; the SE(2) operations are those of coarsen.h, the trajectory is
// loop_support.h's.  Caller's numbering throughout.
//   u_e        the weight of edge e = (a, b, m): 0 for an inactive edge, an edge with a == b and an edge a round rejected
//   C          the constant poses; c0 the smallest of them
//   X_i        = (P_c0 o T_c0^-1) o T_i: the odometry trajectory moved rigidly onto c0
//   x0_i       stage R: exp(i theta_c) on C, (X_i.c, X_i.s) elsewhere;  stage T: x_c + i y_c on C, X_i.x + i X_i.y elsewhere
//   stage R    min sum_e u_e |z_b - phi_e z_a|^2,  phi_e = exp(i m_theta);  zh_i = z_i / |z_i|, theta_i = atan2(Im z_i, Re z_i)
//   stage T    min sum_e u_e |t_b - t_a - zh_a (m_x + i m_y)|^2
//   H x = b    one row per pose; row i owns the slots [rp[i], rp[i + 1]), sorted by edge index, a slot = (col, edge | HEAD),
//              HEAD set when i is the edge's b.  Slot value: -u phi (HEAD) or -u conj(phi), phi = 1 in stage T; slot term of b:
//              +g (HEAD) or -g with g = u zh_a (m_x + i m_y), 0 in stage R.  d_i = the sum of u over the row's slots, in slot
//              order.  A slot whose column is constant moves -value x0_col into b_i and holds 0.  A row of C, and a row with
//              d_i = 0 (no positive-weight edge), is an identity row: d = 1, b = x0, every slot 0 -- such a pose keeps x0.
//   PCG        z = r / d;  |r| and |b| over the rows that are not identity rows;  stop at |r|^2 <= rtol^2 |b|^2
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "loop_support.h"
#include "pgo.h"

namespace pgo {

struct alignas(16) Cx {
  double re, im;
};
__host__ __device__ __forceinline__ Cx cx(double re, double im) { return Cx{re, im}; }
__host__ __device__ __forceinline__ Cx cx_add(const Cx& a, const Cx& b) { return Cx{a.re + b.re, a.im + b.im}; }
__host__ __device__ __forceinline__ Cx cx_sub(const Cx& a, const Cx& b) { return Cx{a.re - b.re, a.im - b.im}; }
__host__ __device__ __forceinline__ Cx cx_mul(const Cx& a, const Cx& b) { return Cx{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__host__ __device__ __forceinline__ Cx cx_scale(double s, const Cx& a) { return Cx{s * a.re, s * a.im}; }
__host__ __device__ __forceinline__ double cx_dot(const Cx& a, const Cx& b) { return a.re * b.re + a.im * b.im; }   // Re(a^H b)

constexpr int32_t CHORDAL_HEAD = INT32_MIN;   // the orientation of a slot, in the sign bit of its edge
__host__ __device__ __forceinline__ int32_t chordal_slot_edge(int32_t se) { return se & INT32_MAX; }
__host__ __device__ __forceinline__ bool chordal_slot_head(int32_t se) { return se < 0; }

// what a stage reads of the graph; the host passes arrays in the caller's order, the device the handle's planes behind its tables
//   G.meas(e, &mx, &my, &mt)   the measurement of caller's edge e
//   G.pose(i, &x, &y, &th)     the current pose of caller's pose i (read on C only)
//   G.constant(i)              i is in C
//   G.traj(i)                  T_i (Se2)
struct ChordalStart {   // P_c0 o T_c0^-1
  Se2 G;
};
template <class Graph>
__host__ __device__ __forceinline__ ChordalStart chordal_start(const Graph& g, int32_t c0) {
  double x, y, th;
  g.pose(c0, &x, &y, &th);
  return ChordalStart{se2_compose(se2_make(x, y, th), se2_inverse(g.traj(c0)))};
}
// X_i
template <class Graph>
__host__ __device__ __forceinline__ Se2 chordal_moved(const Graph& g, const ChordalStart& S, int32_t i) {
  return se2_compose(S.G, g.traj(i));
}
template <class Graph>
__host__ __device__ __forceinline__ Cx chordal_x0(const Graph& g, const ChordalStart& S, int stage, int32_t i) {
  if (g.constant(i)) {
    double x, y, th;
    g.pose(i, &x, &y, &th);
    if (stage) return cx(x, y);
    double s, c;
    sincos(th, &s, &c);
    return cx(c, s);
  }
  const Se2 X = chordal_moved(g, S, i);
  return stage ? cx(X.x, X.y) : cx(X.c, X.s);
}

// Row i of a stage: the slot values, d_i, b_i, x0_i and whether the row is an identity row.  u: the weights, caller's order;
// zh: stage T only.
template <class Graph>
__host__ __device__ __forceinline__ void chordal_row(const Graph& g, const ChordalStart& S, int stage, int32_t i, const int32_t* rp, const int32_t* col,
                                                     const int32_t* se, const double* u, const Cx* zh, Cx* val, double* d_out, Cx* b_out, Cx* x_out,
                                                     uint8_t* ident_out) {
  const Cx xi = chordal_x0(g, S, stage, i);
  const bool is_const = g.constant(i);
  double d = 0.0;
  Cx b = cx(0.0, 0.0);
  for (int64_t s = rp[i]; s < rp[i + 1]; ++s) {
    val[s] = cx(0.0, 0.0);
    if (is_const) continue;
    const int32_t e = chordal_slot_edge(se[s]), j = col[s];
    const bool head = chordal_slot_head(se[s]);
    const double w = u[e];
    if (!(w > 0.0)) continue;
    double mx, my, mt;
    g.meas(e, &mx, &my, &mt);
    Cx v;
    if (stage) {
      v = cx(-w, 0.0);
      const Cx gt = cx_scale(w, cx_mul(zh[head ? j : i], cx(mx, my)));
      b = head ? cx_add(b, gt) : cx_sub(b, gt);
    } else {
      double sn, cs;
      sincos(mt, &sn, &cs);
      v = cx(-w * cs, head ? -w * sn : w * sn);
    }
    d += w;
    if (g.constant(j)) b = cx_sub(b, cx_mul(v, chordal_x0(g, S, stage, j)));
    else val[s] = v;
  }
  const bool ident = is_const || !(d > 0.0);
  *d_out = ident ? 1.0 : d;
  *b_out = ident ? xi : b;
  *x_out = xi;
  *ident_out = ident ? 1 : 0;
}

// (H p)_i = d_i p_i + the slot products, summed in slot order from 0
__host__ __device__ __forceinline__ Cx chordal_row_product(int32_t i, const int32_t* rp, const int32_t* col, const Cx* val, const double* d, const Cx* p) {
  Cx acc = cx(0.0, 0.0);
  for (int64_t s = rp[i]; s < rp[i + 1]; ++s) acc = cx_add(acc, cx_mul(val[s], p[col[s]]));
  return cx_add(cx_scale(d[i], p[i]), acc);
}

// the PCG scalars, one place for the host loop and the device kernels: a zero denominator means r = 0 (exact convergence)
__host__ __device__ __forceinline__ double chordal_ratio(double num, double den) { return den != 0.0 ? num / den : 0.0; }
__host__ __device__ __forceinline__ bool chordal_converged(double rr, double bb, double rtol) { return rr <= rtol * rtol * bb; }

// stage R's result on pose i: theta, zh, |z| and whether the pose is degenerate.  An identity row keeps x0 (|z| = 1 there).
struct ChordalHeading {
  double theta, mag;
  Cx zh;
  int32_t degenerate;
};
template <class Graph>
__host__ __device__ __forceinline__ ChordalHeading chordal_heading(const Graph& g, const ChordalStart& S, int32_t i, const Cx& z, double mag_min) {
  ChordalHeading R;
  R.degenerate = 0;
  if (g.constant(i)) {
    double x, y, th, s, c;
    g.pose(i, &x, &y, &th);
    sincos(th, &s, &c);
    R.theta = th;
    R.zh = cx(c, s);
    R.mag = 1.0;
    return R;
  }
  R.mag = sqrt(z.re * z.re + z.im * z.im);
  if (!(R.mag >= mag_min)) {   // (a NaN counts)
    const Se2 X = chordal_moved(g, S, i);
    R.theta = X.th;
    R.zh = cx(X.c, X.s);
    R.degenerate = 1;
    return R;
  }
  R.theta = atan2(z.im, z.re);
  R.zh = cx(z.re / R.mag, z.im / R.mag);
  return R;
}

// the report of edge e = (a, b, m)
__host__ __device__ __forceinline__ void chordal_residual(double mx, double my, double mt, double th_a, double th_b, const Cx& zh_a, const Cx& t_a,
                                                          const Cx& t_b, double* res_xy, double* res_th) {
  const Cx r = cx_sub(cx_sub(t_b, t_a), cx_mul(zh_a, cx(mx, my)));
  *res_xy = sqrt(r.re * r.re + r.im * r.im);
  *res_th = fabs(coarsen_wrap(th_b - th_a - mt));
}
// is the edge rejected for the next round?  (a NaN residual rejects)
__host__ __device__ __forceinline__ bool chordal_rejects(double u, bool chain, double res_xy, double res_th, double reject_xy, double reject_th) {
  return u > 0.0 && !chain && !(res_xy <= reject_xy && res_th <= reject_th);
}

// ------------------------------------------------------------------ the tables and the checks (host)
// rows sorted by (pose, edge index): a counting sort over the endpoints, stable in the edge index.  An edge with a == b has no slot.
inline void chordal_slots(int64_t N, int64_t E, const int32_t* ia, const int32_t* ib, std::vector<int32_t>* rp, std::vector<int32_t>* col,
                          std::vector<int32_t>* se) {
  rp->assign((size_t)(N + 1), 0);
  for (int64_t e = 0; e < E; ++e)
    if (ia[e] != ib[e]) {
      ++(*rp)[(size_t)ia[e] + 1];
      ++(*rp)[(size_t)ib[e] + 1];
    }
  for (int64_t i = 0; i < N; ++i) (*rp)[i + 1] += (*rp)[i];
  col->assign((size_t)(*rp)[N], 0);
  se->assign((size_t)(*rp)[N], 0);
  std::vector<int32_t> next(rp->begin(), rp->end() - 1);
  for (int64_t e = 0; e < E; ++e) {
    if (ia[e] == ib[e]) continue;
    const int32_t sa = next[ia[e]]++, sb = next[ib[e]]++;
    (*col)[sa] = ib[e];
    (*se)[sa] = (int32_t)e;
    (*col)[sb] = ia[e];
    (*se)[sb] = (int32_t)e | CHORDAL_HEAD;
  }
}

// a pose of a component that has a positive-weight edge and no constant pose (the smallest pose of the first such component
// in the order of the poses), or -1
inline int32_t chordal_unanchored(int64_t N, int64_t E, const int32_t* ia, const int32_t* ib, const double* u, const uint8_t* constant) {
  std::vector<int32_t> root((size_t)N);
  for (int64_t i = 0; i < N; ++i) root[i] = (int32_t)i;
  auto find = [&](int32_t i) {
    while (root[i] != i) i = root[i] = root[root[i]];
    return i;
  };
  std::vector<uint8_t> has_edge((size_t)N, 0), has_const((size_t)N, 0);
  for (int64_t e = 0; e < E; ++e)
    if (u[e] > 0.0 && ia[e] != ib[e]) {
      const int32_t a = find(ia[e]), b = find(ib[e]);
      if (a != b) root[a > b ? a : b] = a > b ? b : a;   // (the root is the component's smallest pose)
    }
  for (int64_t e = 0; e < E; ++e)
    if (u[e] > 0.0 && ia[e] != ib[e]) has_edge[find(ia[e])] = 1;
  for (int64_t i = 0; i < N; ++i)
    if (constant[i]) has_const[find((int32_t)i)] = 1;
  for (int64_t i = 0; i < N; ++i)
    if (root[i] == (int32_t)i && has_edge[i] && !has_const[i]) return (int32_t)i;
  return -1;
}

// ------------------------------------------------------------------ the serial evaluation (host)
struct ChordalHostGraph {
  const int32_t *ia, *ib;
  const double *m, *poses, *T;   // m: E x 3, T: N x SUPPORT_POSE
  const uint8_t* is_const;
  void meas(int32_t e, double* mx, double* my, double* mt) const {
    *mx = m[3 * (int64_t)e];
    *my = m[3 * (int64_t)e + 1];
    *mt = m[3 * (int64_t)e + 2];
  }
  void pose(int32_t i, double* x, double* y, double* th) const {
    *x = poses[3 * (int64_t)i];
    *y = poses[3 * (int64_t)i + 1];
    *th = poses[3 * (int64_t)i + 2];
  }
  bool constant(int32_t i) const { return is_const[i] != 0; }
  Se2 traj(int32_t i) const { return support_load(T + (int64_t)SUPPORT_POSE * i); }
};

struct ChordalPcgResult {
  int32_t iters, converged;
  double rel;   // |r| / |b| (|r| where b = 0)
};
// Jacobi-PCG on the assembled rows, x in (x0) and out.  The convergence test is made after every iteration.
inline ChordalPcgResult chordal_pcg_serial(int64_t N, const int32_t* rp, const int32_t* col, const Cx* val, const double* d, const Cx* b,
                                           const uint8_t* ident, double rtol, int32_t max_iters, Cx* x) {
  std::vector<Cx> r((size_t)N), z((size_t)N), p((size_t)N), q((size_t)N);
  double rz = 0.0, rr = 0.0, bb = 0.0;
  for (int64_t i = 0; i < N; ++i) {
    r[i] = cx_sub(b[i], chordal_row_product((int32_t)i, rp, col, val, d, x));
    z[i] = cx_scale(1.0 / d[i], r[i]);
    p[i] = z[i];
    rz += cx_dot(r[i], z[i]);
    if (!ident[i]) {
      rr += cx_dot(r[i], r[i]);
      bb += cx_dot(b[i], b[i]);
    }
  }
  ChordalPcgResult R{0, chordal_converged(rr, bb, rtol) ? 1 : 0, 0.0};
  while (!R.converged && R.iters < max_iters) {
    double pq = 0.0;
    for (int64_t i = 0; i < N; ++i) {
      q[i] = chordal_row_product((int32_t)i, rp, col, val, d, p.data());
      pq += cx_dot(p[i], q[i]);
    }
    const double alpha = chordal_ratio(rz, pq);
    double rz_new = 0.0;
    rr = 0.0;
    for (int64_t i = 0; i < N; ++i) {
      x[i] = cx_add(x[i], cx_scale(alpha, p[i]));
      r[i] = cx_sub(r[i], cx_scale(alpha, q[i]));
      z[i] = cx_scale(1.0 / d[i], r[i]);
      rz_new += cx_dot(r[i], z[i]);
      if (!ident[i]) rr += cx_dot(r[i], r[i]);
    }
    const double beta = chordal_ratio(rz_new, rz);
    for (int64_t i = 0; i < N; ++i) p[i] = cx_add(z[i], cx_scale(beta, p[i]));
    rz = rz_new;
    ++R.iters;
    R.converged = chordal_converged(rr, bb, rtol) ? 1 : 0;
  }
  R.rel = bb > 0.0 ? sqrt(rr / bb) : sqrt(rr);
  return R;
}

inline bool chordal_options_ok(const pgo_chordal_options* o) {
  return o && std::isfinite(o->rtol) && o->rtol > 0.0 && o->max_iters >= 1 && o->check_every >= 1 && std::isfinite(o->mag_min) && o->mag_min >= 0.0 &&
         o->rounds >= 0 && o->rounds <= PGO_CHORDAL_MAX_ROUNDS && !std::isnan(o->reject_xy) && o->reject_xy > 0.0 && !std::isnan(o->reject_th) &&
         o->reject_th > 0.0;
}

// The whole statement on arrays.  u (E, in: the starting weights; out: 0 where a round rejected), is_const (N), chain (N - 1:
// the chain edge of every pair) and T (N x SUPPORT_POSE) are the caller's; poses_out N x 3, res_out E x 2 (xy, theta).
// Returns PGO_OK, or PGO_ERR_UNSUPPORTED with *where = a pose of a component without a constant pose, or PGO_ERR_NUMERIC with
// *where = -1: the solution is not finite.
inline int chordal_serial(int64_t N, int64_t E, const int32_t* ia, const int32_t* ib, const double* meas, const double* poses, const uint8_t* is_const,
                          const int32_t* chain, const double* T, const pgo_chordal_options* o, double* u, double* poses_out, double* res_out,
                          pgo_chordal_summary* sum, int32_t* where) {
  ChordalHostGraph g{ia, ib, meas, poses, T, is_const};
  std::vector<int32_t> rp, col, se;
  chordal_slots(N, E, ia, ib, &rp, &col, &se);
  std::vector<uint8_t> is_chain((size_t)E, 0), ident((size_t)N);
  for (int64_t i = 0; i + 1 < N; ++i) is_chain[chain[i]] = 1;
  int32_t c0 = -1;
  for (int64_t i = 0; i < N && c0 < 0; ++i)
    if (is_const[i]) c0 = (int32_t)i;
  std::vector<Cx> val(col.size() + 1), b((size_t)N), x((size_t)N), zh((size_t)N);
  std::vector<double> d((size_t)N), theta((size_t)N);
  memset(sum, 0, sizeof *sum);
  if (c0 < 0) {
    *where = 0;
    return PGO_ERR_UNSUPPORTED;
  }
  for (int32_t round = 0; round <= o->rounds; ++round) {
    *where = chordal_unanchored(N, E, ia, ib, u, is_const);
    if (*where >= 0) return PGO_ERR_UNSUPPORTED;
    const ChordalStart S = chordal_start(g, c0);   // (c0 >= 0: N >= 2 poses on a chain with a positive weight somewhere, or every row is an identity row)
    pgo_chordal_solve& R = sum->solve[round];
    R.min_mag = INFINITY;
    for (int stage = 0; stage < 2; ++stage) {
      for (int64_t i = 0; i < N; ++i)
        chordal_row(g, S, stage, (int32_t)i, rp.data(), col.data(), se.data(), u, zh.data(), val.data(), &d[i], &b[i], &x[i], &ident[i]);
      const ChordalPcgResult P = chordal_pcg_serial(N, rp.data(), col.data(), val.data(), d.data(), b.data(), ident.data(), o->rtol, o->max_iters, x.data());
      R.iters[stage] = P.iters;
      R.converged[stage] = P.converged;
      R.rel_residual[stage] = P.rel;
      if (stage == 0)
        for (int64_t i = 0; i < N; ++i) {
          const ChordalHeading Hd = chordal_heading(g, S, (int32_t)i, x[i], o->mag_min);
          theta[i] = Hd.theta;
          zh[i] = Hd.zh;
          R.n_degenerate += Hd.degenerate;
          if (!is_const[i] && R.min_mag == R.min_mag && !(Hd.mag >= R.min_mag)) R.min_mag = Hd.mag;   // (a NaN |z| makes the minimum NaN, and it stays)
        }
    }
    int32_t n_new = 0;
    bool finite = true;
    for (int64_t i = 0; i < N; ++i) {
      if (is_const[i]) memcpy(poses_out + 3 * i, poses + 3 * i, 24);
      else {
        poses_out[3 * i] = x[i].re;
        poses_out[3 * i + 1] = x[i].im;
        poses_out[3 * i + 2] = theta[i];
      }
      finite = finite && coarsen_finite3(poses_out[3 * i], poses_out[3 * i + 1], poses_out[3 * i + 2]);
    }
    for (int64_t e = 0; e < E; ++e) {
      const int32_t a = ia[e], bb = ib[e];
      double rxy, rth;
      chordal_residual(meas[3 * e], meas[3 * e + 1], meas[3 * e + 2], poses_out[3 * (int64_t)a + 2], poses_out[3 * (int64_t)bb + 2], zh[a],
                       cx(poses_out[3 * (int64_t)a], poses_out[3 * (int64_t)a + 1]), cx(poses_out[3 * (int64_t)bb], poses_out[3 * (int64_t)bb + 1]), &rxy, &rth);
      res_out[2 * e] = rxy;
      res_out[2 * e + 1] = rth;
      if (round < o->rounds && chordal_rejects(u[e], is_chain[e] != 0, rxy, rth, o->reject_xy, o->reject_th)) {
        u[e] = 0.0;
        ++n_new;
      }
    }
    R.n_rejected = n_new;
    sum->n_solves = round + 1;
    sum->n_rejected += n_new;
    sum->n_degenerate = R.n_degenerate;
    sum->min_mag = R.min_mag;
    if (!finite) {
      *where = -1;
      return PGO_ERR_NUMERIC;
    }
    if (n_new == 0) break;
  }
  return PGO_OK;
}

}  // namespace pgo
