#pragma once
// Trajectory error of an estimate against a reference (include/pgo.h, "scoring"): ONE statement of the per-pose and per-pair
// formulas and of the closing arithmetic, evaluated on the host by pgo_trajectory_error_eval (serially, in the caller's order),
// on the device by the kernels of score.hip.h (fixed trees), and by tests/native/traj_error_main.cpp.  Plain doubles only.
//   ATE  e_i = R(phi) p_i + t - q_i                                 (Horn's alignment without scale, or phi = 0, t = 0)
//   RPE  E_i = (Q_i^-1 Q_{i+d})^-1 (P_i^-1 P_{i+d})                 (Sturm et al.; invariant to the alignment)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "pgo.h"

namespace pgo {

// the angle wrapped into (-pi, pi] through atan2(sin, cos)
__host__ __device__ __forceinline__ double traj_wrap(double a) {
  double s, c;
  sincos(a, &s, &c);
  return atan2(s, c);
}

__host__ __device__ __forceinline__ bool traj_pose_finite(const double* p) {
  return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]);
}

// A compensated sum, value s + c (TwoSum, branch-free): the centroids and the centred moments of the alignment are summed this
// way on the host and on the device, so that phi and t are good to a few ulp whatever the number of poses and the order of the
// terms -- a per-pose error inherits every error of the transform, multiplied by |p|.  (The error sums themselves are plain.)
struct TrajAcc {
  double s, c;
};
__host__ __device__ __forceinline__ void traj_acc_merge(TrajAcc& A, double s2, double c2) {
  const double t = A.s + s2, bb = t - A.s;
  const double err = (A.s - (t - bb)) + (s2 - bb);
  A.c = (A.c + c2) + err;
  A.s = t;
}
__host__ __device__ __forceinline__ void traj_acc_add(TrajAcc& A, double x) { traj_acc_merge(A, x, 0.0); }
__host__ __device__ __forceinline__ double traj_acc_value(const TrajAcc& A) { return A.s + A.c; }

// the rigid transform applied to the estimate
struct TrajAlign {
  double phi, c, s, tx, ty;
};
__host__ __device__ __forceinline__ TrajAlign traj_identity() { return TrajAlign{0.0, 1.0, 0.0, 0.0, 0.0}; }

// one pose's terms of the centred moments: a += (p - pbar).(q - qbar), b += (p - pbar) x (q - qbar)
__host__ __device__ __forceinline__ void traj_moment_terms(double px, double py, double qx, double qy, double pbx, double pby,
                                                           double qbx, double qby, double& a, double& b) {
  const double ux = px - pbx, uy = py - pby, vx = qx - qbx, vy = qy - qby;
  a = ux * vx + uy * vy;
  b = ux * vy - uy * vx;
}
// phi = atan2(b, a) (0 when a = b = 0), t = qbar - R(phi) pbar
__host__ __device__ __forceinline__ TrajAlign traj_align_from_moments(double a, double b, double pbx, double pby, double qbx,
                                                                      double qby) {
  TrajAlign T;
  T.phi = (a == 0.0 && b == 0.0) ? 0.0 : atan2(b, a);
  sincos(T.phi, &T.s, &T.c);
  T.tx = qbx - (T.c * pbx - T.s * pby);
  T.ty = qby - (T.s * pbx + T.c * pby);
  return T;
}

// ATE of one pose: trans2 = |R(phi) p + t - q|^2, rot = |wrap(theta_p + phi - theta_q)|
__host__ __device__ __forceinline__ void traj_pose_error(const TrajAlign& T, double px, double py, double pt, double qx, double qy,
                                                         double qt, double& trans2, double& rot) {
  const double ex = (T.c * px - T.s * py) + T.tx - qx, ey = (T.s * px + T.c * py) + T.ty - qy;
  trans2 = ex * ex + ey * ey;
  rot = fabs(traj_wrap(pt + T.phi - qt));
}

// RPE of the pair (i, j = i + d): trans2 = |trans(E)|^2, rot = |angle(E)| of E = (Q_i^-1 Q_j)^-1 (P_i^-1 P_j)
__host__ __device__ __forceinline__ void traj_pair_error(double pix, double piy, double pit, double pjx, double pjy, double pjt,
                                                         double qix, double qiy, double qit, double qjx, double qjy, double qjt,
                                                         double& trans2, double& rot) {
  double sp, cp, sq, cq;
  sincos(pit, &sp, &cp);
  sincos(qit, &sq, &cq);
  const double dpx = pjx - pix, dpy = pjy - piy, dqx = qjx - qix, dqy = qjy - qiy;
  const double ax = cp * dpx + sp * dpy, ay = -sp * dpx + cp * dpy;   // trans(P_i^-1 P_j)
  const double bx = cq * dqx + sq * dqy, by = -sq * dqx + cq * dqy;   // trans(Q_i^-1 Q_j)
  const double dq = qjt - qit;                                        // angle(Q_i^-1 Q_j)
  double sd, cd;
  sincos(dq, &sd, &cd);
  const double ux = ax - bx, uy = ay - by;
  const double ex = cd * ux + sd * uy, ey = -sd * ux + cd * uy;       // R(dq)' (a - b)
  trans2 = ex * ex + ey * ey;
  rot = fabs(traj_wrap((pjt - pit) - dq));
}

// the sums and maxima of a call, as the host loop or the device fold hands them over (a maximum of nothing: -1, index -1)
struct TrajSums {
  double n, t2, t1, r2;        // counted poses; sums of trans^2, trans, rot^2
  double np, pt2, pr2;         // counted pairs; sums of the pairs' trans^2 and rot^2
  double tmax, rmax, ptmax, prmax;
  int32_t tmax_i, ptmax_i;   // the poses of tmax and ptmax (the pair (i, i + d) is named by i)
};
// the result record.  The maxima of the translations are carried squared (the square root is monotonic: the same pose wins)
__host__ __device__ __forceinline__ void traj_finish(const TrajSums& S, const TrajAlign& T, pgo_traj_error* out) {
  out->n_poses = (int32_t)S.n;
  out->n_pairs = (int32_t)S.np;
  out->align_x = T.tx;
  out->align_y = T.ty;
  out->align_phi = T.phi;
  const bool any = S.n > 0.0, anyp = S.np > 0.0;
  out->ate_max_pose = any ? S.tmax_i : -1;
  out->ate_rmse = any ? sqrt(S.t2 / S.n) : 0.0;
  out->ate_mean = any ? S.t1 / S.n : 0.0;
  out->ate_max = any ? sqrt(S.tmax) : 0.0;
  out->rot_rmse = any ? sqrt(S.r2 / S.n) : 0.0;
  out->rot_max = any ? S.rmax : 0.0;
  out->rpe_max_pose = anyp ? S.ptmax_i : -1;
  out->rpe_trans_rmse = anyp ? sqrt(S.pt2 / S.np) : 0.0;
  out->rpe_trans_max = anyp ? sqrt(S.ptmax) : 0.0;
  out->rpe_rot_rmse = anyp ? sqrt(S.pr2 / S.np) : 0.0;
  out->rpe_rot_max = anyp ? S.prmax : 0.0;
}

// the running maximum with its index: a later value wins only when it is larger, or equal at a smaller index
__host__ __device__ __forceinline__ void traj_take_max(double& v, int32_t& i, double v2, int32_t i2) {
  if (v2 > v || (v2 == v && i2 < i)) {
    v = v2;
    i = i2;
  }
}

// ------------------------------------------------------------------ the serial evaluation (host)
// est, ref: n x 3 (x, y, theta); mask (or nullptr): non-zero = the pose counts.  Returns -1, or the smallest counted pose that is
// not finite in either trajectory (nothing is written then).  per_pose (or nullptr): n x 2 = (trans, |rot|), 0 where not counted.
inline int64_t traj_error_serial(int64_t n, const double* est, const double* ref, const uint8_t* mask, int align, int64_t delta,
                                 pgo_traj_error* out, double* per_pose) {
  auto counted = [&](int64_t i) { return !mask || mask[i]; };
  for (int64_t i = 0; i < n; ++i)
    if (counted(i) && !(traj_pose_finite(est + 3 * i) && traj_pose_finite(ref + 3 * i))) return i;
  TrajAlign T = traj_identity();
  if (align) {
    double cnt = 0.0;
    TrajAcc spx = {0.0, 0.0}, spy = {0.0, 0.0}, sqx = {0.0, 0.0}, sqy = {0.0, 0.0};
    for (int64_t i = 0; i < n; ++i)
      if (counted(i)) {
        cnt += 1.0;
        traj_acc_add(spx, est[3 * i]);
        traj_acc_add(spy, est[3 * i + 1]);
        traj_acc_add(sqx, ref[3 * i]);
        traj_acc_add(sqy, ref[3 * i + 1]);
      }
    if (cnt > 0.0) {
      const double pbx = traj_acc_value(spx) / cnt, pby = traj_acc_value(spy) / cnt, qbx = traj_acc_value(sqx) / cnt,
                   qby = traj_acc_value(sqy) / cnt;
      TrajAcc a = {0.0, 0.0}, b = {0.0, 0.0};
      for (int64_t i = 0; i < n; ++i)
        if (counted(i)) {
          double ai, bi;
          traj_moment_terms(est[3 * i], est[3 * i + 1], ref[3 * i], ref[3 * i + 1], pbx, pby, qbx, qby, ai, bi);
          traj_acc_add(a, ai);
          traj_acc_add(b, bi);
        }
      T = traj_align_from_moments(traj_acc_value(a), traj_acc_value(b), pbx, pby, qbx, qby);
    }
  }
  TrajSums S = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1.0, -1.0, -1.0, -1.0, -1, -1};
  for (int64_t i = 0; i < n; ++i) {
    double t2 = 0.0, rot = 0.0;
    if (counted(i)) {
      traj_pose_error(T, est[3 * i], est[3 * i + 1], est[3 * i + 2], ref[3 * i], ref[3 * i + 1], ref[3 * i + 2], t2, rot);
      S.n += 1.0;
      S.t2 += t2;
      S.t1 += sqrt(t2);
      S.r2 += rot * rot;
      traj_take_max(S.tmax, S.tmax_i, t2, (int32_t)i);
      S.rmax = fmax(S.rmax, rot);
      const int64_t j = i + delta;
      if (delta > 0 && j < n && counted(j)) {
        double p2, prot;
        traj_pair_error(est[3 * i], est[3 * i + 1], est[3 * i + 2], est[3 * j], est[3 * j + 1], est[3 * j + 2], ref[3 * i],
                        ref[3 * i + 1], ref[3 * i + 2], ref[3 * j], ref[3 * j + 1], ref[3 * j + 2], p2, prot);
        S.np += 1.0;
        S.pt2 += p2;
        S.pr2 += prot * prot;
        traj_take_max(S.ptmax, S.ptmax_i, p2, (int32_t)i);
        S.prmax = fmax(S.prmax, prot);
      }
    }
    if (per_pose) {
      per_pose[2 * i] = sqrt(t2);
      per_pose[2 * i + 1] = rot;
    }
  }
  traj_finish(S, T, out);
  return -1;
}

}  // namespace pgo
