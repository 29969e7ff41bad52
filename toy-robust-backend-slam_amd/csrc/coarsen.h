#pragma once
// Coarsening a pose graph along its odometry chain and spreading a coarse solution back (include/pgo.h, "hierarchical
// initialisation"): ONE statement of the SE(2) operations, of the transport of a measurement and of the
// prolongation blend, evaluated on the host by pgo_coarsen_plan / pgo_prolong_eval (serially, in the caller's order), on the
// device by the kernels of coarsen.hip.h (fixed trees), and by tests/native/coarsen_main.cpp.  Plain doubles only.
//   stride S, key pose k = fine pose kS, K = ceil(N / S)
//   Z_i      the chain edge of the pair (i, i + 1) as a motion from i to i + 1 (the inverse of an edge stored as (i + 1, i))
//   C_i      = Z_{kS} o ... o Z_{i-1}                    kS < i < (k + 1)S;  C_{kS} = (0, 0, 0)
//   Cend_k   = C_{(k+1)S-1} o Z_{(k+1)S-1}               k < K - 1: the motion from key pose k to key pose k + 1
//   edge (a, b, m)  ->  (a / S, b / S, C_a o m o C_b^-1)  theta wrapped
//   P_i      = blend of F_i = X_k o C_i and B_i = X_{k+1} o Cend_k^-1 o C_i at t = (i - kS) / S
// Angles are wrapped (atan2(sin, cos)) in two places only: theta of a coarse measurement, and B_th - F_th in the blend.
// Information matrices ("with information": pgo_coarsen_info_plan, pgo_coarsen_info) ride along as covariances.  A pair
// (A, Sigma_A) couples a motion with the covariance of ADDITIVE noise on its own triple (x, y, theta) -- what a g2o information
// matrix is the inverse of --, six doubles in the order of info6 (xx, xy, xt, yy, yt, tt):
//   identity   (se2_identity(), 0)
//   compose    (A, Sigma_A) o (B, Sigma_B) = (A o B, F Sigma_A F' + G Sigma_B G')
//                F = [1 0 -(s_A B.x + c_A B.y); 0 1 c_A B.x - s_A B.y; 0 0 1]      G = [c_A -s_A 0; s_A c_A 0; 0 0 1]
//   inverse    B = A^-1: (B, H Sigma_A H'),  H = [-c_A -s_A B.y; s_A -c_A -B.x; 0 0 -1]
// first order in the noise.  The covariance of a product is sum_i D_i Sigma_i D_i' with D_i the derivative of the whole product
// in its i-th factor: the chain rule makes it independent of the association, so trees and serial folds agree up to rounding.
//   Z_i      as a pair: (m, Omega^-1) of the chain edge, the pair inverted for an edge stored as (i + 1, i); Omega = I without
//            information matrices.  C_i and Cend_k follow as above, as pairs.
//   composite edge k:  information = Sigma(Cend_k)^-1
//   edge (a, b, m, Omega):  pair(C_a) o (m, Omega^-1) o pair(C_b)^-1 -- a and b lie in different segments, so the three factors
//            are independent; its mean, wrapped, is the measurement above; information = the inverse of its covariance
// Omega^-1 and Sigma^-1 go through gate_chol3: factor, invert the factor, multiply.  Wrapping an angle does not touch Sigma.
// Coarse edges that share chain motions (the edges that leave or enter one segment, and that segment's composite) are
// CORRELATED; the coarse graph treats them as independent.  That correlation is ignored.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "gate.h"

namespace pgo {

// an element of SE(2) with its rotation carried as (c, s) beside the angle: compositions multiply the rotations and add the
// angles, so a chain of them takes one sincos per input and none per composition
struct Se2 {
  double x, y, th, c, s;
};
__host__ __device__ __forceinline__ Se2 se2_identity() { return Se2{0.0, 0.0, 0.0, 1.0, 0.0}; }
__host__ __device__ __forceinline__ Se2 se2_make(double x, double y, double th) {
  Se2 A;
  A.x = x;
  A.y = y;
  A.th = th;
  sincos(th, &A.s, &A.c);
  return A;
}
// A o B: first A, then B in A's frame.  se2_compose(se2_identity(), B) is B bitwise
__host__ __device__ __forceinline__ Se2 se2_compose(const Se2& A, const Se2& B) {
  Se2 R;
  R.x = A.x + (A.c * B.x - A.s * B.y);
  R.y = A.y + (A.s * B.x + A.c * B.y);
  R.th = A.th + B.th;
  R.c = A.c * B.c - A.s * B.s;
  R.s = A.s * B.c + A.c * B.s;
  return R;
}
__host__ __device__ __forceinline__ Se2 se2_inverse(const Se2& A) {
  Se2 R;
  R.x = -(A.c * A.x + A.s * A.y);
  R.y = -(A.c * A.y - A.s * A.x);
  R.th = -A.th;
  R.c = A.c;
  R.s = -A.s;
  return R;
}
// the angle wrapped into (-pi, pi] through atan2(sin, cos)
__host__ __device__ __forceinline__ double coarsen_wrap(double a) {
  double s, c;
  sincos(a, &s, &c);
  return atan2(s, c);
}
__host__ __device__ __forceinline__ bool coarsen_finite3(double x, double y, double th) {
  return std::isfinite(x) && std::isfinite(y) && std::isfinite(th);
}

// Z_i of a chain edge stored with the measurement (mx, my, mt): as it stands, or inverted when the edge runs (i + 1, i)
__host__ __device__ __forceinline__ Se2 coarsen_chain_motion(double mx, double my, double mt, bool reversed) {
  const Se2 M = se2_make(mx, my, mt);
  return reversed ? se2_inverse(M) : M;
}

// the transport of the measurement m of an edge (a, b) to the key poses of its ends: C_a o m o C_b^-1, theta wrapped
__host__ __device__ __forceinline__ void coarsen_transport(const Se2& Ca, double mx, double my, double mt, const Se2& Cb, double out[3]) {
  const Se2 R = se2_compose(se2_compose(Ca, se2_make(mx, my, mt)), se2_inverse(Cb));
  out[0] = R.x;
  out[1] = R.y;
  out[2] = coarsen_wrap(R.th);
}

// ------------------------------------------------------------------ pairs (motion, covariance)
struct Se2Cov {
  Se2 m;
  double v[6];   // xx xy xt yy yt tt
};
__host__ __device__ __forceinline__ Se2Cov pair_identity() { return Se2Cov{se2_identity(), {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}}; }
// R Sigma R' with R = [c -s 0; s c 0; 0 0 1]; (c, s) = (1, 0) returns Sigma bitwise
__host__ __device__ __forceinline__ void cov_rotate(const double v[6], double c, double s, double o[6]) {
  const double t1 = c * v[0] - s * v[1], t2 = c * v[1] - s * v[3];
  const double t3 = s * v[0] + c * v[1], t4 = s * v[1] + c * v[3];
  o[0] = t1 * c - t2 * s;
  o[1] = t1 * s + t2 * c;
  o[2] = c * v[2] - s * v[4];
  o[3] = t3 * s + t4 * c;
  o[4] = s * v[2] + c * v[4];
  o[5] = v[5];
}
// F Sigma F' with F = [1 0 fx; 0 1 fy; 0 0 1]
__host__ __device__ __forceinline__ void cov_shear(const double v[6], double fx, double fy, double o[6]) {
  o[0] = v[0] + (2.0 * fx * v[2] + fx * fx * v[5]);
  o[1] = v[1] + (fx * v[4] + fy * v[2] + fx * fy * v[5]);
  o[2] = v[2] + fx * v[5];
  o[3] = v[3] + (2.0 * fy * v[4] + fy * fy * v[5]);
  o[4] = v[4] + fy * v[5];
  o[5] = v[5];
}
// the mean is se2_compose itself; composing with pair_identity() on either side leaves a pair bitwise unchanged (a covariance
// holds no negative zero: cov_invert does not produce one, and a sum with +0 removes it)
__host__ __device__ __forceinline__ Se2Cov pair_compose(const Se2Cov& A, const Se2Cov& B) {
  Se2Cov R;
  R.m = se2_compose(A.m, B.m);
  double f[6], g[6];
  cov_shear(A.v, -(A.m.s * B.m.x + A.m.c * B.m.y), A.m.c * B.m.x - A.m.s * B.m.y, f);
  cov_rotate(B.v, A.m.c, A.m.s, g);
#pragma unroll
  for (int i = 0; i < 6; ++i) R.v[i] = f[i] + g[i];
  return R;
}
// the mean is se2_inverse itself.  H = -F G with G the rotation by -theta_A and F the shear by (-B.y, B.x): H Sigma H' = F G Sigma G' F'
__host__ __device__ __forceinline__ Se2Cov pair_inverse(const Se2Cov& A) {
  Se2Cov R;
  R.m = se2_inverse(A.m);
  double g[6];
  cov_rotate(A.v, A.m.c, -A.m.s, g);
  cov_shear(g, -R.m.y, R.m.x, R.v);
  return R;
}
// o = w^-1 of a symmetric 3x3 (either way between information and covariance): w = L L' (gate_chol3), M = L^-1, o = M' M.
// false -- o is not written -- when w is not finite and positive definite.  o holds no negative zero.
__host__ __device__ __forceinline__ bool cov_invert(const double w[6], double o[6]) {
  double l[6];
  if (!gate_chol3(w, l)) return false;
  const double m0 = 1.0 / l[0], m2 = 1.0 / l[2], m5 = 1.0 / l[5];
  const double m1 = -(l[1] * m0) / l[2];
  const double m3 = -(l[3] * m0 + l[4] * m1) / l[5];
  const double m4 = -(l[4] * m2) / l[5];
  o[0] = m0 * m0 + m1 * m1 + m3 * m3 + 0.0;
  o[1] = m1 * m2 + m3 * m4 + 0.0;
  o[2] = m3 * m5 + 0.0;
  o[3] = m2 * m2 + m4 * m4 + 0.0;
  o[4] = m4 * m5 + 0.0;
  o[5] = m5 * m5;
  return true;
}
// Z_i as a pair.  w: the chain edge's information, read only when has_info (else the identity).  false: it is not finite and
// positive definite.  (The kernels pass w in registers: a pointer that may be null would put it in scratch.)
__host__ __device__ __forceinline__ bool coarsen_chain_pair_w(double mx, double my, double mt, bool has_info, const double w[6], bool reversed,
                                                              Se2Cov* out) {
  Se2Cov P;
  P.m = se2_make(mx, my, mt);
  if (has_info) {
    if (!cov_invert(w, P.v)) return false;
  } else {
    P.v[0] = P.v[3] = P.v[5] = 1.0;
    P.v[1] = P.v[2] = P.v[4] = 0.0;
  }
  *out = reversed ? pair_inverse(P) : P;
  return true;
}
// info6: the information, nullptr = the identity
__host__ __device__ __forceinline__ bool coarsen_chain_pair(double mx, double my, double mt, const double* info6, bool reversed, Se2Cov* out) {
  double w[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (info6)
    for (int i = 0; i < 6; ++i) w[i] = info6[i];
  return coarsen_chain_pair_w(mx, my, mt, info6 != nullptr, w, reversed, out);
}
// the transport with information: pair(C_a) o (m, Omega^-1) o pair(C_b)^-1.  meas = coarsen_transport's; cov its covariance.
// false: Omega is not finite and positive definite (nothing written)
__host__ __device__ __forceinline__ bool coarsen_transport_pair_w(const Se2Cov& Ca, double mx, double my, double mt, bool has_info,
                                                                  const double w[6], const Se2Cov& Cb, double meas[3], double cov[6]) {
  Se2Cov M;
  if (!coarsen_chain_pair_w(mx, my, mt, has_info, w, false, &M)) return false;
  const Se2Cov R = pair_compose(pair_compose(Ca, M), pair_inverse(Cb));
  meas[0] = R.m.x;
  meas[1] = R.m.y;
  meas[2] = coarsen_wrap(R.m.th);
#pragma unroll
  for (int i = 0; i < 6; ++i) cov[i] = R.v[i];
  return true;
}
__host__ __device__ __forceinline__ bool coarsen_transport_pair(const Se2Cov& Ca, double mx, double my, double mt, const double* info6,
                                                                const Se2Cov& Cb, double meas[3], double cov[6]) {
  double w[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (info6)
    for (int i = 0; i < 6; ++i) w[i] = info6[i];
  return coarsen_transport_pair_w(Ca, mx, my, mt, info6 != nullptr, w, Cb, meas, cov);
}
// the information of a coarse covariance; NaN throughout when the covariance has lost positive definiteness to rounding
__host__ __device__ __forceinline__ void coarsen_info_of(const double cov[6], double info[6]) {
  if (!cov_invert(cov, info))
    for (int i = 0; i < 6; ++i) info[i] = NAN;
}

// The prolongation of fine pose i = kS + r (0 <= r < S): Xk the coarse pose of its segment, Xn the next one (read only when
// has_next), Ci its composite, Cend the segment's closing composite (read only when has_next).  r = 0 returns Xk bitwise.
__host__ __device__ __forceinline__ void coarsen_prolong_pose(const double Xk[3], const double* Xn, const double Ci[3], const double* Cend,
                                                              bool has_next, int32_t r, int32_t S, double out[3]) {
  if (r == 0) {
    out[0] = Xk[0];
    out[1] = Xk[1];
    out[2] = Xk[2];
    return;
  }
  const Se2 C = se2_make(Ci[0], Ci[1], Ci[2]);
  const Se2 F = se2_compose(se2_make(Xk[0], Xk[1], Xk[2]), C);
  if (!has_next) {   // the last segment: forward only
    out[0] = F.x;
    out[1] = F.y;
    out[2] = F.th;
    return;
  }
  const Se2 B = se2_compose(se2_compose(se2_make(Xn[0], Xn[1], Xn[2]), se2_inverse(se2_make(Cend[0], Cend[1], Cend[2]))), C);
  const double t = (double)r / (double)S;
  out[0] = (1.0 - t) * F.x + t * B.x;
  out[1] = (1.0 - t) * F.y + t * B.y;
  out[2] = F.th + t * coarsen_wrap(B.th - F.th);
}

// ------------------------------------------------------------------ the serial evaluation (host)
// chain[i] (i < N - 1): the edge joining poses i and i + 1.  C: N x 3, Cend: (K - 1) x 3 (either may be nullptr: then the other
// is still filled; composites are folded left to right, C_{i+1} = C_i o Z_i).
inline void coarsen_composites_serial(int64_t N, int64_t S, const int32_t* chain, const int32_t* ia, const double* meas, double* C,
                                      double* Cend) {
  Se2 A = se2_identity();
  for (int64_t i = 0; i < N; ++i) {
    if (i % S == 0) A = se2_identity();
    if (C) {
      C[3 * i] = A.x;
      C[3 * i + 1] = A.y;
      C[3 * i + 2] = A.th;
    }
    if (i + 1 < N) {
      const int64_t e = chain[i];
      A = se2_compose(A, coarsen_chain_motion(meas[3 * e], meas[3 * e + 1], meas[3 * e + 2], ia[e] != (int32_t)i));
      if ((i + 1) % S == 0 && Cend) {
        const int64_t k = i / S;
        Cend[3 * k] = A.x;
        Cend[3 * k + 1] = A.y;
        Cend[3 * k + 2] = A.th;
      }
    }
  }
}

// the same with information: info6 (E x 6) or nullptr = the identity; Ccov: N x 6, Cendcov: (K - 1) x 6 (either pair of outputs
// may be nullptr).  The means are coarsen_composites_serial's bitwise.  Returns the chain edge whose information is not finite
// and positive definite (the first along the chain; the outputs are unfinished then), or -1.
inline int64_t coarsen_composites_info_serial(int64_t N, int64_t S, const int32_t* chain, const int32_t* ia, const double* meas,
                                              const double* info6, double* C, double* Cend, double* Ccov, double* Cendcov) {
  Se2Cov A = pair_identity();
  for (int64_t i = 0; i < N; ++i) {
    if (i % S == 0) A = pair_identity();
    if (C) {
      C[3 * i] = A.m.x;
      C[3 * i + 1] = A.m.y;
      C[3 * i + 2] = A.m.th;
    }
    if (Ccov)
      for (int c = 0; c < 6; ++c) Ccov[6 * i + c] = A.v[c];
    if (i + 1 < N) {
      const int64_t e = chain[i];
      Se2Cov Z;
      if (!coarsen_chain_pair(meas[3 * e], meas[3 * e + 1], meas[3 * e + 2], info6 ? info6 + 6 * e : nullptr, ia[e] != (int32_t)i, &Z)) return e;
      A = pair_compose(A, Z);
      if ((i + 1) % S == 0) {
        const int64_t k = i / S;
        if (Cend) {
          Cend[3 * k] = A.m.x;
          Cend[3 * k + 1] = A.m.y;
          Cend[3 * k + 2] = A.m.th;
        }
        if (Cendcov)
          for (int c = 0; c < 6; ++c) Cendcov[6 * k + c] = A.v[c];
      }
    }
  }
  return -1;
}

// coarse poses X (K x 3) -> fine poses out (N x 3)
inline void coarsen_prolong_serial(int64_t N, int64_t S, const double* C, const double* Cend, const double* X, double* out) {
  const int64_t K = (N + S - 1) / S;
  for (int64_t i = 0; i < N; ++i) {
    const int64_t k = i / S;
    const bool has_next = k < K - 1;
    coarsen_prolong_pose(X + 3 * k, has_next ? X + 3 * (k + 1) : nullptr, C + 3 * i, has_next ? Cend + 3 * k : nullptr, has_next,
                         (int32_t)(i - k * S), (int32_t)S, out + 3 * i);
  }
}

}  // namespace pgo
