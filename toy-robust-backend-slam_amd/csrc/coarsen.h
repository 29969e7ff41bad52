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
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

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
