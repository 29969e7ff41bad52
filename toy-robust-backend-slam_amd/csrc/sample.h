#pragma once
// The noise of pgo_posterior_sample (include/pgo.h, "posterior sampling"), stated once for the host and the device: a
// counter-based generator, so that the standard normal triple of an edge (or a prior) in a sample is a pure function of
//     (seed, stream, index, sample)
// and of nothing else.  What that gives:
//   - the noise of an edge does not depend on the internal pose or edge ordering, on the grid, on the pass width, or on which
//     other samples a call draws: `index` is the edge's index in the CALLER's edge order (the prior's position in the order
//     given to pgo_set_priors), `sample` the global sample number;
//   - duplicate edges (the same endpoints, the same measurement) have different indices and so independent noise;
//   - both endpoints of an edge regenerate its triple where they consume it: no E x 3 x m noise panel is ever stored.
//
// Generator: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), multipliers
// 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85.
//   key     = (seed low 32 bits, seed high 32 bits)
//   counter = (index, word, sample, stream)        stream: 0 = edges, 1 = priors;  word: 0 or 1
// From the output words (o0, o1, o2, o3) of one counter:
//   u0 = (((uint64) o1 << 21 | o0 >> 11) + 0.5) 2^-53,   u1 likewise from (o3, o2)          both in (0, 1)
//   z0 = sqrt(-2 ln u0) cos(2 pi u1),  z1 = sqrt(-2 ln u0) sin(2 pi u1)                     (Box-Muller)
// and a triple is (z0, z1) of word 0 followed by z0 of word 1.
// (In double precision k + 0.5 is a tie for k >= 2^52 and the one value k = 2^53 - 1 would round up to u = 1: the tie is taken
// downwards there, u = 1 - 2^-53, which is as close to the exact 1 - 2^-54 and keeps u inside (0, 1).)
// The device's log / sin / cos need not match libm bitwise: the triples agree to ~1e-15.
//
// __host__ __device__, no HIP types: tests/native/sample_main.cpp compiles this header with a plain C++ compiler.
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PGO_SAMPLE_HD __host__ __device__ __forceinline__
#else
#define PGO_SAMPLE_HD inline
#endif

namespace pgo {

constexpr uint32_t SAMPLE_STREAM_EDGE = 0, SAMPLE_STREAM_PRIOR = 1;

// out = Philox4x32-10(counter, key)
PGO_SAMPLE_HD void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0;
    c1 = n1;
    c2 = n2;
    c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// the uniform variate of the word pair (lo, hi): ((hi << 21 | lo >> 11) + 0.5) 2^-53, inside (0, 1)
PGO_SAMPLE_HD double sample_uniform(uint32_t lo, uint32_t hi) {
  const uint64_t k = ((uint64_t)hi << 21) | (uint64_t)(lo >> 11);
  const double u = ((double)k + 0.5) * 0x1p-53;
  return u < 1.0 ? u : 0x1.fffffffffffffp-1;
}

// the two uniforms of one counter's output
PGO_SAMPLE_HD void sample_uniform_pair(uint64_t seed, uint32_t stream, uint32_t index, uint32_t sample, uint32_t word, double* u0, double* u1) {
  const uint32_t ctr[4] = {index, word, sample, stream}, key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t o[4];
  philox4x32_10(ctr, key, o);
  *u0 = sample_uniform(o[0], o[1]);
  *u1 = sample_uniform(o[2], o[3]);
}

// the standard normal triple of (seed, stream, index, sample)
PGO_SAMPLE_HD void sample_triple(uint64_t seed, uint32_t stream, uint32_t index, uint32_t sample, double z[3]) {
  const double two_pi = 6.283185307179586476925286766559;
  double u0, u1;
  sample_uniform_pair(seed, stream, index, sample, 0u, &u0, &u1);
  const double r0 = sqrt(-2.0 * log(u0)), a0 = two_pi * u1;
#if defined(__HIP_DEVICE_COMPILE__)
  double sn, cs;   // (one argument reduction for both)
  __builtin_assume(a0 >= 0.0 && a0 < 6.5);
  sincos(a0, &sn, &cs);
  z[0] = r0 * cs;
  z[1] = r0 * sn;
#else
  z[0] = r0 * cos(a0);
  z[1] = r0 * sin(a0);
#endif
  sample_uniform_pair(seed, stream, index, sample, 1u, &u0, &u1);
  const double a1 = two_pi * u1;
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_assume(a1 >= 0.0 && a1 < 6.5);
#endif
  z[2] = sqrt(-2.0 * log(u0)) * cos(a1);
}

// R (lower triangular, row-major 3x3) with R R' = L for a symmetric positive SEMI-definite L = (l00 l01 l02 l11 l12 l22): the
// Cholesky factorisation in which a pivot that is not positive (after the first: not above 1e-14 of its diagonal entry, the
// rounding of the eliminations before it) leaves a zero column -- diag(a, a, 0) is legal.
PGO_SAMPLE_HD void sample_chol3_psd(const double l[6], double R[9]) {
  for (int i = 0; i < 9; ++i) R[i] = 0.0;
  const double d0 = l[0];
  if (d0 > 0.0) {
    R[0] = sqrt(d0);
    R[3] = l[1] / R[0];
    R[6] = l[2] / R[0];
  }
  const double d1 = l[3] - R[3] * R[3];
  if (d1 > 1e-14 * l[3]) {
    R[4] = sqrt(d1);
    R[7] = (l[4] - R[6] * R[3]) / R[4];
  }
  const double d2 = l[5] - R[6] * R[6] - R[7] * R[7];
  if (d2 > 1e-14 * l[5]) R[8] = sqrt(d2);
}

}  // namespace pgo
