// The noise of pgo_posterior_sample (csrc/sample.h) on the host, compiled by g++ with AddressSanitizer +
// UndefinedBehaviorSanitizer:
//     sample_main check            the Philox4x32-10 known answers, u in (0, 1) at the all-zero and all-one words, the triple's
//                                  definition, the semi-definite 3x3 Cholesky; prints "sample ok"
//     sample_main triples IN OUT   IN: "n" then n lines "seed stream index sample"; OUT: the triple of each, 17 digits
// Built and run by tests/test_sample_native.py.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "sample.h"

static int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAILED line %d: %s\n", __LINE__, #cond);           \
      ++failures;                                                \
    }                                                            \
  } while (0)

static void known(const uint32_t c[4], const uint32_t k[2], const uint32_t want[4]) {
  uint32_t o[4];
  pgo::philox4x32_10(c, k, o);
  for (int i = 0; i < 4; ++i) CHECK(o[i] == want[i]);
}

static int check() {
  {   // Salmon et al.'s known answers
    const uint32_t c0[4] = {0, 0, 0, 0}, k0[2] = {0, 0}, w0[4] = {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u};
    known(c0, k0, w0);
    const uint32_t f = 0xffffffffu, c1[4] = {f, f, f, f}, k1[2] = {f, f}, w1[4] = {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu};
    known(c1, k1, w1);
    const uint32_t c2[4] = {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, k2[2] = {0xa4093822u, 0x299f31d0u},
                   w2[4] = {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u};
    known(c2, k2, w2);
  }
  {   // the uniforms stay inside (0, 1) at both ends, and are what the formula says in between
    const double lo = pgo::sample_uniform(0u, 0u), hi = pgo::sample_uniform(0xffffffffu, 0xffffffffu);
    CHECK(lo > 0.0 && lo < 1.0 && lo == 0x1p-54);
    CHECK(hi > 0.0 && hi < 1.0 && hi == 0x1.fffffffffffffp-1);
    CHECK(pgo::sample_uniform(0x800u, 0u) == 1.5 * 0x1p-53);                // k = 1
    CHECK(pgo::sample_uniform(0u, 1u) == ((double)(1u << 21) + 0.5) * 0x1p-53);   // the high word starts at bit 21
    CHECK(pgo::sample_uniform(0x7ffu, 0u) == lo);                           // the low 11 bits of the low word are not used
    CHECK(isfinite(sqrt(-2.0 * log(lo))) && sqrt(-2.0 * log(hi)) >= 0.0);
  }
  {   // the triple: (z0, z1) of word 0 and z0 of word 1 of the counter (index, word, sample, stream), key = the seed's halves
    const uint64_t seed = 0x0123456789abcdefull;
    const uint32_t stream = 1, index = 4242, sample = 77;
    double z[3];
    pgo::sample_triple(seed, stream, index, sample, z);
    const double two_pi = 6.283185307179586476925286766559;
    double want[3];
    for (uint32_t word = 0; word < 2; ++word) {
      const uint32_t c[4] = {index, word, sample, stream}, k[2] = {0x89abcdefu, 0x01234567u};
      uint32_t o[4];
      pgo::philox4x32_10(c, k, o);
      const double u0 = (double)(((uint64_t)o[1] << 21) | (o[0] >> 11)) * 0x1p-53 + 0x1p-54;
      const double u1 = (double)(((uint64_t)o[3] << 21) | (o[2] >> 11)) * 0x1p-53 + 0x1p-54;
      const double r = sqrt(-2.0 * log(u0));
      if (word == 0) {
        want[0] = r * cos(two_pi * u1);
        want[1] = r * sin(two_pi * u1);
      } else {
        want[2] = r * cos(two_pi * u1);
      }
    }
    for (int i = 0; i < 3; ++i) CHECK(fabs(z[i] - want[i]) <= 1e-15 * (1.0 + fabs(want[i])));
    // another sample, another index, the other stream, another seed: another triple
    double y[3];
    pgo::sample_triple(seed, stream, index, sample + 1, y);
    CHECK(y[0] != z[0] && y[1] != z[1] && y[2] != z[2]);
    pgo::sample_triple(seed, stream, index + 1, sample, y);
    CHECK(y[0] != z[0] && y[1] != z[1] && y[2] != z[2]);
    pgo::sample_triple(seed, 0, index, sample, y);
    CHECK(y[0] != z[0] && y[1] != z[1] && y[2] != z[2]);
    pgo::sample_triple(seed + (1ull << 32), stream, index, sample, y);
    CHECK(y[0] != z[0] && y[1] != z[1] && y[2] != z[2]);
  }
  {   // R R' = L, a zero pivot a zero column
    const double full[6] = {4.0, 2.0, -1.0, 5.0, 0.5, 3.0}, flat[6] = {2.5, 0.0, 0.0, 2.5, 0.0, 0.0}, zero[6] = {0, 0, 0, 0, 0, 0},
                 rank1[6] = {1.0, 2.0, 3.0, 4.0, 6.0, 9.0};
    const double* all[4] = {full, flat, zero, rank1};
    for (const double* l : all) {
      double R[9];
      pgo::sample_chol3_psd(l, R);
      const double L[9] = {l[0], l[1], l[2], l[1], l[3], l[4], l[2], l[4], l[5]};
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
          double s = 0.0;
          for (int k = 0; k < 3; ++k) s += R[3 * a + k] * R[3 * b + k];
          CHECK(fabs(s - L[3 * a + b]) <= 1e-14 * (1.0 + fabs(L[3 * a + b])));
          if (b > a) CHECK(R[3 * a + b] == 0.0);
          CHECK(isfinite(R[3 * a + b]));
        }
    }
    double R[9];
    pgo::sample_chol3_psd(flat, R);
    CHECK(R[6] == 0.0 && R[7] == 0.0 && R[8] == 0.0);
  }
  if (failures) return 1;
  printf("sample ok\n");
  return 0;
}

static int triples(const char* in_path, const char* out_path) {
  FILE* in = fopen(in_path, "r");
  FILE* out = fopen(out_path, "w");
  if (!in || !out) return 1;
  long n = 0;
  if (fscanf(in, "%ld", &n) != 1) return 1;
  for (long i = 0; i < n; ++i) {
    uint64_t seed;
    uint32_t stream, index, sample;
    if (fscanf(in, "%" SCNu64 " %" SCNu32 " %" SCNu32 " %" SCNu32, &seed, &stream, &index, &sample) != 4) return 1;
    double z[3];
    pgo::sample_triple(seed, stream, index, sample, z);
    fprintf(out, "%.17g %.17g %.17g\n", z[0], z[1], z[2]);
  }
  fclose(in);
  if (fclose(out) != 0) return 1;
  printf("sample triples ok: %ld\n", n);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "check")) return check();
  if (argc == 4 && !strcmp(argv[1], "triples")) return triples(argv[2], argv[3]);
  fprintf(stderr, "usage: sample_main check | triples IN OUT\n");
  return 2;
}
