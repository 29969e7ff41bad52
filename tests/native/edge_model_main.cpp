// The SE(2) edge model of csrc/edge_model.h on the host: the statement the kernels (k_edge_eval, k_edge_chi2, k_gate_eval,
// k_window_solve) evaluate, compiled by g++ (under AddressSanitizer + UndefinedBehaviorSanitizer by the CPU test).
//     edge_model_main IN OUT
// IN:  one edge per line:  x1 y1 t1  x2 y2 t2  dx dy dth  flags phi        (flags bit 0: DCS)
// OUT: one line per edge, 42 numbers at 17 digits:  r (3) J (18, 3 x 6 row-major) of the plain model with heading
//      asin(sin delta), then r (3) J (18) after the DCS step (equal to the plain ones when bit 0 is clear).
// Built and run by tests/test_edge_model_host.py and tests/test_gpu_edge_model.py.
#include <cstdio>

#include "edge_model.h"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* in = fopen(argv[1], "r");
  FILE* out = fopen(argv[2], "w");
  if (!in || !out) return 1;
  double v[9], phi;
  unsigned fl;
  long n = 0;
  while (fscanf(in, "%lf %lf %lf %lf %lf %lf %lf %lf %lf %u %lf", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], &v[8], &fl,
                &phi) == 11) {
    double ex, ey, sind, J[18];
    pgo::edge_plain<true>(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], ex, ey, sind, J);
    double et = asin(sind);
    // the residual-only instantiation is the same statement
    double ex0, ey0, sind0;
    pgo::edge_plain<false>(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], ex0, ey0, sind0, nullptr);
    if (ex0 != ex || ey0 != ey || sind0 != sind) return 3;
    fprintf(out, "%.17g %.17g %.17g", ex, ey, et);
    for (int c = 0; c < 18; ++c) fprintf(out, " %.17g", J[c]);
    if (fl & 1u) {
      double cx = ex, cy = ey, ct = et;
      pgo::edge_dcs<false>(phi, cx, cy, ct, nullptr);
      pgo::edge_dcs<true>(phi, ex, ey, et, J);
      if (cx != ex || cy != ey || ct != et) return 3;
    }
    fprintf(out, " %.17g %.17g %.17g", ex, ey, et);
    for (int c = 0; c < 18; ++c) fprintf(out, " %.17g", J[c]);
    fprintf(out, "\n");
    ++n;
  }
  fclose(in);
  if (fclose(out) != 0) return 1;
  printf("edge model ok: %ld edges\n", n);
  return 0;
}
