// The joint gate's elimination of csrc/gate.h on the host (gate_joint_serial: what pgo_gate_joint_evaluate runs, the statements
// k_gate_joint_step runs on the device), compiled by g++ plainly and with AddressSanitizer + UndefinedBehaviorSanitizer.
//     gate_joint_main IN OUT
// IN:  "n chi2_gate min_info_gain", then per candidate "status force r0 r1 r2 I11 I12 I13 I22 I23 I33", then the 3n rows of P.
// OUT: per candidate "accepted status chi2_cond info_gain_cond r_cond[3] P_cond[9]", then "n_accepted chi2_joint info_gain_joint",
//      17 digits.  Exit status 3 + the candidate when a pivot is not positive definite.
// Built and run by tests/test_gate_joint_native.py.
#include <cstdio>
#include <vector>

#include "gate.h"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* in = fopen(argv[1], "r");
  if (!in) return 1;
  int n;
  double chi2_gate, min_gain;
  if (fscanf(in, "%d %lf %lf", &n, &chi2_gate, &min_gain) != 3 || n < 0 || n > PGO_GATE_JOINT_MAX) return 1;
  const size_t W = 3 * (size_t)n;
  std::vector<int32_t> status(n);
  std::vector<int8_t> force(n);
  std::vector<double> r(W), info(6 * (size_t)n), P(W * W), B(3 * W + 1);
  for (int k = 0; k < n; ++k) {
    int st, f;
    if (fscanf(in, "%d %d", &st, &f) != 2) return 1;
    status[k] = st;
    force[k] = (int8_t)f;
    for (int i = 0; i < 3; ++i)
      if (fscanf(in, "%lf", &r[3 * k + i]) != 1) return 1;
    for (int i = 0; i < 6; ++i)
      if (fscanf(in, "%lf", &info[6 * k + i]) != 1) return 1;
  }
  for (size_t i = 0; i < W * W; ++i)
    if (fscanf(in, "%lf", &P[i]) != 1) return 1;
  fclose(in);
  std::vector<pgo_gate_joint_result> joint(n);
  pgo_gate_joint_summary sum;
  int bad = -1;
  const int st = pgo::gate_joint_serial(n, r.data(), P.data(), info.data(), status.data(), force.data(), chi2_gate, min_gain, joint.data(), B.data(), &bad);
  if (st != pgo::GATE_OK) {
    printf("gate joint: the pivot of candidate %d is not positive definite\n", bad);
    return 3 + bad;
  }
  pgo::gate_joint_summarise(n, joint.data(), &sum);
  FILE* out = fopen(argv[2], "w");
  if (!out) return 1;
  for (int k = 0; k < n; ++k) {
    const pgo_gate_joint_result& o = joint[k];
    fprintf(out, "%d %d %.17g %.17g", o.accepted, o.status, o.chi2_cond, o.info_gain_cond);
    for (int i = 0; i < 3; ++i) fprintf(out, " %.17g", o.r_cond[i]);
    for (int i = 0; i < 9; ++i) fprintf(out, " %.17g", o.P_cond[i]);
    fprintf(out, "\n");
  }
  fprintf(out, "%d %.17g %.17g\n", sum.n_accepted, sum.chi2_joint, sum.info_gain_joint);
  if (fclose(out) != 0) return 1;
  printf("gate joint ok: %d candidates, %d accepted\n", n, sum.n_accepted);
  return 0;
}
