// The trajectory error of csrc/traj_error.h on the host: the statement pgo_trajectory_error_eval runs and the kernels of
// score.hip.h evaluate, compiled by g++ with AddressSanitizer + UndefinedBehaviorSanitizer.
//     traj_error_main IN OUT
// IN:  "n align rpe_delta has_mask", then n lines "ex ey et qx qy qt mask" (17 digits).
// OUT: the fields of pgo_traj_error in the order of the struct, one per line (17 digits), then n lines "trans rot".
// Built and run by tests/test_score_native.py.
#include <cstdio>
#include <vector>

#include "traj_error.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "r");
  if (!in) return 1;
  long n;
  int align, delta, has_mask;
  if (fscanf(in, "%ld %d %d %d", &n, &align, &delta, &has_mask) != 4 || n < 1) return 1;
  std::vector<double> est((size_t)3 * n), ref((size_t)3 * n), per((size_t)2 * n);
  std::vector<uint8_t> mask((size_t)n);
  for (long i = 0; i < n; ++i) {
    int m;
    if (fscanf(in, "%lf %lf %lf %lf %lf %lf %d", &est[3 * i], &est[3 * i + 1], &est[3 * i + 2], &ref[3 * i], &ref[3 * i + 1],
               &ref[3 * i + 2], &m) != 7)
      return 1;
    mask[i] = (uint8_t)m;
  }
  fclose(in);
  pgo_traj_error e;
  const int64_t bad = pgo::traj_error_serial(n, est.data(), ref.data(), has_mask ? mask.data() : nullptr, align, delta, &e, per.data());
  if (bad >= 0) {
    printf("pose %ld is not finite\n", (long)bad);
    return 3;
  }
  FILE* out = fopen(argv[2], "w");
  if (!out) return 1;
  fprintf(out, "%d\n%d\n%d\n%d\n", e.n_poses, e.n_pairs, e.ate_max_pose, e.rpe_max_pose);
  const double d[12] = {e.align_x,  e.align_y, e.align_phi,      e.ate_rmse,      e.ate_mean,     e.ate_max,
                        e.rot_rmse, e.rot_max, e.rpe_trans_rmse, e.rpe_trans_max, e.rpe_rot_rmse, e.rpe_rot_max};
  for (double v : d) fprintf(out, "%.17g\n", v);
  for (long i = 0; i < n; ++i) fprintf(out, "%.17g %.17g\n", per[2 * i], per[2 * i + 1]);
  if (fclose(out) != 0) return 1;
  printf("traj error ok: %ld poses, %d counted, %d pairs\n", n, e.n_poses, e.n_pairs);
  return 0;
}
