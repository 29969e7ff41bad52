// Test hooks (pgo_debug_set_knob, include/pgo.h): process-wide, read when a handle is created.  -1 = library default.
#include <atomic>
#include <cstring>
#include <string>

#include "pgo_internal.h"

namespace pgo {
namespace {
struct Knob {
  const char* name;
  std::atomic<long long> value;
};
Knob g_knobs[] = {{"spmv_pipe", {-1}}, {"fused_p", {-1}}, {"direct_fail_at", {-1}}, {"direct_setup_fail", {-1}}, {"single_reduction", {-1}}, {"verify_residual", {-1}}, {"shm_timeout_s", {-1}}, {"pad_tiles", {-1}}, {"cov_poses_per_pass", {-1}}, {"cov_direct_cols", {-1}}, {"gate_joint_shape", {-1}}, {"score_grid", {-1}}, {"coarsen_grid", {-1}}, {"gnc_grid", {-1}}, {"support_grid", {-1}}, {"chordal_grid", {-1}}, {"mix_grid", {-1}}, {"prior_add_grid", {-1}}};
}  // namespace

long long knob(const char* name) {
  for (Knob& k : g_knobs)
    if (!strcmp(k.name, name)) return k.value.load();
  return -1;
}
}  // namespace pgo

extern "C" int pgo_debug_set_knob(const char* name, long long value) {
  if (!name) return pgo::fail(PGO_ERR_INVALID_ARG, "pgo_debug_set_knob: null name");
  for (pgo::Knob& k : pgo::g_knobs)
    if (!strcmp(k.name, name)) {
      k.value.store(value < 0 ? -1 : value);
      return PGO_OK;
    }
  return pgo::fail(PGO_ERR_INVALID_ARG, std::string("pgo_debug_set_knob: unknown knob ") + name);
}
