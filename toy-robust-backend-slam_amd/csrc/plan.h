#pragma once
// What a handle is going to do, decided once: pure functions from facts -- option values, the environment, test-hook values
// and the shape of the shard -- to decisions.  pgo_handle::create (solver_create.hip) gathers the facts, calls the stages
// below in the order the data becomes available, and then only allocates, uploads and launches what the plan says; nothing
// writes the plan after create() returns (what changes during a handle's life is live state beside it, solver_handle.hip.h).
// Plain C++17, no HIP types: tests/native/plan_main.cpp evaluates every rule here on the host under ASan + UBSan.
//
//   before the structure   plan_pre       block size, chain length, pose reordering, shard alignment
//   after the structure    plan_padding   the padded tile layout
//                          plan_shard     product kernel, grids, partial capacity, group / chain / solo shapes, loop form, halo
//   direct solve           plan_direct    the decision ladder with its refusals, the take-over case, every size
//   coarse level           plan_coarse    the refusals, the auto rule, the sizes, and what the level takes from the LM loop
//   at last                plan_finish    the loop form once the coarse decision is known
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <string>

#include "constants.h"
#include "pgo_internal.h"

namespace pgo {

// ---------------------------------------------------------------------------------------------------------------- facts
struct PlanKnobs {   // pgo_debug_set_knob values (-1 = library default), read by the caller: nothing here looks a hook up
  long long pad_tiles = -1, spmv_pipe = -1, fused_p = -1, single_reduction = -1, verify_residual = -1, direct_fail_at = -1;
};
struct PlanEnv {
  int world = 1, rank = 0;
  bool has_comm = false, force_collectives = false, batch_mode = false;
  bool multi_rank() const { return has_comm && (world > 1 || force_collectives); }
};
struct ShardFacts {   // of this rank's shard (pgo::ShardStructure), after build_shard_structure
  int64_t N = 0, E = 0, NL = 0, EL = 0;
  int n_tiles = 0;
  int64_t n_inc = 0;           // after pad_tiles_to_slots, where it ran
  int64_t rows_per_rank = 0, lo = 0;
  bool tiles_plain = true;     // every tile: at most WG incidences and at most 85 rows (no chunked heavy row, one row-phase pass)
  bool tiles_fit_wg = true;    // every tile: at most WG incidences (the batched handle's test)
};
struct PlanRefusal {   // PGO_OK, or the status and the detail text create() fails with
  int status = PGO_OK;
  std::string why;
  explicit operator bool() const { return status != PGO_OK; }
};

inline int plan_cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
inline int plan_up8(int g) { return ((g + 7) / 8) * 8; }   // XCD-aware kernels need gridDim % 8 == 0

// ------------------------------------------------------------------------------------------------- before the structure
inline bool chain_len_valid(int chain_len) {
  return chain_len == 0 || !(chain_len < dev::CHAIN_CHUNK || chain_len % dev::CHAIN_CHUNK != 0 || dev::CHAIN_TILE % chain_len != 0);
}

struct PlanPre {   // identical on every rank: it reads the whole graph, the options and the world size only
  PlanRefusal no;
  int grp_B = 1;        // poses per block-Jacobi block as resolved (1 with the chain preconditioner)
  int chain_len = 0;
  bool reorder = false;
  int order_segment = ORDER_SEGMENT;   // chain segments must stay contiguous under the renumbering
  int64_t row_align = 1;
};
inline PlanPre plan_pre(const pgo_options& opt, const PlanEnv& env, int32_t N, int32_t E, const int32_t* ia, const int32_t* ib) {
  PlanPre P;
  P.grp_B = resolve_block_poses(opt.pcg_block_poses, N);
  P.chain_len = resolve_chain_len(opt.pcg_chain_len, opt.pcg_block_poses, N, E, ia, ib);
  if (!chain_len_valid(P.chain_len)) {
    P.no = {PGO_ERR_INVALID_ARG, "pcg_chain_len: a multiple of 4 that divides 256 (4 ... 256), 0 = off, -1 = auto"};
    return P;
  }
  if (P.chain_len) P.grp_B = 1;
  // internal pose numbering
  // auto: several ranks (it shrinks every rank's halo 2.6-2.9x), and single-rank graphs too large for the direct solve, where
  // it is worth -11 % of K3's fabric traffic (977 -> 870 MB per product at 1M poses: the gathers of neighbouring tiles hit
  // the XCD's L2), -16 % of K2's and -22 % of K1's reads: 38.7 / 40.1 -> 39.7 / 41.5 GN it/s (profiles/r03_order.md)
  P.reorder = opt.pose_ordering == 1 || (opt.pose_ordering < 0 && (env.world > 1 || N > DIRECT_MAX_POSES));
  P.order_segment = std::max<int>(ORDER_SEGMENT, P.chain_len);
  P.row_align = P.chain_len ? P.chain_len : P.grp_B;
  if (opt.pcg_coarse_poses > 0 && env.multi_rank() && !env.batch_mode) {
    // the second preconditioner level on several ranks: shards of whole aggregates, so that the aggregation is the one-rank
    // aggregation (plan_coarse)
    P.row_align = std::lcm(P.row_align, (int64_t)opt.pcg_coarse_poses);
    if (P.row_align * env.world > (int64_t)1 << 30) P.no = {PGO_ERR_INVALID_ARG, "pcg_coarse_poses: too large to align the shards to"};
  }
  return P;
}

// -------------------------------------------------------------------------------------------------- after the structure
// Graphs large enough for the one-tile-per-workgroup product kernel (k_spmv_1, below) get the padded-slot layout: every
// tile's incidences at TILE_INC t (structure.cpp, pad_tiles_to_slots).  Test hook "pad_tiles" = 0 keeps the dense layout.
inline int one_tile_min(const PlanKnobs& k) { return k.pad_tiles == 1 ? 0 : 4096; }   // (test hook: the large-graph layout and product kernel on a graph of any size)
inline bool plan_padding(const PlanKnobs& k, const PlanEnv& env, int n_tiles) {
  return !env.batch_mode && n_tiles > one_tile_min(k) && k.pad_tiles != 0;
}

// What every rank must agree on: the form of the PCG loop and its collectives.  Decided from rank-independent inputs only.
struct PlanAll {
  int chain_len = 0;
  int chain_chunk = 0, chain_steps = 0;   // lean apply: poses per lane (2 / 4) and recurrence steps
  int solo_steps = 0, solo_scan = 0;      // batched handles: the one-workgroup PCG's recurrence (solo.hip.h)
  bool use_halo = false;                  // halo exchange of the search direction (world > 1, opt.halo_exchange)
  bool fused_p = false;                   // small graphs on one rank: the direction update rides in the next SpMV (two launches per iteration)
  bool use_sr = false;                    // single-reduction PCG loop (k_cg_sr_*)
  bool fused_p_buffer = false, sr_buffer = false;   // p_full2 / sr_s exist: the one-level answer (they are allocated before the coarse level is)
  bool verify_residual = false;           // test hook: pcg() reports the true residual of its solution
};
// What a rank sizes for itself from its own shard: grids, capacities, list lengths.
struct PlanOwn {
  bool spmv_pipe = false;       // software-pipelined K3 (k_spmv_p): when no tile is a chunked heavy row or has > 85 rows
  bool spmv_one_tile = false;   // the plain-tile product kernel as k_spmv_1: one tile per workgroup, as many workgroups as tiles
  int64_t inc_stride = 64;      // whole 64-incidence groups (dev::hoff_index)
  int g_edge = 1, g_rows = 1, g_vec = 1, g_flat = 1, g_spmv = 1, g_asm = 1;
  int part_cap = 0;
  // block-Jacobi over groups of B poses (B > 1): explicit dense inverses.  (grp_B falls back to 1 on a rank that owns no rows;
  // the group kernels run no collective, so the loop form does not depend on it.)
  int grp_B = 1, grp_nb = 3, grp_pad = 32, n_groups = 0, g_grp = 1;
  size_t grp_lds = 0;
  int grp_prep_grid = 1;
  int chain_pad = 0;
  int chain_scan = 0;   // > 0: the lean apply runs its recurrence as this many scan levels (few long segments)
  int chain_nw = 4;     // wavefronts per workgroup of the lean kernels: 1 on small graphs (a tile per CU)
  int g_chain = 1;
  // The one schedule decision that still reads a per-rank fact (n_tiles > 0): it belongs with PlanAll and sits here until it is
  // decided from rank-independent inputs.
  bool overlap = false;
  int g_spmv_loc = 0;
  int n_rr = 0, g_rr = 0;   // rows with remote columns (counted by create() once overlap is decided) and k_spmv_remote's grid
};
struct PlanShard {
  PlanRefusal no;
  PlanAll all;
  PlanOwn own;
};

inline int remote_rows_grid(int n_rr) { return std::min(std::max(1, (n_rr + dev::WG - 1) / dev::WG), 512); }

// (fused_p / use_sr: the one-level answer; plan_finish settles them once the coarse decision is known)
inline PlanShard plan_shard(const pgo_options& opt, const PlanEnv& env, const PlanKnobs& knob, const PlanPre& pre, const ShardFacts& F) {
  PlanShard R;
  PlanAll& A = R.all;
  PlanOwn& O = R.own;
  const int64_t NL = F.NL, EL = F.EL;
  const int chain_len = A.chain_len = pre.chain_len;
  O.inc_stride = ((F.n_inc + 63) / 64) * 64;
  if (O.inc_stride == 0) O.inc_stride = 64;
  O.g_edge = plan_up8(std::max(1, plan_cdiv(EL, dev::WG)));
  O.g_rows = std::max(1, plan_cdiv(NL, dev::WG));
  O.g_vec = std::min(std::max(1, plan_cdiv(NL, dev::WG)), 1024);
  O.g_flat = std::min(std::max(1, plan_cdiv(3 * NL, dev::WG)), 1024);
  O.g_spmv = plan_up8(std::min(std::max(1, F.n_tiles), 2048));
  O.g_asm = plan_up8(std::min(std::max(1, F.n_tiles), 1 << 20));
  O.part_cap = std::max(std::max(O.g_edge, 2048), plan_up8(std::max(1, F.n_tiles))) + 8 + 512;   // (k_spmv_1: one dot partial per tile)   // (+ the coarse level's dot partials behind the one-level r.z partials)
  // The same 512 behind K1's g_edge cost partials take k_prior_eval's (eval_enqueue appends them in part[5], which holds nothing
  // of the coarse level then): whoever shrinks that slack meets this line, and pgo_set_priors checks the sum at run time.
  static_assert(dev::PRIOR_MAX_GRID <= 512, "part_cap: no room for the pose priors' cost partials behind K1's");
  {
    // the software-pipelined product kernel (k_spmv_p) needs plain tiles: no chunked heavy row, at most 85 rows
    // (one row-phase pass).  Measured on one box at 1M poses: k_spmv_t 185.7 us (8 workgroups per CU), k_spmv_p
    // 172.4 / 175.5 / 168.8 / 165.1 us at 8 / 6 / 5 / 4 workgroups per CU -- hence 4.
    O.spmv_pipe = knob.spmv_pipe != 0 && F.tiles_plain;   // (test hook: 0 keeps k_spmv_t so that the two product kernels can be compared)
    if (O.spmv_pipe) {
      const int per_cu = 4;
      O.g_spmv = ((std::min(std::max(1, F.n_tiles), 256 * per_cu) + 7) / 8) * 8;
      // Large graphs: one tile per workgroup (k_spmv_1) -- 151 us against the pipelined form's 164-166 us at 1M poses; test
      // hook "spmv_pipe" = 2 keeps k_spmv_p there.  Up to 4096 tiles the persistent forms stay: fewer partials, no
      // k_fold_partials launch in a latency-bound iteration (100k poses, 3.2k tiles: 247 vs 237 GN it/s; 60k: 369 vs 329).
      // (One dot partial per tile: part_cap above is at least up8(n_tiles) + 520.)
      if (F.n_tiles > one_tile_min(knob) && knob.spmv_pipe != 2) {
        O.spmv_one_tile = true;
        O.g_spmv = plan_up8(F.n_tiles);
      }
    }
  }
  // halo lists for the point-to-point exchange of the search direction
  A.use_halo = env.world > 1 && opt.halo_exchange != 0;
  if (A.use_halo && opt.halo_overlap != 0 && F.n_tiles > 0) {
    O.overlap = true;
    O.g_spmv_loc = plan_up8(std::min(std::max(1, F.n_tiles), 1536));  // + g_rr <= 2048 partials
  }
  // preconditioner block size
  O.grp_B = pre.grp_B;
  if (O.grp_B > 1 && NL > 0) {
    O.grp_nb = 3 * O.grp_B;
    O.grp_pad = O.grp_nb;  // lanes per group in the apply kernels (any value <= WG works: slot = tid / grp_pad)
    O.n_groups = (int)((NL + O.grp_B - 1) / O.grp_B);
    const int gpw = dev::WG / O.grp_pad;
    O.g_grp = std::min(std::max(1, (O.n_groups + gpw - 1) / gpw), 2048);
    const int prep_gpw = (O.grp_nb <= 24) ? dev::WG / 64 : 1;  // groups per workgroup in k_prepare_groups
    O.grp_lds = (size_t)prep_gpw * O.grp_nb * (O.grp_nb + 1) * sizeof(double);
    O.grp_prep_grid = std::min((O.n_groups + prep_gpw - 1) / prep_gpw, 65536);
  } else {
    O.grp_B = 1;
  }
  // One-workgroup PCG (solo.hip.h): a single rank, a chain or 3x3 block-Jacobi preconditioner, no chunked heavy row.
  // Batched handles only: on a single graph one CU's L1 paces the solve -- INTEL 36 us per PCG iteration against 27 us for
  // the three-kernel loop on 256 CUs, MIT / FR079 8 % faster -- the win is the BATCH, where every problem has a CU of its own
  if (env.batch_mode && !(env.world == 1 && !env.force_collectives && O.grp_B == 1 && NL > 0 && F.tiles_fit_wg)) {
    R.no = {PGO_ERR_UNSUPPORTED, "pgo_batch: a problem has a row with more than 256 incidences"};
    return R;
  }
  if (chain_len) {   // (also on a rank that owns no rows: every rank must resolve to the same PCG loop and the same collectives)
    O.chain_pad = (int)(((NL + dev::CHAIN_TILE - 1) / dev::CHAIN_TILE) * dev::CHAIN_TILE);
    if (!env.batch_mode) {
      // apply kernel: the lean form (one DPP-shift recurrence step per lane of a segment), 2 poses per lane for segments of
      // <= 64 poses, 4 for longer ones (INTEL, chain-256: the earlier scan form over whole 256-row tiles took 20 us per apply
      // -- five tiles, latency-bound -- of a 30 us PCG iteration)
      A.chain_chunk = chain_len <= 64 ? 2 : 4;   // 4: segments of up to 256 poses (the small chain-like graphs)
      A.chain_steps = chain_len / A.chain_chunk - 1;
      const int64_t n_wt = (NL + 64 * A.chain_chunk - 1) / (64 * A.chain_chunk);
      // Small graphs (few tiles, nothing to overlap with): one wavefront per workgroup, so that every tile loads through
      // its own CU's L1, and -- for segments of more than 16 lanes -- the recurrence as a log-depth scan (INTEL, 256-pose
      // segments: 7.4 -> 4.8 us per apply); large graphs keep the 4-wave workgroups and the serial DPP recurrence,
      // which needs fewer registers and no LDS-crossbar shuffles.
      const bool small = n_wt <= 512;
      O.chain_nw = small ? 1 : 4;
      O.chain_scan = 0;
      if (small && chain_len / A.chain_chunk > 16)
        for (int l = 1; l < chain_len / A.chain_chunk; l <<= 1) ++O.chain_scan;
      // every workgroup of the NEXT kernel re-sums this kernel's per-workgroup partials, so fewer, longer-running
      // workgroups are cheaper all round: 2048 -> 512 (and 1024 for the flat vector kernels) 25.43 -> 24.65 ms per LM
      // iteration at 1M poses (same box, 3 interleaved repetitions)
      O.g_chain = (int)std::max<int64_t>(1, std::min<int64_t>((n_wt + O.chain_nw - 1) / O.chain_nw, O.chain_nw == 1 ? 2048 : 512));
    } else {
      A.chain_chunk = dev::SOLO_CH;  // the 256-row tile layout of the factor planes
      A.chain_steps = chain_len / A.chain_chunk - 1;
      const int64_t n_wt = (NL + 64 * A.chain_chunk - 1) / (64 * A.chain_chunk);
      O.chain_nw = n_wt <= 512 ? 1 : 4;
      O.chain_scan = 0;
      O.g_chain = (int)std::min<int64_t>((n_wt + O.chain_nw - 1) / O.chain_nw, 2048);
      const int lanes = chain_len / dev::SOLO_CH;  // lanes per segment: serial recurrence up to 16, else log-depth scan
      A.solo_steps = lanes - 1;
      A.solo_scan = 0;
      if (lanes > 16)
        for (int l = 1; l < lanes; l <<= 1) ++A.solo_scan;
    }
  }
  {
    const int64_t fused_max = 16384;
    A.fused_p = A.fused_p_buffer = knob.fused_p != 0 && env.world == 1 && !env.force_collectives && !env.batch_mode && NL > 0 && NL <= fused_max;
  }
  {
    // One reduction point per PCG iteration instead of two (k_cg_sr_*): where the all-reduces are latency -- several ranks --
    // and only in the inexact mode (pcg_rtol >= 1e-6: the recurrence for A p drifts over the thousands of iterations of
    // the exact mode); needs the lean chain apply.  Test hook "single_reduction": 1 = also on one rank, 0 = never.
    const long long kn = knob.single_reduction;
    A.use_sr = A.sr_buffer = chain_len > 0 && !A.fused_p && !env.batch_mode && opt.pcg_rtol >= 1e-6 &&
                             (kn == 1 || (kn != 0 && (env.world > 1 || env.force_collectives)));
    A.verify_residual = knob.verify_residual == 1;
  }
  return R;
}

// --------------------------------------------------------------------------------------------------------- direct solve
// Direct solve for small chain-like graphs (direct.hip.h).  opt.linear_solver: 0 = auto, 1 = PCG, 2 = direct.
// Auto picks it in the "exact" mode only (pcg_rtol <= 1e-8, where PCG stands in for the reference's
// SPARSE_NORMAL_CHOLESKY, main.cpp:154-163) and only while the caller left the preconditioner to the library; it needs
// one rank, METHOD 0 / 1, a constant pose, an edge between every pair of consecutive poses, and few enough other edges.
struct DirectFacts {
  int32_t N = 0;
  bool info_mode = false, has_constant_pose = false, permuted = false;
  // of the shard's edge list, needed only where plan_direct_gate passes (DirectPlan::need_chain):
  int32_t gap = -1;   // the first i without an edge (i, i + 1), or -1
  int m = 0;          // edges outside the odometry chain
};
struct DirectPlan {
  PlanRefusal no;
  bool need_chain = false;   // the gate passed: gap and m decide the rest
  bool direct = false;       // the handle solves directly from its first LM iteration
  bool dl_possible = false;     // auto, rank above DIRECT_AUTO_RANK: the direct solve can take over from PCG (lm_iteration)
  double dl_est_seconds = 0.0;  // what a direct solve of this rank costs (model fitted to INTEL / FRH / M3500)
  // sizes: functions of N and m alone, the same for a handle that starts direct and for one that switches later
  int dl_m = 0, dl_K = 0, dl_Kp = 0, dl_ld = 0, dl_refine = 1;
  int dl_nsep = 0, dl_sep[dev::DLR_MAX_SEP] = {0}, dl_nU = 0;
  int dl_nseg = 1, dl_seglen = 1;
  int dl_nseg2 = 1, dl_seglen2 = 1;   // the finer segmentation of k_dlr_solve1 (up to 256 segments of <= 16 poses)
  bool dl_fine = false;               // ... exists (dl_pre2)
  int dl_fail_at = 0;                 // test hook "direct_fail_at": poison the direct solve of this LM iteration
};

inline void plan_direct_sizes(DirectPlan* D, int32_t N, int m, long long knob_fail_at) {
  D->dl_m = m;
  D->dl_K = 3 * m;
  D->dl_Kp = std::max(dev::CHOL_NB, ((D->dl_K + dev::CHOL_NB - 1) / dev::CHOL_NB) * dev::CHOL_NB);
  // separators: the chain is factorised in nsep + 1 pieces side by side (k_dlr_factor is one wavefront's dependent chain:
  // 0.3 us per pose)
  D->dl_nsep = 0;
  if (N >= 256) {
    // 3 separators up to ~5000 poses (INTEL / MIT: 3 -> 826 / 2392 GN it/s, 5 -> 813 / 2294, 7 -> 788 / 2116, 15 -> 606 / 1209:
    // every separator adds 3 columns and a row of the Schur system), then one per ~1200 poses (40k poses: 3 -> 156, 15 -> 205)
    D->dl_nsep = std::min(dev::DLR_MAX_SEP, std::max(3, (int)(N / 1200)));
    for (int j = 0; j < D->dl_nsep; ++j) D->dl_sep[j] = (int)(((int64_t)(j + 1) * N) / (D->dl_nsep + 1));
  }
  D->dl_nU = 3 * D->dl_nsep;
  D->dl_ld = ((D->dl_K + 1 + D->dl_nU + 63) / 64) * 64;
  D->dl_refine = 1;   // (a second step does not lower FRH's 5e-8: that residual is what the conditioning allows)
  if (knob_fail_at > 0) D->dl_fail_at = (int)knob_fail_at;   // test hook
  const int want_seg = 32;   // segments the chain sweeps are cut into (at most DLR_MAX_SEG)
  D->dl_seglen = std::max(1, (N + want_seg - 1) / want_seg);
  D->dl_nseg = (N + D->dl_seglen - 1) / D->dl_seglen;
  D->dl_fine = N <= 4096;
  if (D->dl_fine) {
    D->dl_seglen2 = std::max(1, (N + 255) / 256);
    D->dl_nseg2 = (N + D->dl_seglen2 - 1) / D->dl_seglen2;
  }
}

inline PlanRefusal direct_no(int want, const std::string& why) {
  if (want == 2) return {PGO_ERR_UNSUPPORTED, "linear_solver = direct: " + why};
  return {};
}
// the part of the ladder that needs no look at the edges
inline DirectPlan plan_direct_gate(const pgo_options& opt, const PlanEnv& env, const DirectFacts& F) {
  DirectPlan D;
  const int want = opt.linear_solver;
  if (want == 1) return D;
  if (want != 0 && want != 2) {
    D.no = {PGO_ERR_INVALID_ARG, "linear_solver: 0 = auto, 1 = PCG, 2 = direct (chain + low rank)"};
    return D;
  }
  if (want == 0 && (!(opt.pcg_rtol <= 1e-8) || opt.pcg_chain_len != -1 || opt.pcg_block_poses != 0)) return D;
  if (env.world != 1 || env.force_collectives) D.no = direct_no(want, "one rank only");
  else if (env.batch_mode) D.no = direct_no(want, "not inside a batched handle");
  // information weighting: the chain blocks inherit the information matrices' condition numbers (INTEL: 1e11) and the
  // Woodbury correction loses the solution (measured: residual 1e-3 after refinement); MIT-like inputs would work, but the
  // library cannot tell from the graph -- PCG there
  else if (F.info_mode) D.no = direct_no(want, "not with information weighting");
  else if (!F.has_constant_pose) D.no = direct_no(want, "needs a constant pose (it anchors the chain)");
  else if (F.permuted) D.no = direct_no(want, "the internal pose ordering is on");
  else if (F.N < 2 || F.N > DIRECT_MAX_POSES) D.no = direct_no(want, "2 .. " + std::to_string(DIRECT_MAX_POSES) + " poses");
  else D.need_chain = true;
  return D;
}
// ... and the part that does (F.gap, F.m)
inline DirectPlan plan_direct(const pgo_options& opt, const PlanEnv& env, const PlanKnobs& knob, const DirectFacts& F) {
  DirectPlan D = plan_direct_gate(opt, env, F);
  if (!D.need_chain) return D;
  const int want = opt.linear_solver;
  if (F.gap >= 0) {
    D.no = direct_no(want, "poses " + std::to_string(F.gap) + " and " + std::to_string(F.gap + 1) + " are not joined by an edge");
    return D;
  }
  const int K = 3 * F.m;
  if (want == 0 && K > DIRECT_AUTO_RANK) {
    // beyond this rank the dense Cholesky is no longer cheap (M3500, 5862: 12.7 ms per LM iteration) and whether PCG beats it
    // depends on the conditioning, which nobody knows beforehand (M3500 with DCS: 1460 PCG iterations per LM iteration =
    // 21 ms; without: 230 = 4 ms).  So the handle starts with PCG and lm_iteration() switches to the direct solve once a
    // PCG solve has cost more than the direct one would (both from counts, not clocks: the decision is reproducible)
    if (K + 1 <= DIRECT_MAX_RANK) {
      D.dl_possible = true;
      // cost model of a direct solve: the capacitance Cholesky (M3500, rank 5862: 11.7 ms; ~ rank^2.5 between INTEL, FRH and
      // M3500) + the chain (factorisation and sweeps: 0.15 us per pose, 5k .. 40k-pose chains) + 1 ms of fixed latencies
      const double kk = K / 5862.0;
      D.dl_est_seconds = 1.0e-3 + 11.7e-3 * kk * kk * std::sqrt(kk) + 0.15e-6 * F.N;
      plan_direct_sizes(&D, F.N, F.m, knob.direct_fail_at);
    }
    return D;
  }
  if (K + 1 > DIRECT_MAX_RANK) {
    D.no = direct_no(want, std::to_string(F.m) + " edges outside the odometry chain (at most " + std::to_string((DIRECT_MAX_RANK - 1) / 3) + ")");
    return D;
  }
  plan_direct_sizes(&D, F.N, F.m, knob.direct_fail_at);
  D.direct = true;
  return D;
}

// --------------------------------------------------------------------------------------------------------- coarse level
// Second preconditioner level (coarse.hip.h).  opt.pcg_coarse_poses: 0 = off, > 0 = poses per aggregate, -1 = auto.
// Every decision is taken on rank-independent inputs (the graph, the options, the shard size): all ranks enable the level, or
// none does.  Only co_aoff and co_nown are a rank's own.
struct CoarsePlan {
  PlanRefusal no;
  bool on = false;   // the level exists (for the LM loop, or -- plan_coarse_for_covariance -- for covariance calls only)
  bool co_multi = false;
  int co_agg = 0, co_nagg = 0, co_K = 0, co_Kp = 0;
  int co_aoff = 0, co_nown = 0;   // this rank's aggregates: [co_aoff, co_aoff + co_nown) (co_nagg counts all of them)
  int co_ndot = 0;                // partials of r_c . e_c appended to the r.z partials
  bool co_explicit = false;       // explicit inverse N'N (coarse orders <= COARSE_EXPLICIT_RANK: one product per apply)
};

// the auto rule's aggregate size for a shard of NL poses (also the size of the level that covariance calls build for
// themselves): 16 poses up to 8192 poses, else 64, doubled until the coarse order fits the dense factorisation
inline int coarse_auto_poses(int64_t NL) {
  int want = NL <= 8192 ? 16 : 64;
  while (3 * ((NL + want - 1) / want) + 1 > COARSE_MAX_RANK) want *= 2;
  return want;
}

// want: opt.pcg_coarse_poses, or the aggregate size a covariance call asks for; direct: the handle starts on the direct solve
inline CoarsePlan plan_coarse(const pgo_options& opt, const PlanEnv& env, const ShardFacts& F, bool direct, int want) {
  CoarsePlan C;
  const bool multi = env.multi_rank();
  const int64_t NL = F.NL, N = F.N;
  if (want == 0) return C;
  auto no = [&](const std::string& why) {
    if (want > 0) C.no = {PGO_ERR_UNSUPPORTED, "pcg_coarse_poses: " + why};
    return C;
  };
  // several ranks: only on request (auto stays one level until a multi-GPU box has measured it).
  if (multi && want < 0) return C;
  if (env.batch_mode) return no("not inside a batched handle");
  if (N < 2) return C;
  if (want < 0) {
    // auto (measured on MI355X, scripts/exp_coarse.py, GN it/s one level -> two levels):
    //   tight solves (pcg_rtol <= 1e-3) of graphs that stay on PCG -- M3500 METHOD 1 47 -> 156 (16-pose aggregates, coarse
    //   order 657; 32: 128, 64: 100), FRH 35 -> 199 (16), synthetic 10k at 1e-10 108 -> 137 (64; 16: 127), 100k at 1e-10
    //   3.7 -> 12.3 and at 1e-3 14.9 -> 40.5 (64, order 4689; 128 and more: no gain) -- 16 poses up to 8192 poses, else
    //   64, doubled until the coarse order fits the dense factorisation;
    //   loose solves (the inexact mode) stay on one level: measured both ways -- synthetic 10k at rtol 0.1, 64-pose aggregates:
    //   371 -> 771 over a long run at large radius, but 582 -> 530 over the first 50 LM iterations, where a solve needs few PCG
    //   iterations anyway and the coarse factorisation per LM iteration is pure overhead; 100k: 189 -> 80 .. 121.
    // ... and only while the caller left the one-level preconditioner to the library (like the direct solve's auto rule): an
    // explicit pcg_block_poses / pcg_chain_len is a request for exactly that preconditioner
    if (direct || NL < 512 || opt.pcg_chain_len != -1 || opt.pcg_block_poses != 0 || !(opt.pcg_rtol <= 1e-3)) return C;
    want = coarse_auto_poses(NL);
  }
  C.co_agg = want;
  if (multi && F.rows_per_rank % C.co_agg != 0) {
    C.no = {PGO_ERR_INVALID_ARG, "pcg_coarse_poses: shards not aligned to the aggregates"};
    return C;
  }
  // aggregates: runs of co_agg consecutive rows, numbered globally; this rank owns [co_aoff, co_aoff + co_nown) (one rank: all)
  C.co_nagg = (int)((N + C.co_agg - 1) / C.co_agg);
  C.co_aoff = (int)(F.lo / C.co_agg);
  C.co_nown = (int)((NL + C.co_agg - 1) / C.co_agg);
  C.co_K = 3 * C.co_nagg;
  if (C.co_K + 1 > COARSE_MAX_RANK) return no("the coarse matrix would have order " + std::to_string(C.co_K) + " (at most " + std::to_string(COARSE_MAX_RANK - 1) + ")");
  C.co_Kp = ((C.co_K + dev::CHOL_NB - 1) / dev::CHOL_NB) * dev::CHOL_NB;
  C.co_explicit = C.co_Kp <= COARSE_EXPLICIT_RANK;
  C.co_ndot = C.co_explicit ? (C.co_Kp + 3) / 4 : (C.co_Kp + 255) / 256;
  C.co_multi = multi;
  C.on = true;
  return C;
}

// The rigid-body coarse level for handles that were created without it (direct solves, the inexact mode, pcg_coarse_poses = 0)
// on graphs of >= 512 poses: built at the first covariance call, with the aggregate size of the auto rule, and used by
// covariance calls only -- the LM loop's plan does not know it.
inline CoarsePlan plan_coarse_for_covariance(const pgo_options& opt, const PlanEnv& env, const ShardFacts& F) {
  if (F.NL < 512) return {};
  return plan_coarse(opt, env, F, false, coarse_auto_poses(F.NL));
}

// ---------------------------------------------------------------------------------------------------------------- whole
struct Plan {
  PlanPre pre;
  PlanAll all;   // identical on every rank
  PlanOwn own;   // sized per rank
  DirectPlan dl;
  CoarsePlan co;       // the LM loop's second level
  CoarsePlan co_cov;   // the level covariance calls build where the LM loop has none (on: it can be built)
};

// What the coarse level takes from the LM loop: the loops that fold launches together assume the one-level preconditioner, so
// two-level solves take the plain three-kernel loop (several ranks: the two-reduction loop on every rank); and ranks above the
// direct solve's cheap range get two-level PCG instead of the PCG / direct alternation under linear_solver = 0.
inline void plan_finish(const pgo_options& opt, Plan* P) {
  if (!P->co.on) return;
  P->all.fused_p = false;
  P->all.use_sr = false;
  if (opt.linear_solver == 0) P->dl.dl_possible = false;
}

}  // namespace pgo
