#pragma once
// The sizes and thresholds that both the device code and the host's decisions (plan.h) depend on, each defined here and
// nowhere else.  Plain C++: no HIP types, so that g++ takes plan.h and its stand-alone test without a HIP include.
namespace pgo {

#ifndef PGO_TILE_INC
#define PGO_TILE_INC 256   // (experiment builds may lower it: smaller tiles, more workgroups)
#endif
constexpr int TILE_INC = PGO_TILE_INC;

namespace dev {
constexpr int WG = 256;          // workgroup size of every kernel here (4 waves)
constexpr int PS = 3;            // doubles per pose in the GATHERED vector p.  Padding to 4 (32 B, never straddling a
                                 // 64-byte sector) was measured: no fewer fetched bytes (FETCH_SIZE 566 vs 557 MiB), so 3.
constexpr int CHAIN_CHUNK = 4;                        // the segment length is a multiple of this
constexpr int CHAIN_TILE = 256;                       // rows of the largest tile = 64 lanes x CHAIN_CHUNK: n_pad is a multiple
constexpr int SOLO_CH = 4;                // chain layout: 256-row wave tiles
constexpr int CHOL_NB = 32;
constexpr int DLR_MAX_SEP = 15;  // separator poses: the chain factorisation runs nsep + 1 pieces side by side (3 separators up to ~2000 poses)
constexpr int DLR_MAX_SEG = 64;
constexpr int PRIOR_MAX_GRID = 256;   // workgroups of k_prior_eval = cost partials appended to K1's (a grid-stride loop above 65536 priors)
}  // namespace dev

constexpr int DIRECT_MAX_POSES = 65536;   // largest graph the direct (chain + low-rank) solve takes
constexpr int DIRECT_MAX_RANK = 6144;    // 3 x (edges outside the chain) + 1: order of the dense capacitance matrix
// Cost model of the adaptive PCG / direct choice (solver_lm.hip): MEASURED ON MI355X -- a PCG iteration of the two-launch
// loop on graphs of a few thousand poses, and the rank up to which auto takes the direct solve outright (INTEL + 50: 918 ->
// 1.5 ms per LM iteration; FRH, 4515: 13 ms against 29 ms of PCG; M3500, 5862: 22 ms, the same as PCG).  Device-specific
// constants, not options: they only decide speed, never results.
constexpr double PCG_SECONDS_PER_ITER_SMALL = 14e-6;
constexpr int DIRECT_PROBE_EVERY = 10;
constexpr int DIRECT_AUTO_RANK = 2048;
constexpr int COARSE_MAX_RANK = 6144;        // order of the dense coarse matrix (k_chol_panel's range)
constexpr int COARSE_EXPLICIT_RANK = 1024;   // up to here the explicit inverse N'N is formed once per LM iteration

}  // namespace pgo
