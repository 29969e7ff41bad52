// csrc/plan.h on the host: the stage functions over a table of named cases -- one line "case NAME key=value ..." each, which
// tests/test_plan_native.py compares with known answers -- then a sweep of the partial-array capacity, the rank-independence
// of the common side of the plan, and structural invariants over pseudo-random facts (checked here; any miss ends the run).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "plan.h"

using namespace pgo;

static long g_checks = 0;
#define CHECK(cond)                                                             \
  do {                                                                          \
    ++g_checks;                                                                 \
    if (!(cond)) {                                                              \
      fprintf(stderr, "plan_main.cpp:%d: CHECK failed: %s\n", __LINE__, #cond); \
      exit(1);                                                                  \
    }                                                                           \
  } while (0)

static pgo_options default_options() {   // the fields plan.h reads, as pgo_options_default sets them
  pgo_options o{};
  o.method = 1;
  o.pcg_rtol = 1e-10;
  o.pose_ordering = -1;
  o.pcg_chain_len = -1;
  o.pcg_block_poses = 0;
  o.halo_exchange = 0;
  o.halo_overlap = 0;
  o.linear_solver = 0;
  o.pcg_coarse_poses = -1;
  return o;
}

struct In {
  pgo_options opt = default_options();
  PlanEnv env;
  PlanKnobs knob;
  ShardFacts F;
  DirectFacts D;
  In() { D.has_constant_pose = true; }
  // a one-rank shard of n poses in n_tiles tiles
  In& shape(int64_t n, int n_tiles) {
    F.N = F.NL = n;
    F.rows_per_rank = n;
    F.EL = F.E = n > 0 ? n - 1 : 0;
    F.n_tiles = n_tiles;
    F.n_inc = 2 * F.EL;
    D.N = (int32_t)n;
    return *this;
  }
};

static const char* spmv_form(const PlanOwn& O) { return !O.spmv_pipe ? "t" : O.spmv_one_tile ? "1" : "p"; }
static std::string quoted(const PlanRefusal& r) { return "status=" + std::to_string(r.status) + " why=\"" + r.why + "\""; }

// the whole plan for one rank, in create()'s order; prints the first refusal, or the decisions
static bool g_refused = false;
static Plan evaluate(const char* name, const In& in, bool print = true) {
  Plan P;
  g_refused = true;
  P.pre = plan_pre(in.opt, in.env, (int32_t)in.F.N, 0, nullptr, nullptr);
  if (P.pre.no) {
    if (print) printf("case %s refused=pre %s\n", name, quoted(P.pre.no).c_str());
    return P;
  }
  const bool pad = plan_padding(in.knob, in.env, in.F.n_tiles);
  const PlanShard sh = plan_shard(in.opt, in.env, in.knob, P.pre, in.F);
  if (sh.no) {
    if (print) printf("case %s refused=shard %s\n", name, quoted(sh.no).c_str());
    return P;
  }
  P.all = sh.all;
  P.own = sh.own;
  P.dl = plan_direct(in.opt, in.env, in.knob, in.D);
  if (P.dl.no) {
    if (print) printf("case %s refused=direct %s\n", name, quoted(P.dl.no).c_str());
    return P;
  }
  P.co = plan_coarse(in.opt, in.env, in.F, P.dl.direct, in.opt.pcg_coarse_poses);
  if (P.co.no) {
    if (print) printf("case %s refused=coarse %s\n", name, quoted(P.co.no).c_str());
    return P;
  }
  if (!P.co.on) P.co_cov = plan_coarse_for_covariance(in.opt, in.env, in.F);
  plan_finish(in.opt, &P);
  g_refused = false;
  if (!print) return P;
  printf("case %s refused=none grp_B=%d chain_len=%d reorder=%d row_align=%" PRId64 " pad=%d spmv=%s g_spmv=%d part_cap=%d", name, P.own.grp_B,
         P.all.chain_len, (int)P.pre.reorder, P.pre.row_align, (int)pad, spmv_form(P.own), P.own.g_spmv, P.own.part_cap);
  printf(" chunk=%d steps=%d nw=%d scan=%d g_chain=%d solo_steps=%d solo_scan=%d", P.all.chain_chunk, P.all.chain_steps, P.own.chain_nw,
         P.own.chain_scan, P.own.g_chain, P.all.solo_steps, P.all.solo_scan);
  printf(" fused_p=%d use_sr=%d use_halo=%d overlap=%d", (int)P.all.fused_p, (int)P.all.use_sr, (int)P.all.use_halo, (int)P.own.overlap);
  printf(" direct=%d dl_possible=%d dl_est=%.17g dl_m=%d dl_K=%d dl_Kp=%d dl_ld=%d dl_nU=%d dl_nsep=%d dl_seglen=%d dl_nseg=%d dl_fine=%d dl_seglen2=%d dl_nseg2=%d",
         (int)P.dl.direct, (int)P.dl.dl_possible, P.dl.dl_est_seconds, P.dl.dl_m, P.dl.dl_K, P.dl.dl_Kp, P.dl.dl_ld, P.dl.dl_nU, P.dl.dl_nsep,
         P.dl.dl_seglen, P.dl.dl_nseg, (int)P.dl.dl_fine, P.dl.dl_seglen2, P.dl.dl_nseg2);
  printf(" sep=");
  for (int j = 0; j < P.dl.dl_nsep; ++j) printf("%s%d", j ? "/" : "", P.dl.dl_sep[j]);
  printf(" coarse=%d co_agg=%d co_K=%d co_Kp=%d co_ndot=%d co_explicit=%d cov_agg=%d\n", (int)P.co.on, P.co.co_agg, P.co.co_K, P.co.co_Kp, P.co.co_ndot,
         (int)P.co.co_explicit, P.co_cov.on ? P.co_cov.co_agg : 0);
  return P;
}

// ---- structural invariants of one plan (what the launch code relies on)
static void invariants(const In& in, const Plan& P) {
  const PlanOwn& O = P.own;
  for (int g : {O.g_edge, O.g_rows, O.g_vec, O.g_flat, O.g_spmv, O.g_asm, O.g_grp, O.g_chain}) CHECK(g >= 1);
  if (O.grp_B > 1) CHECK(O.grp_prep_grid >= 1 && O.n_groups >= 1 && O.grp_nb == 3 * O.grp_B && O.grp_pad <= dev::WG);
  for (int g : {O.g_edge, O.g_spmv, O.g_asm}) CHECK(g % 8 == 0);   // the XCD-aware kernels
  if (O.overlap) CHECK(O.g_spmv_loc >= 1 && O.g_spmv_loc % 8 == 0 && O.g_spmv_loc + remote_rows_grid(1 << 30) <= 2048);
  CHECK(O.g_spmv <= O.part_cap - 520 && O.g_edge <= O.part_cap && 2048 <= O.part_cap);
  CHECK(O.inc_stride >= 64 && O.inc_stride % 64 == 0 && O.inc_stride >= in.F.n_inc);
  if (P.all.chain_len) {
    CHECK(P.all.chain_chunk == 2 || P.all.chain_chunk == 4);
    CHECK(P.all.chain_steps == P.all.chain_len / P.all.chain_chunk - 1);
    CHECK(O.chain_nw == 1 || O.chain_nw == 4);
    CHECK(O.chain_pad % dev::CHAIN_TILE == 0 && O.chain_pad >= in.F.NL);
  }
  CHECK(!(P.all.fused_p && P.all.use_sr));
  CHECK(!(P.co.on && (P.all.fused_p || P.all.use_sr)));
  CHECK(!(P.dl.direct && P.dl.dl_possible));
  if (P.co.on) CHECK(P.co.co_Kp % 32 == 0 && P.co.co_Kp >= P.co.co_K && P.co.co_K + 1 <= COARSE_MAX_RANK && P.co.co_ndot >= 1);
  if (P.dl.direct || P.dl.dl_possible) {
    const DirectPlan& D = P.dl;
    CHECK(D.dl_Kp % 32 == 0 && D.dl_Kp >= D.dl_K && D.dl_Kp >= 32 && D.dl_K + 1 <= DIRECT_MAX_RANK);
    CHECK(D.dl_ld % 64 == 0 && D.dl_ld >= D.dl_K + 1 + D.dl_nU);
    CHECK(D.dl_nsep <= dev::DLR_MAX_SEP && D.dl_nseg >= 1 && D.dl_nseg <= dev::DLR_MAX_SEG && (int64_t)D.dl_nseg * D.dl_seglen >= in.D.N);
    if (D.dl_fine) CHECK(D.dl_nseg2 >= 1 && D.dl_nseg2 <= 256 && D.dl_seglen2 <= 16 && (int64_t)D.dl_nseg2 * D.dl_seglen2 >= in.D.N);
    for (int j = 0; j < D.dl_nsep; ++j) CHECK(D.dl_sep[j] > (j ? D.dl_sep[j - 1] : 0) && D.dl_sep[j] < in.D.N);
  }
}

static bool same_all(const Plan& a, const Plan& b) {   // the side every rank must agree on
  const PlanAll &x = a.all, &y = b.all;
  return a.pre.grp_B == b.pre.grp_B && a.pre.chain_len == b.pre.chain_len && a.pre.reorder == b.pre.reorder && a.pre.row_align == b.pre.row_align &&
         x.chain_len == y.chain_len && x.chain_chunk == y.chain_chunk && x.chain_steps == y.chain_steps && x.solo_steps == y.solo_steps &&
         x.solo_scan == y.solo_scan && x.use_halo == y.use_halo && x.fused_p == y.fused_p && x.use_sr == y.use_sr &&
         x.fused_p_buffer == y.fused_p_buffer && x.sr_buffer == y.sr_buffer && x.verify_residual == y.verify_residual &&
         a.dl.direct == b.dl.direct && a.dl.dl_possible == b.dl.dl_possible && a.co.on == b.co.on && a.co.co_multi == b.co.co_multi &&
         a.co.co_agg == b.co.co_agg && a.co.co_nagg == b.co.co_nagg && a.co.co_K == b.co.co_K && a.co.co_Kp == b.co.co_Kp &&
         a.co.co_ndot == b.co.co_ndot && a.co.co_explicit == b.co.co_explicit;
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {   // splitmix64, fixed seed
  uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
static int64_t pick(std::initializer_list<int64_t> v) { return v.begin()[rnd() % v.size()]; }

int main() {
  // ---------------------------------------------------------------- product kernel
  evaluate("spmv_3", In().shape(600, 3));
  evaluate("spmv_4096", In().shape(400000, 4096));
  evaluate("spmv_4097", In().shape(400000, 4097));
  { In in; in.shape(400000, 4097); in.knob.spmv_pipe = 2; evaluate("spmv_4097_pipe2", in); }
  { In in; in.shape(400000, 4097); in.knob.spmv_pipe = 0; evaluate("spmv_4097_pipe0", in); }
  { In in; in.shape(600, 3); in.knob.spmv_pipe = 0; evaluate("spmv_3_pipe0", in); }
  { In in; in.shape(600, 3); in.knob.pad_tiles = 1; evaluate("spmv_3_pad1", in); }
  { In in; in.shape(400000, 4097); in.knob.pad_tiles = 0; evaluate("spmv_4097_pad0", in); }
  for (int nt : {3, 4097}) {   // one tile not plain (257 incidences: neither test holds; 86 rows: only the batch test holds)
    In in;
    in.shape(400000, nt);
    in.F.tiles_plain = false;
    evaluate(nt == 3 ? "spmv_3_rows86" : "spmv_4097_rows86", in);
    in.F.tiles_fit_wg = false;
    evaluate(nt == 3 ? "spmv_3_inc257" : "spmv_4097_inc257", in);
  }
  { In in; in.shape(400000, 4097); in.F.EL = 1000; evaluate("part_cap_4097", in); }
  // ---------------------------------------------------------------- chain apply
  struct { const char* name; int len; int64_t NL; } chain[] = {{"chain_64_65536", 64, 65536}, {"chain_64_65537", 64, 65537}, {"chain_256_3500", 256, 3500},
                                                               {"chain_32_1000", 32, 1000}, {"chain_4_1000", 4, 1000}};
  for (auto& c : chain) {
    In in;
    in.shape(c.NL, 16);
    in.opt.pcg_chain_len = c.len;
    evaluate(c.name, in);
  }
  for (int len : {2, 6, 96, 512}) {
    In in;
    in.shape(1000, 16);
    in.opt.pcg_chain_len = len;
    evaluate(("chain_bad_" + std::to_string(len)).c_str(), in);
  }
  for (int len : {256, 64}) {
    In in;
    in.shape(1024, 8);
    in.env.batch_mode = true;
    in.opt.pcg_chain_len = len;
    evaluate(("batch_chain_" + std::to_string(len)).c_str(), in);
  }
  { In in; in.shape(1024, 8); in.env.batch_mode = true; in.opt.pcg_chain_len = 64; in.F.tiles_plain = in.F.tiles_fit_wg = false; evaluate("batch_inc257", in); }
  // ---------------------------------------------------------------- fused update, single reduction (PCG asked for: no direct solve, no coarse level)
  auto loop_case = [](const char* name, int64_t NL, int world, bool force, bool batch, long long k_fused, long long k_sr, double rtol, int chain_len, int coarse) {
    In in;
    in.shape(NL, 16);
    in.F.N = NL * world;
    in.env.world = world;
    in.env.has_comm = world > 1 || force;
    in.env.force_collectives = force;
    in.env.batch_mode = batch;
    in.knob.fused_p = k_fused;
    in.knob.single_reduction = k_sr;
    in.opt.linear_solver = 1;
    in.opt.pcg_rtol = rtol;
    in.opt.pcg_chain_len = chain_len;
    in.opt.pcg_block_poses = batch ? 1 : 0;   // (a batch takes 3x3 blocks or the chain)
    in.opt.pcg_coarse_poses = coarse;
    evaluate(name, in);
  };
  loop_case("fused_16384", 16384, 1, false, false, -1, -1, 1e-10, 0, 0);
  loop_case("fused_16385", 16385, 1, false, false, -1, -1, 1e-10, 0, 0);
  loop_case("fused_world2", 8192, 2, false, false, -1, -1, 1e-10, 0, 0);
  loop_case("fused_force", 8192, 1, true, false, -1, -1, 1e-10, 0, 0);
  loop_case("fused_batch", 8192, 1, false, true, -1, -1, 1e-10, 0, 0);
  loop_case("fused_knob0", 8192, 1, false, false, 0, -1, 1e-10, 0, 0);
  loop_case("fused_coarse", 8192, 1, false, false, -1, -1, 1e-10, 0, 16);
  loop_case("sr_world2", 8192, 2, false, false, -1, -1, 1e-6, 64, 0);
  loop_case("sr_world2_tight", 8192, 2, false, false, -1, -1, 9e-7, 64, 0);
  loop_case("sr_world1", 8192, 1, false, false, -1, -1, 1e-6, 64, 0);
  loop_case("sr_world1_knob1_large", 16385, 1, false, false, -1, 1, 1e-6, 64, 0);
  loop_case("sr_world1_knob1_small", 16384, 1, false, false, -1, 1, 1e-6, 64, 0);
  loop_case("sr_world2_knob0", 8192, 2, false, false, -1, 0, 1e-6, 64, 0);
  loop_case("sr_world2_coarse", 8192, 2, false, false, -1, -1, 1e-6, 64, 64);
  // ---------------------------------------------------------------- reorder, alignment
  { In in; in.shape(1000, 4); in.F.N = 2000; in.env.world = 2; in.env.has_comm = true; evaluate("reorder_world2", in); }
  evaluate("reorder_65537", In().shape(65537, 300));
  evaluate("reorder_65536", In().shape(65536, 300));
  auto align_case = [](const char* name, int world, bool batch, int chain_len, int block, int coarse) {
    In in;
    in.shape(1 << 20, 4096);
    in.env.world = world;
    in.env.has_comm = world > 1;
    in.env.batch_mode = batch;
    in.opt.linear_solver = 1;
    in.opt.pcg_chain_len = chain_len;
    in.opt.pcg_block_poses = block;
    in.opt.pcg_coarse_poses = coarse;
    in.F.rows_per_rank = (int64_t)1 << 20;
    const PlanPre P = plan_pre(in.opt, in.env, (int32_t)in.F.N, 0, nullptr, nullptr);
    printf("case %s refused=%s %s row_align=%" PRId64 "\n", name, P.no ? "pre" : "none", quoted(P.no).c_str(), P.row_align);
  };
  align_case("align_chain64_coarse48_world2", 2, false, 64, 0, 48);
  align_case("align_block4_coarse6_world2", 2, false, 0, 4, 6);
  align_case("align_chain64_coarse48_world1", 1, false, 64, 0, 48);
  align_case("align_chain64_coarse48_world2_batch", 2, true, 64, 0, 48);
  align_case("align_overflow", 2, false, 64, 0, (1 << 29) + 1);   // lcm = 64 (2^29 + 1), twice that > 2^30
  align_case("align_at_limit", 2, false, 64, 0, 1 << 29);         // lcm = 2^29, twice that = 2^30: taken
  // ---------------------------------------------------------------- coarse level (PCG asked for, so that the direct solve does not take the graph)
  for (int64_t NL : {511, 512, 8192, 8193, 131008, 131072}) {
    In in;
    in.shape(NL, 64);
    in.opt.linear_solver = 1;
    evaluate(("coarse_auto_" + std::to_string(NL)).c_str(), in);
  }
  { In in; in.shape(8192, 64); in.opt.linear_solver = 1; in.opt.pcg_rtol = 2e-3; evaluate("coarse_auto_loose", in); }
  { In in; in.shape(8192, 64); in.opt.linear_solver = 1; in.opt.pcg_chain_len = 64; evaluate("coarse_auto_chain", in); }
  { In in; in.shape(8192, 64); in.opt.linear_solver = 1; in.opt.pcg_block_poses = 4; evaluate("coarse_auto_block", in); }
  { In in; in.shape(8192, 64); in.D.m = 20; evaluate("coarse_auto_direct", in); }
  { In in; in.shape(8192, 64); in.F.N = 16384; in.opt.linear_solver = 1; in.env.world = 2; in.env.has_comm = true; evaluate("coarse_auto_world2", in); }
  { In in; in.shape(40000, 300); in.opt.linear_solver = 1; in.opt.pcg_coarse_poses = 16; evaluate("coarse_16_at_40000", in); }
  { In in; in.shape(1024, 8); in.env.batch_mode = true; in.opt.linear_solver = 1; in.opt.pcg_block_poses = 1; in.opt.pcg_coarse_poses = 16; evaluate("coarse_batch", in); }
  for (int Kp : {32, 1024, 1056, 6112}) {   // co_ndot on either side of the explicit inverse's range
    In in;
    in.shape((int64_t)(Kp / 3) * 64, 64);   // K = 3 (Kp / 3) rounds up to Kp
    in.opt.linear_solver = 1;
    in.opt.pcg_coarse_poses = 64;
    evaluate(("coarse_ndot_" + std::to_string(Kp)).c_str(), in);
  }
  // ---------------------------------------------------------------- direct solve: the ladder, silent under auto, an error under linear_solver = 2
  for (int want : {0, 2}) {
    auto ladder = [&](const char* what, In in) {
      in.opt.linear_solver = want;
      in.opt.pcg_coarse_poses = 0;
      evaluate((std::string("direct_") + (want ? "forced_" : "auto_") + what).c_str(), in);
    };
    { In in; in.shape(1000, 4); in.D.m = 20; ladder("ok", in); }
    { In in; in.shape(500, 4); in.F.N = 1000; in.D.N = 1000; in.D.m = 20; in.env.world = 2; in.env.has_comm = true; ladder("world2", in); }
    { In in; in.shape(1000, 4); in.D.m = 20; in.env.has_comm = true; in.env.force_collectives = true; ladder("force", in); }
    { In in; in.shape(1024, 4); in.D.m = 20; in.env.batch_mode = true; in.opt.pcg_block_poses = 1; ladder("batch", in); }   // (a batch takes 3x3 blocks or the chain)
    { In in; in.shape(1000, 4); in.D.m = 20; in.D.info_mode = true; ladder("info", in); }
    { In in; in.shape(1000, 4); in.D.m = 20; in.D.has_constant_pose = false; ladder("no_constant", in); }
    { In in; in.shape(1000, 4); in.D.m = 20; in.D.permuted = true; ladder("permuted", in); }
    { In in; in.shape(1, 1); ladder("n1", in); }
    { In in; in.shape(65537, 300); in.D.m = 20; in.D.permuted = false; ladder("n65537", in); }
    { In in; in.shape(1000, 4); in.D.m = 20; in.D.gap = 417; ladder("gap", in); }
    { In in; in.shape(1000, 4); in.D.m = 2048; ladder("too_many", in); }
    { In in; in.shape(1000, 4); in.D.m = 683; ladder("rank_2049", in); }
    { In in; in.shape(1000, 4); in.D.m = 682; ladder("rank_2046", in); }
    // every refusal at once: the first in the ladder's order wins
    { In in; in.shape(500, 4); in.D.N = 65537; in.D.m = 4000; in.D.gap = 3; in.env.world = 2; in.env.has_comm = true;
      in.D.info_mode = in.D.permuted = true; in.D.has_constant_pose = false; ladder("all_at_once", in); }
  }
  { In in; in.shape(1000, 4); in.D.m = 20; in.opt.pcg_rtol = 1e-7; evaluate("direct_auto_rtol_1e-7", in); }
  { In in; in.shape(1000, 4); in.D.m = 20; in.opt.pcg_rtol = 1e-8; evaluate("direct_auto_rtol_1e-8", in); }
  { In in; in.shape(1000, 4); in.D.m = 20; in.opt.pcg_chain_len = 64; evaluate("direct_auto_explicit_chain", in); }
  { In in; in.shape(1000, 4); in.D.m = 683; in.opt.pcg_rtol = 1e-8; in.opt.pcg_coarse_poses = 0; evaluate("direct_takeover", in); }
  { In in; in.shape(1000, 4); in.D.m = 683; in.opt.pcg_rtol = 1e-8; evaluate("direct_takeover_coarse_auto", in); }
  { In in; in.shape(1000, 4); in.D.m = 20; in.opt.linear_solver = 7; evaluate("direct_bad_option", in); }
  for (int32_t N : {255, 256, 4096, 4097, 6000, 65536}) {
    In in;
    in.shape(N, 4);
    in.D.m = 20;
    in.opt.linear_solver = 2;
    in.opt.pose_ordering = 0;
    evaluate(("direct_sizes_" + std::to_string(N)).c_str(), in);
  }

  // ---------------------------------------------------------------- the partials hold every product grid (licenses k_spmv_1 without a capacity test)
  long n_sweep = 0;
  for (int nt = 0; nt <= 70000; ++nt)
    for (int64_t EL : {(int64_t)0, (int64_t)1000, (int64_t)600000, (int64_t)40000000})
      for (long long pipe : {-1LL, 0LL, 2LL})
        for (long long pad : {-1LL, 0LL, 1LL}) {
          if (nt % 97 != 0 && nt > 4200 && nt < 69900 && (pipe != -1 || pad != -1)) continue;   // (the hooks: densely only around the thresholds)
          In in;
          in.shape(1000, nt);
          in.F.EL = EL;
          in.knob.spmv_pipe = pipe;
          in.knob.pad_tiles = pad;
          PlanPre pre;
          const PlanShard sh = plan_shard(in.opt, in.env, in.knob, pre, in.F);
          CHECK(!sh.no);
          CHECK(sh.own.part_cap == std::max(std::max(sh.own.g_edge, 2048), plan_up8(std::max(1, nt))) + 520);
          CHECK(sh.own.g_spmv >= 1 && sh.own.g_spmv % 8 == 0 && sh.own.g_spmv <= sh.own.part_cap - 520);
          if (sh.own.spmv_one_tile) CHECK(sh.own.g_spmv == plan_up8(nt) && plan_up8(nt) + 8 + 512 <= sh.own.part_cap);
          ++n_sweep;
        }
  printf("sweep part_cap ok: %ld shapes\n", n_sweep);

  // ---------------------------------------------------------------- what every rank must agree on, on a world whose last rank owns no rows
  long n_ranks = 0;
  for (int variant = 0; variant < 4; ++variant) {
    const int world = 3, N = 128;
    pgo_options opt = default_options();
    opt.linear_solver = variant == 3 ? 0 : 1;
    opt.pcg_chain_len = variant == 1 ? 0 : 64;
    opt.pcg_block_poses = variant == 1 ? 4 : 0;
    opt.pcg_coarse_poses = variant == 2 ? 0 : 64;
    opt.pcg_rtol = variant == 0 ? 0.1 : 1e-10;
    opt.halo_exchange = 1;
    opt.halo_overlap = variant != 2;
    Plan first;
    for (int rank = 0; rank < world; ++rank) {
      In in;
      in.opt = opt;
      in.env.world = world;
      in.env.rank = rank;
      in.env.has_comm = true;
      const PlanPre pre = plan_pre(opt, in.env, N, 0, nullptr, nullptr);
      CHECK(!pre.no);
      const int64_t rpr = rows_per_rank(N, world, (int)pre.row_align);
      const int64_t lo = std::min<int64_t>(N, rank * rpr), hi = std::min<int64_t>(N, (rank + 1) * rpr);
      in.F.N = N;
      in.F.E = N - 1;
      in.F.rows_per_rank = rpr;
      in.F.lo = lo;
      in.F.NL = hi - lo;
      in.F.EL = in.F.NL ? in.F.NL + 1 : 0;
      in.F.n_tiles = in.F.NL ? 1 : 0;
      in.F.n_inc = 2 * in.F.NL;
      in.D.N = N;
      if (rank == world - 1) CHECK(in.F.NL == 0);   // the case the property is about
      const Plan P = evaluate("rank", in, false);
      CHECK(!g_refused);
      invariants(in, P);
      if (rank == 0) first = P;
      CHECK(same_all(first, P));
      ++n_ranks;
    }
    if (variant == 0 || variant == 3) CHECK(first.co.on && first.co.co_multi && first.co.co_nagg == 2 && !first.all.use_sr);
    if (variant == 2) CHECK(!first.co.on && first.all.use_halo && !first.own.overlap);
  }
  printf("rank independence ok: %ld plans\n", n_ranks);

  // ---------------------------------------------------------------- structural invariants over pseudo-random facts
  long n_random = 0, n_refused = 0;
  for (int it = 0; it < 6000; ++it) {
    In in;
    const int world = (int)pick({1, 1, 1, 2, 3, 8});
    in.env.world = world;
    in.env.rank = (int)(rnd() % world);
    in.env.force_collectives = world == 1 && rnd() % 8 == 0;
    in.env.has_comm = world > 1 || in.env.force_collectives || rnd() % 4 == 0;
    in.env.batch_mode = world == 1 && rnd() % 6 == 0;
    in.opt.pcg_chain_len = (int)pick({-1, -1, 0, 4, 8, 16, 32, 64, 128, 256, 12, 512});
    in.opt.pcg_block_poses = (int)pick({0, 0, 1, 2, 4, 8, 32, 40});
    in.opt.pcg_coarse_poses = (int)pick({-1, -1, 0, 16, 64, 48, 1000});
    in.opt.pcg_rtol = (double)pick({1, 10, 1000, 1000000, 100000000}) * 1e-10;
    in.opt.linear_solver = (int)pick({0, 0, 1, 2});
    in.opt.pose_ordering = (int)pick({-1, 0, 1});
    in.opt.halo_exchange = (int)(rnd() % 2);
    in.opt.halo_overlap = (int)(rnd() % 2);
    in.knob.pad_tiles = pick({-1, -1, 0, 1});
    in.knob.spmv_pipe = pick({-1, -1, 0, 2});
    in.knob.fused_p = pick({-1, 0});
    in.knob.single_reduction = pick({-1, 0, 1});
    in.knob.direct_fail_at = pick({-1, 3});
    const int64_t N = pick({1, 2, 5, 255, 256, 511, 512, 3500, 8192, 8193, 16384, 16385, 65536, 65537, 131072, 1000000, 3000000});
    const PlanPre pre = plan_pre(in.opt, in.env, (int32_t)N, 0, nullptr, nullptr);
    const int64_t rpr = pre.no ? N : rows_per_rank((int32_t)N, world, (int)pre.row_align);
    const int64_t lo = std::min<int64_t>(N, in.env.rank * rpr), hi = std::min<int64_t>(N, (in.env.rank + 1) * rpr);
    in.F.N = N;
    in.F.rows_per_rank = rpr;
    in.F.lo = lo;
    in.F.NL = hi - lo;
    in.F.E = N + (int64_t)(rnd() % 4000);
    in.F.EL = in.F.NL ? in.F.NL + (int64_t)(rnd() % 4000) : 0;
    in.F.n_inc = 2 * in.F.EL + (int64_t)(rnd() % 64);
    in.F.n_tiles = in.F.NL ? (int)std::max<int64_t>(1, in.F.n_inc / 200) : 0;
    in.F.tiles_fit_wg = rnd() % 8 != 0;
    in.F.tiles_plain = in.F.tiles_fit_wg && rnd() % 4 != 0;
    in.D.N = (int32_t)N;
    in.D.info_mode = rnd() % 8 == 0;
    in.D.has_constant_pose = rnd() % 8 != 0;
    in.D.permuted = pre.reorder;
    in.D.gap = rnd() % 8 == 0 ? (int32_t)(rnd() % (uint64_t)N) : -1;
    in.D.m = (int)pick({0, 1, 20, 682, 683, 2047, 2048, 5000});
    const Plan P = evaluate("random", in, false);
    if (g_refused) {
      ++n_refused;
      continue;
    }
    invariants(in, P);
    ++n_random;
  }
  CHECK(n_random > 2000 && n_refused > 200);
  printf("random invariants ok: %ld plans, %ld refused\n", n_random, n_refused);
  printf("plan ok: %ld checks\n", g_checks);
  return 0;
}
