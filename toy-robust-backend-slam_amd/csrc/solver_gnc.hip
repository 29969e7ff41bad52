// The edge weight plane and graduated non-convexity (include/pgo.h, "edge weight plane", "graduated non-convexity"): the host
// halves of pgo_set_edge_weights / pgo_get_edge_weights, pgo_gnc_update (gnc.hip.h) and the outer loop pgo_gnc_solve, and
// pgo_gnc_weight_eval, the serial host evaluation of the same statement (gnc.h).
#include "solver_handle.hip.h"
#include "gnc.hip.h"

int pgo_handle::weights_alloc() {
  const int64_t EL = S.n_edges_local;   // (one rank: every edge is local)
  if (!e_w) PGOC(dalloc(&e_w, EL));
  return PGO_OK;
}

// every weight is checked before anything changes; then the plane is rewritten in the local edge order and the running solve
// (if any) is stale.  NULL: no plane -- K1 is back on the instantiations the handle's losses and mask ask for.
int pgo_handle::set_edge_weights(const double* w) {
  const char* who = "pgo_set_edge_weights";
  PGOC(requires(who, PLAIN_HANDLE));
  const int64_t EL = S.n_edges_local;
  if (w)
    for (int64_t e = 0; e < n_edges_total; ++e)
      if (!(std::isfinite(w[e]) && w[e] >= 0.0 && w[e] <= 1.0))
        return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": edge " + std::to_string(e) + ": the weight must be finite and in [0, 1]");
  HIPC(hipSetDevice(device));
  if (w && EL > 0) {
    PGOC(weights_alloc());
    std::vector<double> loc((size_t)EL);
    for (int64_t k = 0; k < EL; ++k) loc[k] = w[S.orig_edge[k]];
    PGOC(upload(e_w, loc));
    PGOC(sync());   // (`loc` dies with this scope)
  }
  w_set = w != nullptr && EL > 0;
  solve_is_stale();
  return PGO_OK;
}

int pgo_handle::get_edge_weights(double* out) {
  const char* who = "pgo_get_edge_weights";
  PGOC(requires(who, PLAIN_HANDLE));
  if (!out) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": null pointer");
  const int64_t EL = S.n_edges_local;
  if (!w_set) {
    for (int64_t e = 0; e < n_edges_total; ++e) out[e] = 1.0;
    return PGO_OK;
  }
  HIPC(hipSetDevice(device));
  std::vector<double> loc((size_t)EL);
  HIPC(hipMemcpyAsync(loc.data(), e_w, (size_t)EL * sizeof(double), hipMemcpyDeviceToHost, stream));
  PGOC(sync());
  for (int64_t k = 0; k < EL; ++k) out[S.orig_edge[k]] = loc[k];
  return PGO_OK;
}

// reset_selected (pgo_gnc_solve's step 1): every selected weight <- 1, measured there
int pgo_handle::gnc_update(double cbar, double mu, const uint8_t* select, bool reset_selected, pgo_gnc_stats* out) {
  const char* who = "pgo_gnc_update";
  PGOC(requires(who, PLAIN_HANDLE));
  if (!(std::isfinite(cbar) && cbar > 0.0)) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": cbar must be finite and > 0");
  if (std::isnan(mu) || std::isinf(mu)) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": mu is not finite");
  const int mode = reset_selected ? 2 : (mu > 0.0 ? 1 : 0);
  pgo_gnc_stats st;
  memset(&st, 0, sizeof st);
  st.s_max = -1.0;
  const int64_t E = n_edges_total, EL = S.n_edges_local;
  if (EL == 0) {
    if (out) *out = st;
    return PGO_OK;
  }
  HIPC(hipSetDevice(device));
  // ---- buffers, before anything changes: gnc_buf = stats | partials | caller's edge -> local edge | select bytes
  const int64_t nc = (E + dev::WG - 1) / dev::WG;
  pgo::Layout L;
  const auto b_out = L.add<pgo_gnc_stats>(1);
  const auto b_part = L.add<double>(dev::GNC_NPART * nc);
  const auto b_loc = L.add<int32_t>(E);   // (the upload: b_loc to b_sel, or b_sel alone)
  const auto b_sel = L.add<uint8_t>(E);
  bool table_stale = false, fresh_plane = false;   // (a handle's E never changes: the table is written when the buffer is made)
  PGOC(reserve(gnc_buf, L.bytes(), &table_stale));
  if (mode != 0) PGOC(weights_begin(&fresh_plane));
  // ---- upload: the resolved selection (selected AND active), the edge table once, an all-ones plane at its first use
  std::vector<uint8_t> host((size_t)L.bytes(), 0);
  int32_t* loc_h = b_loc.in(host.data());
  uint8_t* sel_h = b_sel.in(host.data());
  for (int64_t k = 0; k < EL; ++k) {
    const int64_t e = S.orig_edge[k];
    loc_h[e] = (int32_t)k;
    const bool active = !(S.flags[k] & dev::EDGE_INACTIVE);
    sel_h[e] = (active && (select ? select[e] != 0 : kind_local[k] != PGO_EDGE_ODOMETRY)) ? 1 : 0;
  }
  if (table_stale) HIPC(hipMemcpyAsync(b_loc.in(gnc_buf.p), loc_h, (size_t)pgo::run_bytes(b_loc, b_sel), hipMemcpyHostToDevice, stream));
  else HIPC(hipMemcpyAsync(b_sel.in(gnc_buf.p), sel_h, (size_t)b_sel.bytes(), hipMemcpyHostToDevice, stream));
  std::vector<double> ones;
  if (fresh_plane) PGOC(weights_ones(&ones));
  dev::GncArgs A;
  A.E = edge_args(poses, nullptr, 0);
  A.loc = b_loc.in(gnc_buf.p);
  A.select = b_sel.in(gnc_buf.p);
  A.w = (mode != 0 || w_set) ? e_w : nullptr;
  A.n = (int32_t)E;
  A.n_chunks = (int32_t)nc;
  A.mode = mode;
  A._pad = 0;
  A.c2 = cbar * cbar;
  A.mu = mu;
  A.part = b_part.in(gnc_buf.p);
  A.out = b_out.in(gnc_buf.p);
  const int grid = launch_grid("gnc_grid", nc);
  hipLaunchKernelGGL(dev::k_gnc_update<>, dim3(grid), dim3(dev::WG), 0, stream, A);
  PGOC(check_launch("k_gnc_update"));
  hipLaunchKernelGGL(dev::k_gnc_fold<>, dim3(1), dim3(dev::WG), 0, stream, A);
  PGOC(check_launch("k_gnc_fold"));
  HIPC(hipMemcpyAsync(&st, A.out, sizeof st, hipMemcpyDeviceToHost, stream));
  PGOC(sync());   // (`host` and `ones` die with this scope)
  if (mode != 0) {
    w_set = true;
    solve_is_stale();
  }
  if (out) *out = st;
  return PGO_OK;
}

namespace {
int check_gnc_options(const char* who, const pgo_gnc_options* o) {
  if (!o) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": null options (cbar has no default)");
  if (!(std::isfinite(o->cbar) && o->cbar > 0.0)) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": cbar must be finite and > 0");
  if (!(std::isfinite(o->mu_factor) && o->mu_factor > 1.0)) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": mu_factor must be finite and > 1");
  if (o->inner_iters < 1 || o->final_iters < 1 || o->max_rounds < 1)
    return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": inner_iters, final_iters and max_rounds must be >= 1");
  return PGO_OK;
}
}  // namespace

int pgo_handle::gnc_solve(const pgo_gnc_options* o, pgo_gnc_summary* summary, pgo_gnc_round* rounds, int32_t rounds_cap) {
  const char* who = "pgo_gnc_solve";
  PGOC(requires(who, PLAIN_HANDLE));
  if (opt.method != 0) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": METHOD 0 only (the weights take the place of DCS)");
  PGOC(check_gnc_options(who, o));
  HIPC(hipSetDevice(device));
  const double t_begin = wall_s();
  const double c2 = o->cbar * o->cbar;
  pgo_gnc_summary G;
  memset(&G, 0, sizeof G);
  // an LM solve of at most `iters` iterations from the current poses: pgo_solve under that iteration limit
  auto solve = [&](int32_t iters) -> int {
    const int32_t keep = opt.max_iters;
    opt.max_iters = std::min(keep, iters);
    int st = lm_begin();
    bool stop = false;
    while (st == PGO_OK && !stop) st = lm_iteration(&stop);
    opt.max_iters = keep;
    if (st == PGO_OK) lm_done = true;
    return st;
  };
  auto finish = [&](int st) -> int {
    fill_summary(&G.final_solve);
    G.seconds_total = wall_s() - t_begin;
    if (summary) *summary = G;
    return st;
  };
  // the poses a round starts from, for a failed inner solve (one buffer of the handle's own, kept)
  const size_t x_bytes = (size_t)3 * n_full * sizeof(double);
  pgo_gnc_stats st;
  PGOC(gnc_update(o->cbar, 0.0, o->select, true, &st));   // 1. selected weights <- 1, rmax2
  G.n_selected = st.n_selected;
  G.rmax2 = st.s_max;
  if (st.n_nonfinite > 0) return fail(PGO_ERR_NUMERIC, std::string(who) + ": a selected edge has a non-finite residual at the starting poses");
  if (!(2.0 * st.s_max > c2)) {   // 2. nothing to graduate (or nothing selected: s_max = -1)
    const int s2 = solve(o->final_iters);
    if (s2 == PGO_OK && termination == PGO_TERM_FAILURE) return finish(fail(PGO_ERR_NUMERIC, std::string(who) + ": the solve failed"));
    return finish(s2);
  }
  if (!gnc_x) PGOC(dalloc(&gnc_x, (int64_t)3 * n_full));
  double mu = pgo::gnc_mu0(c2, st.s_max);   // 3.
  G.mu0 = mu;
  for (int32_t k = 0; k < o->max_rounds; ++k) {   // 4.
    const double t0 = wall_s();
    HIPC(hipMemcpyAsync(gnc_x, poses, x_bytes, hipMemcpyDeviceToDevice, stream));
    const int s1 = solve(o->inner_iters);
    if (s1 != PGO_OK || termination == PGO_TERM_FAILURE) {
      (void)hipMemcpyAsync(poses, gnc_x, x_bytes, hipMemcpyDeviceToDevice, stream);
      (void)hipStreamSynchronize(stream);
      solve_is_stale();
      G.mu_last = mu;
      return finish(s1 != PGO_OK ? s1 : fail(PGO_ERR_NUMERIC, std::string(who) + ": the inner solve of round " + std::to_string(k + 1) + " failed"));
    }
    const int32_t lm_iters = iter, lm_term = termination;
    PGOC(gnc_update(o->cbar, mu, o->select, false, &st));
    pgo_gnc_round R;
    memset(&R, 0, sizeof R);
    R.mu = mu;
    R.weighted_cost = 0.5 * st.weighted_sum;
    R.n_nonbinary = st.n_nonbinary;
    R.n_zero = st.n_zero;
    R.lm_iterations = lm_iters;
    R.lm_termination = lm_term;
    R.seconds = wall_s() - t0;
    if (rounds && k < rounds_cap) rounds[k] = R;
    G.rounds = k + 1;
    G.mu_last = mu;
    G.n_zero = st.n_zero;
    if (opt.verbose)
      printf("gnc round %3d  mu % .6e  weighted cost % .6e  0<w<1 %6d  w=0 %6d  lm %d (%d)\n", k + 1, mu, R.weighted_cost, R.n_nonbinary, R.n_zero,
             lm_iters, lm_term);
    if (st.n_nonbinary == 0 && k > 0) break;
    if (k + 1 == o->max_rounds) G.hit_max_rounds = 1;
    mu *= o->mu_factor;
  }
  const int s5 = solve(o->final_iters);   // 5.
  if (s5 == PGO_OK && termination == PGO_TERM_FAILURE) return finish(fail(PGO_ERR_NUMERIC, std::string(who) + ": the final solve failed"));
  return finish(s5);
}

extern "C" {

void pgo_gnc_options_default(pgo_gnc_options* o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->cbar = 0.0;
  o->mu_factor = 1.4;
  o->inner_iters = 5;
  o->final_iters = 50;
  o->max_rounds = 100;
  o->select = nullptr;
}

int pgo_gnc_weight_eval(double cbar, double mu, int32_t n, const double* s, double* w_out) {
  const char* who = "pgo_gnc_weight_eval";
  if (n < 0 || (n > 0 && (!s || !w_out))) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": bad argument");
  if (!(std::isfinite(cbar) && cbar > 0.0)) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": cbar must be finite and > 0");
  if (!(std::isfinite(mu) && mu > 0.0)) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": mu must be finite and > 0");
  const double c2 = cbar * cbar;
  for (int32_t i = 0; i < n; ++i) w_out[i] = pgo::gnc_tls_weight(c2, mu, s[i]);
  return PGO_OK;
}

int pgo_set_edge_weights(pgo_t* h, const double* w_or_null) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_set_edge_weights: null handle");
  return h->set_edge_weights(w_or_null);
}

int pgo_get_edge_weights(pgo_t* h, double* w_out) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_get_edge_weights: null handle");
  return h->get_edge_weights(w_out);
}

int pgo_gnc_update(pgo_t* h, double cbar, double mu, const uint8_t* select_or_null, pgo_gnc_stats* out) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_gnc_update: null handle");
  return h->gnc_update(cbar, mu, select_or_null, false, out);
}

int pgo_gnc_solve(pgo_t* h, const pgo_gnc_options* opt, pgo_gnc_summary* summary, pgo_gnc_round* rounds, int32_t rounds_cap) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_gnc_solve: null handle");
  return h->gnc_solve(opt, summary, rounds, rounds_cap);
}

}  // extern "C"
