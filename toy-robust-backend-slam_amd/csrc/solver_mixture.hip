// Max-mixture edges (include/pgo.h, "max-mixture edges"): the table of pgo_set_mixtures / pgo_set_mixture_null, the host half
// of pgo_mixture_select (mixture.hip.h), the outer loop pgo_mixture_solve, and pgo_mixture_eval / pgo_mixture_plan, the serial
// host evaluation of the same statement (mixture.h).
#include "solver_handle.hip.h"
#include "mixture.hip.h"

namespace {

// the table as the C-ABI takes it, checked before anything changes; *n_comp = its component count
int check_mix_table(const std::string& who, int64_t n_edges, int32_t n_mix, const int32_t* edge, const int32_t* comp_ptr,
                    const pgo_mix_component* comps, int64_t* n_comp) {
  *n_comp = 0;
  if (n_mix < 0) return fail(PGO_ERR_INVALID_ARG, who + ": n_mix < 0");
  if (n_mix == 0) return PGO_OK;
  if (!edge || !comp_ptr || !comps) return fail(PGO_ERR_INVALID_ARG, who + ": null pointer");
  if (comp_ptr[0] != 0) return fail(PGO_ERR_INVALID_ARG, who + ": comp_ptr[0] must be 0");
  for (int32_t j = 0; j < n_mix; ++j) {
    const std::string at = who + ": mixture " + std::to_string(j) + " (edge " + std::to_string(edge[j]) + "): ";
    if (edge[j] < 0 || edge[j] >= n_edges) return fail(PGO_ERR_INVALID_ARG, at + "the edge is out of range");
    if (j > 0 && edge[j] <= edge[j - 1]) return fail(PGO_ERR_INVALID_ARG, at + "the edge list must be strictly ascending");
    const int64_t K = (int64_t)comp_ptr[j + 1] - comp_ptr[j];
    if (K < 1 || K > PGO_MIX_MAX_COMPONENTS) return fail(PGO_ERR_INVALID_ARG, at + "1 to 8 components per edge");
    for (int32_t k = comp_ptr[j]; k < comp_ptr[j + 1]; ++k) {
      const pgo_mix_component& c = comps[k];
      if (!(std::isfinite(c.meas[0]) && std::isfinite(c.meas[1]) && std::isfinite(c.meas[2])))
        return fail(PGO_ERR_INVALID_ARG, at + "a mean is not finite");
      if (!(std::isfinite(c.weight) && c.weight > 0.0)) return fail(PGO_ERR_INVALID_ARG, at + "a weight must be finite and > 0");
      if (!(std::isfinite(c.info_scale) && c.info_scale > 0.0 && c.info_scale <= 1.0))
        return fail(PGO_ERR_INVALID_ARG, at + "an info_scale must be finite and in (0, 1]");
    }
  }
  *n_comp = comp_ptr[n_mix];
  return PGO_OK;
}

pgo::MixComp make_comp(const pgo_mix_component& c) {
  pgo::MixComp m;
  m.mx = c.meas[0];
  m.my = c.meas[1];
  m.mt = c.meas[2];
  m.w = c.info_scale;
  m.c = pgo::mix_const(c.weight, c.info_scale);
  m._pad = 0.0;
  return m;
}

int check_loss_classes(const std::string& who, int32_t n_classes, const pgo_loss* losses, pgo::LossClass cls[pgo::MAX_LOSS_CLASSES]) {
  for (int k = 0; k < pgo::MAX_LOSS_CLASSES; ++k) cls[k] = pgo::make_loss_class(PGO_LOSS_TRIVIAL, 0.0);
  if (!losses) return PGO_OK;
  if (n_classes < 1 || n_classes > pgo::MAX_LOSS_CLASSES) return fail(PGO_ERR_INVALID_ARG, who + ": 1 to 4 loss classes");
  for (int32_t k = 0; k < n_classes; ++k) {
    if (!pgo::loss_valid(losses[k])) return fail(PGO_ERR_INVALID_ARG, who + ": loss class " + std::to_string(k) + " is not a valid loss");
    cls[k] = pgo::make_loss_class(losses[k].type, losses[k].a);
  }
  return PGO_OK;
}

// what every [gpu] mixture call needs of its handle
int mix_requires(const pgo_handle* h, const char* who) {
  if (h->opt.method != 0) return fail(PGO_ERR_UNSUPPORTED, std::string(who) + ": METHOD 0 only (the selection takes the place of DCS and of the switches)");
  return h->requires(who, pgo_handle::NO_INFO | pgo_handle::ONE_RANK | pgo_handle::NOT_BATCH);
}

struct MixTabLayout {
  pgo::Layout L;
  pgo::Span<int32_t> loc, ptr, sel;
  pgo::Span<pgo::MixComp> comp;
  MixTabLayout(int64_t n, int64_t n_comp) {
    loc = L.add<int32_t>(n);
    ptr = L.add<int32_t>(n + 1);
    sel = L.add<int32_t>(n);
    comp = L.add<pgo::MixComp>(n_comp);
  }
};

}  // namespace

// the planes as the handle was created with them on the former mixture edges, weight 1 there, no table
int pgo_handle::mixtures_clear() {
  if (mix_n == 0) return PGO_OK;
  HIPC(hipSetDevice(device));
  std::vector<double> plane;
  if (mix_applied) {   // (every other edge holds its created measurement already: the whole planes, bitwise)
    PGOC(upload(e_mx, S.mx));
    PGOC(upload(e_my, S.my));
    PGOC(upload(e_mt, S.mt));
  }
  if (w_set) {
    plane.resize((size_t)S.n_edges_local);
    HIPC(hipMemcpyAsync(plane.data(), e_w, plane.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    PGOC(sync());
    for (int32_t k : mix_loc_h) plane[(size_t)k] = 1.0;
    PGOC(upload(e_w, plane));
  }
  PGOC(sync());   // (`plane` dies with this scope)
  if (mix_applied) {
    ls_traj_ready = false;
    cs_stride = 0;
  }
  mix_n = 0;
  mix_applied = false;
  mix_edge_h.clear();
  mix_loc_h.clear();
  mix_ptr_h.clear();
  solve_is_stale();
  return PGO_OK;
}

int pgo_handle::set_mixtures(const char* who, int32_t n_mix, const int32_t* edge, const int32_t* comp_ptr, const pgo_mix_component* comps) {
  PGOC(mix_requires(this, who));
  int64_t n_comp = 0;
  PGOC(check_mix_table(who, n_edges_total, n_mix, edge, comp_ptr, comps, &n_comp));
  if (n_mix == 0) return mixtures_clear();
  HIPC(hipSetDevice(device));
  const MixTabLayout T(n_mix, n_comp);
  bool moved = false;
  PGOC(reserve(mix_tab, T.L.bytes(), &moved));   // (a failed allocation keeps the old buffer: nothing has changed)
  const int cleared = mixtures_clear();
  if (cleared != PGO_OK) {   // a HIP failure half way: the old table may have gone with the old buffer -- the handle has none
    if (moved) {
      mix_n = 0;
      mix_applied = false;
      mix_edge_h.clear();
      mix_loc_h.clear();
      mix_ptr_h.clear();
    }
    return cleared;
  }
  std::vector<int32_t> local_of((size_t)n_edges_total, -1);
  for (int64_t k = 0; k < S.n_edges_local; ++k) local_of[(size_t)S.orig_edge[k]] = (int32_t)k;
  mix_host.assign((size_t)T.L.bytes(), 0);
  int32_t* loc_h = T.loc.in(mix_host.data());
  int32_t* ptr_h = T.ptr.in(mix_host.data());
  int32_t* sel_h = T.sel.in(mix_host.data());
  pgo::MixComp* comp_h = T.comp.in(mix_host.data());
  mix_edge_h.assign(edge, edge + n_mix);
  mix_ptr_h.assign(comp_ptr, comp_ptr + n_mix + 1);
  mix_loc_h.resize((size_t)n_mix);
  for (int32_t j = 0; j < n_mix; ++j) {
    loc_h[j] = mix_loc_h[(size_t)j] = local_of[(size_t)edge[j]];
    sel_h[j] = -1;
  }
  for (int32_t j = 0; j <= n_mix; ++j) ptr_h[j] = comp_ptr[j];
  for (int64_t k = 0; k < n_comp; ++k) comp_h[k] = make_comp(comps[k]);
  HIPC(hipMemcpyAsync(mix_tab.p, mix_host.data(), (size_t)T.L.bytes(), hipMemcpyHostToDevice, stream));
  PGOC(sync());
  mix_n = n_mix;
  mix_applied = false;
  return PGO_OK;
}

int pgo_handle::set_mixture_null(const uint8_t* select, double pi_null, double scale_null) {
  const char* who = "pgo_set_mixture_null";
  PGOC(mix_requires(this, who));
  if (!(std::isfinite(pi_null) && pi_null > 0.0)) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": pi_null must be finite and > 0");
  if (!(std::isfinite(scale_null) && scale_null > 0.0 && scale_null <= 1.0))
    return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": scale_null must be finite and in (0, 1]");
  const int64_t E = n_edges_total;
  std::vector<int32_t> local_of((size_t)E, -1);
  for (int64_t k = 0; k < S.n_edges_local; ++k) local_of[(size_t)S.orig_edge[k]] = (int32_t)k;
  std::vector<int32_t> edge, ptr(1, 0);
  std::vector<pgo_mix_component> comps;
  for (int64_t e = 0; e < E; ++e) {
    const int32_t k = local_of[(size_t)e];
    if (k < 0 || (S.flags[k] & dev::EDGE_INACTIVE)) continue;
    if (!(select ? select[e] != 0 : kind_local[k] != PGO_EDGE_ODOMETRY)) continue;
    pgo_mix_component c;
    c.meas[0] = S.mx[k];
    c.meas[1] = S.my[k];
    c.meas[2] = S.mt[k];
    c.weight = 1.0;
    c.info_scale = 1.0;
    comps.push_back(c);
    c.weight = pi_null;
    c.info_scale = scale_null;
    comps.push_back(c);
    edge.push_back((int32_t)e);
    ptr.push_back((int32_t)comps.size());
  }
  if (edge.empty()) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": no edge is selected");
  return set_mixtures(who, (int32_t)edge.size(), edge.data(), ptr.data(), comps.data());
}

int pgo_handle::mixture_select(const char* who, int32_t apply, pgo_mix_stats* stats, int32_t* chosen, double* q) {
  PGOC(mix_requires(this, who));
  if (mix_n == 0) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": no mixtures are set (pgo_set_mixtures)");
  HIPC(hipSetDevice(device));
  const int64_t n = mix_n, nc = (n + dev::WG - 1) / dev::WG;
  const MixTabLayout T(n, mix_ptr_h[(size_t)n]);
  pgo::Layout L;
  const auto b_out = L.add<pgo_mix_stats>(1);
  const auto b_part = L.add<double>(dev::MIX_NPART * nc);
  const auto b_chosen = L.add<int32_t>(n);
  const auto b_q = L.add<double>(2 * n);
  bool fresh_plane = false;
  PGOC(reserve(mix_work, L.bytes()));
  if (apply) PGOC(weights_begin(&fresh_plane));
  std::vector<double> ones;
  if (fresh_plane) PGOC(weights_ones(&ones));
  dev::MixtureArgs A;
  A.E = edge_args(poses, nullptr, 0);
  A.mx = e_mx;
  A.my = e_my;
  A.mt = e_mt;
  A.w = apply ? e_w : nullptr;
  A.loc = T.loc.in(mix_tab.p);
  A.ptr = T.ptr.in(mix_tab.p);
  A.comp = T.comp.in(mix_tab.p);
  A.sel = T.sel.in(mix_tab.p);
  A.chosen = b_chosen.in(mix_work.p);
  A.q = b_q.in(mix_work.p);
  A.n = (int32_t)n;
  A.n_chunks = (int32_t)nc;
  A.apply = apply ? 1 : 0;
  A._pad = 0;
  A.part = b_part.in(mix_work.p);
  A.out = b_out.in(mix_work.p);
  const int grid = launch_grid("mix_grid", nc);
  hipLaunchKernelGGL(dev::k_mix_select<>, dim3(grid), dim3(dev::WG), 0, stream, A);
  PGOC(check_launch("k_mix_select"));
  hipLaunchKernelGGL(dev::k_mix_fold<>, dim3(1), dim3(dev::WG), 0, stream, A);
  PGOC(check_launch("k_mix_fold"));
  pgo_mix_stats st;
  HIPC(hipMemcpyAsync(&st, A.out, sizeof st, hipMemcpyDeviceToHost, stream));
  if (chosen) HIPC(hipMemcpyAsync(chosen, A.chosen, (size_t)b_chosen.bytes(), hipMemcpyDeviceToHost, stream));
  if (q) HIPC(hipMemcpyAsync(q, A.q, (size_t)b_q.bytes(), hipMemcpyDeviceToHost, stream));
  PGOC(sync());   // (`ones` dies with this scope)
  if (apply) {
    w_set = true;
    mix_applied = true;
    if (st.n_changed > 0) {   // (a measurement moved: what was derived from the planes once is derived again)
      ls_traj_ready = false;
      cs_stride = 0;
    }
    solve_is_stale();
  }
  if (stats) *stats = st;
  return PGO_OK;
}

int pgo_handle::mixture_selection(int32_t* chosen_out) {
  const char* who = "pgo_get_mixture_selection";
  PGOC(mix_requires(this, who));
  if (!chosen_out) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": null pointer");
  if (mix_n == 0) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": no mixtures are set (pgo_set_mixtures)");
  HIPC(hipSetDevice(device));
  const MixTabLayout T(mix_n, mix_ptr_h[(size_t)mix_n]);
  HIPC(hipMemcpyAsync(chosen_out, T.sel.in(mix_tab.p), (size_t)T.sel.bytes(), hipMemcpyDeviceToHost, stream));
  return sync();
}

int pgo_handle::mixture_solve(const pgo_mixture_options* o_in, pgo_mixture_summary* summary, pgo_mixture_round* rounds, int32_t rounds_cap) {
  const char* who = "pgo_mixture_solve";
  PGOC(mix_requires(this, who));
  pgo_mixture_options o;
  pgo_mixture_options_default(&o);
  if (o_in) o = *o_in;
  if (o.inner_iters < 1 || o.final_iters < 1 || o.max_rounds < 1)
    return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": inner_iters, final_iters and max_rounds must be >= 1");
  if (mix_n == 0) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": no mixtures are set (pgo_set_mixtures)");
  HIPC(hipSetDevice(device));
  const double t_begin = wall_s();
  pgo_mixture_summary G;
  memset(&G, 0, sizeof G);
  G.n_mix = mix_n;
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
  const size_t x_bytes = (size_t)3 * n_full * sizeof(double);
  if (!gnc_x) PGOC(dalloc(&gnc_x, (int64_t)3 * n_full));
  pgo_mix_stats st;
  for (int32_t k = 0; k < o.max_rounds; ++k) {
    const double t0 = wall_s();
    PGOC(mixture_select(who, 1, &st, nullptr, nullptr));                 // 1.
    PGOC(eval_enqueue(poses, sw, 1, false, 0));                         // 2. the handle's own cost under the selection
    PGOC(fetch_scal(0, 2));
    pgo_mixture_round R;
    memset(&R, 0, sizeof R);
    R.objective = h_scal[0] + st.offset;
    R.n_changed = st.n_changed;
    for (int i = 0; i < PGO_MIX_MAX_COMPONENTS; ++i) R.count[i] = st.count[i];
    G.rounds = k + 1;
    G.offset = st.offset;
    G.objective = R.objective;
    const bool stop = k > 0 && st.n_changed == 0;                        // 3.
    if (!stop) {                                                         // 4.
      HIPC(hipMemcpyAsync(gnc_x, poses, x_bytes, hipMemcpyDeviceToDevice, stream));
      const int s1 = solve(o.inner_iters);
      if (s1 != PGO_OK || termination == PGO_TERM_FAILURE) {
        (void)hipMemcpyAsync(poses, gnc_x, x_bytes, hipMemcpyDeviceToDevice, stream);
        (void)hipStreamSynchronize(stream);
        solve_is_stale();
        return finish(s1 != PGO_OK ? s1 : fail(PGO_ERR_NUMERIC, std::string(who) + ": the inner solve of round " + std::to_string(k + 1) + " failed"));
      }
      R.lm_iterations = iter;
      R.lm_termination = termination;
    }
    R.seconds = wall_s() - t0;
    if (rounds && k < rounds_cap) rounds[k] = R;
    if (opt.verbose) {
      printf("mixture round %3d  F % .9e  changed %6d  lm %d (%d)  count", k + 1, R.objective, R.n_changed, R.lm_iterations, R.lm_termination);
      for (int i = 0; i < PGO_MIX_MAX_COMPONENTS; ++i) printf(" %d", R.count[i]);
      printf("\n");
    }
    if (stop) break;
    if (k + 1 == o.max_rounds) G.hit_max_rounds = 1;
  }
  const int s5 = solve(o.final_iters);
  if (s5 != PGO_OK) return finish(s5);
  if (termination == PGO_TERM_FAILURE) return finish(fail(PGO_ERR_NUMERIC, std::string(who) + ": the final solve failed"));
  G.objective = cost + G.offset;
  const int s6 = mixture_select(who, 0, &st, nullptr, nullptr);
  if (s6 == PGO_OK) G.n_would_change = st.n_changed;
  return finish(s6);
}

extern "C" {

void pgo_mixture_options_default(pgo_mixture_options* o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->inner_iters = 2;
  o->final_iters = 50;
  o->max_rounds = 50;
}

int pgo_mixture_eval(int32_t n_comp, const pgo_mix_component* comps, const double* s, const pgo_loss* loss, int32_t* chosen, double* q_best,
                     double* margin) {
  const std::string who = "pgo_mixture_eval";
  if (!comps || !s || !chosen || !q_best || !margin) return fail(PGO_ERR_INVALID_ARG, who + ": null pointer");
  const int32_t edge0 = 0, ptr[2] = {0, n_comp};
  int64_t nk = 0;
  if (n_comp < 1 || n_comp > PGO_MIX_MAX_COMPONENTS) return fail(PGO_ERR_INVALID_ARG, who + ": 1 to 8 components");
  PGOC(check_mix_table(who, 1, 1, &edge0, ptr, comps, &nk));
  pgo::LossClass cls[pgo::MAX_LOSS_CLASSES];
  PGOC(check_loss_classes(who, 1, loss, cls));
  pgo::MixPick P = pgo::mix_pick_begin();
  for (int32_t k = 0; k < n_comp; ++k) {
    const pgo::MixComp m = make_comp(comps[k]);
    pgo::mix_pick_take(P, k, pgo::mix_q(cls[0], m.w, m.c, s[k]));
  }
  *chosen = P.k;
  *q_best = pgo::mix_pick_best(P);
  *margin = pgo::mix_pick_margin(P);
  return PGO_OK;
}

int pgo_mixture_plan(int32_t n_poses, const double* poses, int32_t n_edges, const int32_t* ia, const int32_t* ib, int32_t n_mix,
                     const int32_t* edge, const int32_t* comp_ptr, const pgo_mix_component* comps, int32_t n_classes, const pgo_loss* losses,
                     const uint8_t* mix_class, const int32_t* prev, const uint8_t* active, int32_t* chosen, double* q, pgo_mix_stats* stats) {
  const std::string who = "pgo_mixture_plan";
  if (n_poses < 0 || n_edges < 0) return fail(PGO_ERR_INVALID_ARG, who + ": negative size");
  if (n_mix > 0 && (!poses || !ia || !ib || !chosen || !q)) return fail(PGO_ERR_INVALID_ARG, who + ": null pointer");
  int64_t n_comp = 0;
  PGOC(check_mix_table(who, n_edges, n_mix, edge, comp_ptr, comps, &n_comp));
  pgo::LossClass cls[pgo::MAX_LOSS_CLASSES];
  PGOC(check_loss_classes(who, n_classes, losses, cls));
  for (int32_t j = 0; j < n_mix; ++j) {
    const int32_t e = edge[j];
    if (ia[e] < 0 || ia[e] >= n_poses || ib[e] < 0 || ib[e] >= n_poses)
      return fail(PGO_ERR_INVALID_ARG, who + ": edge " + std::to_string(e) + ": an endpoint is out of range");
    if (mix_class && (!losses ? mix_class[j] != 0 : mix_class[j] >= n_classes))
      return fail(PGO_ERR_INVALID_ARG, who + ": mixture " + std::to_string(j) + ": the loss class is out of range");
  }
  pgo_mix_stats st;
  memset(&st, 0, sizeof st);
  st.n_mix = n_mix;
  for (int32_t j = 0; j < n_mix; ++j) {
    const int32_t e = edge[j], before = prev ? prev[j] : -1;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    chosen[j] = before;
    q[2 * j] = q[2 * j + 1] = nan;
    if (active && !active[j]) {
      ++st.n_inactive;
      continue;
    }
    const double* pa = poses + 3 * (int64_t)ia[e];
    const double* pb = poses + 3 * (int64_t)ib[e];
    const pgo::LossClass L = cls[mix_class ? mix_class[j] : 0];
    pgo::MixPick P = pgo::mix_pick_begin();
    double c_best = 0.0;
    for (int32_t k = comp_ptr[j]; k < comp_ptr[j + 1]; ++k) {
      const pgo::MixComp m = make_comp(comps[k]);
      double ex, ey, sind;
      pgo::edge_plain<false>(pa[0], pa[1], pa[2], pb[0], pb[1], pb[2], m.mx, m.my, m.mt, ex, ey, sind, nullptr);
      const double et = asin(sind);
      const int was = P.k;
      pgo::mix_pick_take(P, k - comp_ptr[j], pgo::mix_q(L, m.w, m.c, ex * ex + ey * ey + et * et));
      if (P.k != was) c_best = m.c;
    }
    if (P.k < 0) {
      ++st.n_nonfinite;
      continue;
    }
    chosen[j] = P.k;
    q[2 * j] = pgo::mix_pick_best(P);
    q[2 * j + 1] = pgo::mix_pick_margin(P);
    if (P.k != before) ++st.n_changed;
    st.offset += c_best;
    st.mix_cost += P.q_best;
    ++st.count[P.k];
  }
  if (stats) *stats = st;
  return PGO_OK;
}

int pgo_set_mixtures(pgo_t* h, int32_t n_mix, const int32_t* edge, const int32_t* comp_ptr, const pgo_mix_component* comps) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_set_mixtures: null handle");
  return h->set_mixtures("pgo_set_mixtures", n_mix, edge, comp_ptr, comps);
}

int pgo_set_mixture_null(pgo_t* h, const uint8_t* select_or_null, double pi_null, double scale_null) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_set_mixture_null: null handle");
  return h->set_mixture_null(select_or_null, pi_null, scale_null);
}

int pgo_mixture_select(pgo_t* h, int32_t apply, pgo_mix_stats* stats_or_null, int32_t* chosen_or_null, double* q_or_null) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_mixture_select: null handle");
  return h->mixture_select("pgo_mixture_select", apply, stats_or_null, chosen_or_null, q_or_null);
}

int pgo_get_mixture_selection(pgo_t* h, int32_t* chosen_out) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_get_mixture_selection: null handle");
  return h->mixture_selection(chosen_out);
}

int pgo_mixture_solve(pgo_t* h, const pgo_mixture_options* opt_or_null, pgo_mixture_summary* summary_or_null, pgo_mixture_round* rounds_or_null,
                      int32_t rounds_cap) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_mixture_solve: null handle");
  return h->mixture_solve(opt_or_null, summary_or_null, rounds_or_null, rounds_cap);
}

}  // extern "C"
