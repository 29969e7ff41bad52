// Loop support (include/pgo.h, "loop support"): pgo_loop_support -- the host half of the kernels of loop_support.hip.h -- and
// pgo_loop_support_plan, the serial host statement of the same test (loop_support.h).  The measurements stay where they are,
// in the handle's local edge order; the kernels walk the caller's numbering through the tables of pgo_coarsen (built once per
// handle) and through the table of the selection (the loops sorted by (lo, edge index), built once per selection).  Without
// apply the call touches neither the LM state, the record buffer, the poses nor the weight plane.
#include "solver_handle.hip.h"
#include "loop_support.hip.h"

namespace {
int check_options(const std::string& who, const pgo_loop_support_options* o) {
  if (!o) return fail(PGO_ERR_INVALID_ARG, who + ": null options");
  if (o->window < 1 || o->window > PGO_LOOP_SUPPORT_MAX_WINDOW)
    return fail(PGO_ERR_INVALID_ARG, who + ": window must be 1.." + std::to_string(PGO_LOOP_SUPPORT_MAX_WINDOW));
  if (!(std::isfinite(o->tol_xy) && o->tol_xy > 0.0 && std::isfinite(o->tol_th) && o->tol_th > 0.0))
    return fail(PGO_ERR_INVALID_ARG, who + ": tol_xy and tol_th must be finite and > 0");
  if (o->min_support < 1) return fail(PGO_ERR_INVALID_ARG, who + ": min_support must be >= 1");
  return PGO_OK;
}
}  // namespace

// The trajectory T (loop_support.h), once per handle: its buffer, before anything is enqueued, and its three launches.  The
// caller sets ls_traj_ready after its synchronisation.  Shared with pgo_chordal_init, whose start it is.
int pgo_handle::support_trajectory_alloc() {
  const int64_t N = S.n_poses, P = pgo::SUPPORT_POSE, n_seg = (N + dev::SUPPORT_SEG - 1) / dev::SUPPORT_SEG;
  if (!ls_traj) PGOC(dalloc(&ls_traj, (N + 2 * n_seg) * P));
  return PGO_OK;
}
int pgo_handle::support_trajectory_enqueue() {
  const int64_t N = S.n_poses, P = pgo::SUPPORT_POSE, n_seg = (N + dev::SUPPORT_SEG - 1) / dev::SUPPORT_SEG;
  auto grid_for = [&](int64_t units) { return launch_grid("support_grid", units); };
  auto per_lane = [&](int64_t n) { return grid_for((n + dev::WG - 1) / dev::WG); };
  if (!ls_traj_ready) {
    dev::SupportTrajArgs A;
    A.mx = e_mx;
    A.my = e_my;
    A.mt = e_mt;
    A.chain = cs_chain();
    A.n = (int32_t)N;
    A.n_seg = (int32_t)n_seg;
    A.T = ls_traj;
    A.Cend = ls_traj + N * P;
    A.Tkey = ls_traj + (N + n_seg) * P;
    hipLaunchKernelGGL(dev::k_support_segments<>, dim3(grid_for((n_seg + dev::WG / 64 - 1) / (dev::WG / 64))), dim3(dev::WG), 0, stream, A);
    PGOC(check_launch("k_support_segments"));
    hipLaunchKernelGGL(dev::k_support_keys<>, dim3(1), dim3(dev::WG), 0, stream, A);
    PGOC(check_launch("k_support_keys"));
    hipLaunchKernelGGL(dev::k_support_traj<>, dim3(per_lane(N)), dim3(dev::WG), 0, stream, A);
    PGOC(check_launch("k_support_traj"));
  }
  return PGO_OK;
}

int pgo_handle::loop_support(const pgo_loop_support_options* o, const uint8_t* select, pgo_loop_support_record* out, pgo_loop_support_stats* stats) {
  const char* who = "pgo_loop_support";
  PGOC(requires(who, ONE_RANK | NOT_BATCH));
  PGOC(check_options(who, o));
  if (o->apply) PGOC(requires(who, PLAIN_HANDLE));
  const int64_t N = S.n_poses, E = n_edges_total;
  if (N < 2) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": n_poses must be >= 2");
  HIPC(hipSetDevice(device));
  PGOC(coarsen_tables(who, false));
  // ---- the resolved selection, and its measurements and the chain's checked
  std::vector<uint8_t> sel((size_t)E);
  int64_t bad = -1;
  for (int64_t e = 0; e < E; ++e) {
    const int32_t l = cs_loc_h[e];
    sel[e] = l >= 0 && (select ? select[e] != 0 : kind_local[l] != PGO_EDGE_ODOMETRY);
  }
  if (cs_bad >= 0)   // (rare: look at the edges that matter, in the caller's order)
    for (int64_t k = 0; k < S.n_edges_local; ++k) {
      const int64_t e = S.orig_edge[k];
      if ((sel[e] || cs_loc_h[e] < 0) && !pgo::coarsen_finite3(S.mx[k], S.my[k], S.mt[k]) && (bad < 0 || e < bad)) bad = e;
    }
  if (bad >= 0) return not_finite(who, bad);
  // ---- buffers, before anything is enqueued or changed
  const int64_t P = pgo::SUPPORT_POSE;
  const bool new_table = !ls_tab_ready || sel != ls_sel_h;
  std::vector<int32_t> s_edge, s_lo, s_hi, first, slot_of;
  int64_t n_sel = ls_n_sel;
  if (new_table) {
    pgo::support_sort(N, E, cs_ea_h.data(), cs_eb_h.data(), sel.data(), &s_edge, &s_lo, &s_hi, &first, &slot_of);
    n_sel = (int64_t)s_edge.size();
  }
  const int64_t nc = (E + dev::WG - 1) / dev::WG;
  pgo::Layout LT, LW;
  const auto t_edge = LT.add<int32_t>(n_sel), t_lo = LT.add<int32_t>(n_sel), t_hi = LT.add<int32_t>(n_sel);   // (the host writes
  const auto t_first = LT.add<int32_t>(N + 1), t_slot = LT.add<int32_t>(E);   // t_edge to t_slot, k_support_prepare the rest)
  const auto t_minv = LT.add<double>(n_sel * P);
  const auto w_stats = LW.add<pgo_loop_support_stats>(1);
  const auto w_part = LW.add<double>(dev::SUPPORT_NPART * nc), w_q = LW.add<double>(n_sel);
  const auto w_out = LW.add<pgo_loop_support_record>(E);
  const auto w_cnt = LW.add<int32_t>(3 * n_sel);
  PGOC(support_trajectory_alloc());
  if (new_table) ls_tab_ready = false;   // (the buffer may move and is rewritten)
  PGOC(reserve(ls_tab, LT.bytes()));
  PGOC(reserve(ls_work, LW.bytes()));
  bool fresh_plane = false;
  if (o->apply) PGOC(weights_begin(&fresh_plane));
  if (out) ls_host.resize((size_t)w_out.bytes());
  auto grid_for = [&](int64_t units) { return launch_grid("support_grid", units); };
  auto per_lane = [&](int64_t n) { return grid_for((n + dev::WG - 1) / dev::WG); };
  PGOC(support_trajectory_enqueue());
  dev::SupportArgs A;
  A.mx = e_mx;
  A.my = e_my;
  A.mt = e_mt;
  A.ea = cs_ea();
  A.eb = cs_eb();
  A.eloc = cs_eloc();
  A.T = ls_traj;
  A.s_edge = t_edge.in(ls_tab.p);
  A.s_lo = t_lo.in(ls_tab.p);
  A.s_hi = t_hi.in(ls_tab.p);
  A.first = t_first.in(ls_tab.p);
  A.slot_of = t_slot.in(ls_tab.p);
  A.minv = t_minv.in(ls_tab.p);
  A.n = (int32_t)N;
  A.n_edges = (int32_t)E;
  A.n_sel = (int32_t)n_sel;
  A.n_chunks = (int32_t)nc;
  A.window = o->window;
  A.min_support = o->min_support;
  A.apply = o->apply ? 1 : 0;
  A._pad = 0;
  A.txy2 = o->tol_xy * o->tol_xy;
  A.tth2 = o->tol_th * o->tol_th;
  A.r_cnt = w_cnt.in(ls_work.p);
  A.r_q = w_q.in(ls_work.p);
  A.out = w_out.in(ls_work.p);
  A.w = o->apply ? e_w : nullptr;
  A.part = w_part.in(ls_work.p);
  A.stats = w_stats.in(ls_work.p);
  // ---- the table of the selection, once per selection
  std::vector<uint8_t> img;
  if (new_table) {
    img.resize((size_t)pgo::run_bytes(t_edge, t_slot));   // (the run starts the buffer: the spans address its image as they stand)
    if (n_sel) {
      memcpy(t_edge.in(img.data()), s_edge.data(), (size_t)t_edge.bytes());
      memcpy(t_lo.in(img.data()), s_lo.data(), (size_t)t_lo.bytes());
      memcpy(t_hi.in(img.data()), s_hi.data(), (size_t)t_hi.bytes());
    }
    memcpy(t_first.in(img.data()), first.data(), (size_t)t_first.bytes());
    if (E) memcpy(t_slot.in(img.data()), slot_of.data(), (size_t)t_slot.bytes());
    HIPC(hipMemcpyAsync(t_edge.in(ls_tab.p), img.data(), img.size(), hipMemcpyHostToDevice, stream));
    if (n_sel) {
      hipLaunchKernelGGL(dev::k_support_prepare<>, dim3(per_lane(n_sel)), dim3(dev::WG), 0, stream, A);
      PGOC(check_launch("k_support_prepare"));
    }
  }
  std::vector<double> ones;
  if (fresh_plane) PGOC(weights_ones(&ones));
  if (n_sel) {
    hipLaunchKernelGGL(dev::k_loop_support<>, dim3(per_lane(n_sel)), dim3(dev::WG), 0, stream, A);
    PGOC(check_launch("k_loop_support"));
  }
  hipLaunchKernelGGL(dev::k_support_finish<>, dim3(grid_for(nc)), dim3(dev::WG), 0, stream, A);
  PGOC(check_launch("k_support_finish"));
  hipLaunchKernelGGL(dev::k_support_fold<>, dim3(1), dim3(dev::WG), 0, stream, A);
  PGOC(check_launch("k_support_fold"));
  pgo_loop_support_stats st;
  memset(&st, 0, sizeof st);
  HIPC(hipMemcpyAsync(&st, A.stats, sizeof st, hipMemcpyDeviceToHost, stream));
  if (out && E) HIPC(hipMemcpyAsync(ls_host.data(), A.out, ls_host.size(), hipMemcpyDeviceToHost, stream));
  PGOC(sync());   // (`img` and `ones` die with this scope)
  ls_traj_ready = true;
  if (new_table) {
    ls_sel_h.swap(sel);
    ls_n_sel = (int32_t)n_sel;
    ls_tab_ready = true;
  }
  if (o->apply) {
    w_set = true;
    solve_is_stale();
  }
  if (out && E) memcpy(out, ls_host.data(), ls_host.size());
  if (stats) *stats = st;
  return PGO_OK;
}

extern "C" {

void pgo_loop_support_options_default(pgo_loop_support_options* o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->window = 32;
  o->min_support = 1;
  o->apply = 0;
  o->tol_xy = 0.1;
  o->tol_th = 0.05;
}

int pgo_loop_support_plan(int32_t n_poses, int32_t n_edges, const int32_t* ia, const int32_t* ib, const double* meas, const uint8_t* kind,
                          const uint8_t* select, const pgo_loop_support_options* o, pgo_loop_support_record* out, pgo_loop_support_stats* stats,
                          double* T_or_null) {
  const std::string who = "pgo_loop_support_plan";
  if (n_edges < 0 || !ia || !ib || !meas || !kind || !out || !stats) return fail(PGO_ERR_INVALID_ARG, who + ": null pointer or negative count");
  if (n_poses < 2) return fail(PGO_ERR_INVALID_ARG, who + ": n_poses must be >= 2");
  PGOC(check_options(who, o));
  const int64_t N = n_poses, E = n_edges, P = pgo::SUPPORT_POSE;
  for (int64_t e = 0; e < E; ++e)
    if (ia[e] < 0 || ia[e] >= N || ib[e] < 0 || ib[e] >= N) return fail(PGO_ERR_INVALID_ARG, who + ": edge " + std::to_string(e) + ": endpoint out of range");
  std::vector<int32_t> chain;
  const int32_t gap = pgo::pick_chain_edges(n_poses, E, ia, ib, &chain);
  if (gap >= 0) return no_chain(who, gap);
  std::vector<uint8_t> sel((size_t)E);
  for (int64_t e = 0; e < E; ++e) sel[e] = select ? select[e] != 0 : kind[e] != PGO_EDGE_ODOMETRY;
  for (int64_t i = 0; i + 1 < N; ++i) sel[chain[i]] = 2;   // (a chain edge: checked below, never selected)
  for (int64_t e = 0; e < E; ++e)
    if (sel[e] && !pgo::coarsen_finite3(meas[3 * e], meas[3 * e + 1], meas[3 * e + 2])) return not_finite(who, e);
  for (int64_t i = 0; i + 1 < N; ++i) sel[chain[i]] = 0;
  std::vector<double> T((size_t)(N * P));
  pgo::support_trajectory_serial(N, chain.data(), ia, meas, T.data());
  std::vector<int32_t> s_edge, s_lo, s_hi, first;
  pgo::support_sort(N, E, ia, ib, sel.data(), &s_edge, &s_lo, &s_hi, &first, nullptr);
  const int64_t n_sel = (int64_t)s_edge.size();
  std::vector<double> minv((size_t)(n_sel * P));
  for (int64_t r = 0; r < n_sel; ++r) {
    const int64_t e = s_edge[r];
    pgo::support_store(&minv[(size_t)(r * P)], pgo::se2_inverse(pgo::support_canonical(ia[e], ib[e], meas[3 * e], meas[3 * e + 1], meas[3 * e + 2])));
  }
  const double txy2 = o->tol_xy * o->tol_xy, tth2 = o->tol_th * o->tol_th;
  pgo_loop_support_stats st;
  memset(&st, 0, sizeof st);
  for (int64_t e = 0; e < E; ++e) {
    pgo_loop_support_record& O = out[e];
    O.selected = 0;
    O.n_pairs = 0;
    O.n_consistent = 0;
    O.best = -1;
    O.q_min = -1.0;
    if (!sel[e]) continue;
    const int32_t lo = std::min(ia[e], ib[e]), hi = std::max(ia[e], ib[e]);
    int64_t r0, r1;
    pgo::support_range(first.data(), n_poses, lo, o->window, &r0, &r1);
    const pgo::SupportAcc R = pgo::support_scan((int32_t)e, lo, hi, pgo::support_canonical(ia[e], ib[e], meas[3 * e], meas[3 * e + 1], meas[3 * e + 2]), r0,
                                                r1, s_edge.data(), s_lo.data(), s_hi.data(), minv.data(), T.data(), o->window, txy2, tth2);
    O.selected = 1;
    O.n_pairs = R.n_pairs;
    O.n_consistent = R.n_consistent;
    O.best = R.best;
    O.q_min = R.q_min;
    st.n_selected++;
    st.n_supported += R.n_consistent >= o->min_support;
    st.n_pairs_total += R.n_pairs;
    st.max_pairs = std::max(st.max_pairs, R.n_pairs);
  }
  *stats = st;
  if (T_or_null)
    for (int64_t i = 0; i < N; ++i) memcpy(T_or_null + 3 * i, &T[(size_t)(i * P)], 3 * sizeof(double));
  return PGO_OK;
}

int pgo_loop_support(pgo_t* h, const pgo_loop_support_options* opt, const uint8_t* select_or_null, pgo_loop_support_record* out_or_null,
                     pgo_loop_support_stats* stats_or_null) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_loop_support: null handle");
  return h->loop_support(opt, select_or_null, out_or_null, stats_or_null);
}

}  // extern "C"
