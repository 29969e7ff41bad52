// Chordal initialisation (include/pgo.h, "chordal initialisation"): pgo_chordal_init -- the host half of the kernels of
// chordal.hip.h -- and pgo_chordal_plan, the serial host statement of the same two systems (chordal.h).  The measurements stay
// where they are, in the handle's local edge order; the kernels walk the caller's numbering through the tables of pgo_coarsen and
// the slot table (both built once per handle) and start from the trajectory of pgo_loop_support.  It launches none of the LM
// loop's kernels.  Without commit and apply_weights the call touches neither the LM state, the record buffer, the poses nor the
// weight plane.
#include "solver_handle.hip.h"
#include "chordal.hip.h"

namespace {
int check_options(const std::string& who, const pgo_chordal_options* o) {
  if (!o) return fail(PGO_ERR_INVALID_ARG, who + ": null options");
  if (!pgo::chordal_options_ok(o))
    return fail(PGO_ERR_INVALID_ARG, who + ": rtol must be finite and > 0, max_iters and check_every >= 1, mag_min finite and >= 0, rounds 0.." +
                                         std::to_string(PGO_CHORDAL_MAX_ROUNDS) + ", reject_xy and reject_th > 0");
  return PGO_OK;
}
int unanchored(const std::string& who, int32_t pose) {
  return fail(PGO_ERR_UNSUPPORTED, who + ": the component of pose " + std::to_string(pose) + " has positive-weight edges and no constant pose");
}
int not_finite_solution(const std::string& who) { return fail(PGO_ERR_NUMERIC, who + ": the solution is not finite"); }
}  // namespace

int pgo_handle::chordal_init(const pgo_chordal_options* o, double* poses_out, double* res_out, pgo_chordal_summary* summary) {
  const char* who = "pgo_chordal_init";
  PGOC(requires(who, ONE_RANK | NOT_BATCH));
  PGOC(check_options(who, o));
  if (o->apply_weights) PGOC(requires(who, PLAIN_HANDLE));
  const int64_t N = S.n_poses, E = n_edges_total, EL = S.n_edges_local;
  if (N < 2) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": n_poses must be >= 2");
  HIPC(hipSetDevice(device));
  const double t_begin = wall_s();
  PGOC(coarsen_tables(who, false));
  // ---- the weights, the constant poses and the checks, on the host
  std::vector<double> u((size_t)E, 0.0), plane;
  if (w_set) {
    plane.resize((size_t)EL);
    HIPC(hipMemcpyAsync(plane.data(), e_w, (size_t)EL * sizeof(double), hipMemcpyDeviceToHost, stream));
    PGOC(sync());
  }
  int64_t bad = -1;
  for (int64_t k = 0; k < EL; ++k) {
    const int64_t e = S.orig_edge[k];
    const bool active = !(S.flags[k] & dev::EDGE_INACTIVE);
    u[e] = active && cs_ea_h[e] != cs_eb_h[e] ? (w_set ? plane[k] : 1.0) : 0.0;
    if (cs_bad >= 0 && (u[e] > 0.0 || cs_loc_h[e] < 0) && !pgo::coarsen_finite3(S.mx[k], S.my[k], S.mt[k]) && (bad < 0 || e < bad)) bad = e;
  }
  if (bad >= 0) return not_finite(who, bad);
  std::vector<uint8_t> is_const((size_t)N);
  int32_t c0 = -1;
  for (int64_t i = 0; i < N; ++i) {
    const int64_t row = perm.empty() ? i : (int64_t)perm[i];
    is_const[i] = row == fixed_internal || (!act_const_h.empty() && act_const_h[row]);
    if (is_const[i] && c0 < 0) c0 = (int32_t)i;
  }
  if (c0 < 0) return unanchored(who, 0);
  int32_t loose = pgo::chordal_unanchored(N, E, cs_ea_h.data(), cs_eb_h.data(), u.data(), is_const.data());
  if (loose >= 0) return unanchored(who, loose);
  // ---- buffers, before anything is enqueued or changed
  std::vector<int32_t> rp, col, se;
  if (!ch_tab_ready) {
    pgo::chordal_slots(N, E, cs_ea_h.data(), cs_eb_h.data(), &rp, &col, &se);
    ch_slots = (int64_t)col.size();
  }
  const int64_t n_slots = ch_slots, n_tiles = (N + dev::CHORDAL_TILE - 1) / dev::CHORDAL_TILE, n_chunks = (E + dev::WG - 1) / dev::WG,
                n_part = std::max(n_tiles, n_chunks);
  pgo::Layout LT, LW;
  const auto t_rp = LT.add<int32_t>(N + 1), t_col = LT.add<int32_t>(n_slots), t_se = LT.add<int32_t>(n_slots), t_loc = LT.add<int32_t>(E);
  const auto w_u = LW.add<double>(E);   // (the upload: w_u to w_const)
  const auto w_const = LW.add<uint8_t>(N);
  const auto w_rej = LW.add<uint8_t>(E), w_ident = LW.add<uint8_t>(N);
  const auto w_val = LW.add<pgo::Cx>(n_slots);
  const auto w_b = LW.add<pgo::Cx>(N), w_x = LW.add<pgo::Cx>(N), w_r = LW.add<pgo::Cx>(N), w_z = LW.add<pgo::Cx>(N), w_p = LW.add<pgo::Cx>(N),
             w_q = LW.add<pgo::Cx>(N), w_zh = LW.add<pgo::Cx>(N);
  const auto w_d = LW.add<double>(N), w_theta = LW.add<double>(N);
  const auto w_part = LW.add<double>(dev::CHORDAL_NPART * n_part);
  const auto w_st = LW.add<dev::ChordalState>(1);
  const auto w_poses = LW.add<double>(3 * N), w_res = LW.add<double>(2 * E);   // (the copy-out: w_poses to w_res)
  PGOC(support_trajectory_alloc());
  PGOC(reserve(ch_tab, LT.bytes()));
  PGOC(reserve(ch_work, LW.bytes()));
  bool fresh_plane = false;
  if (o->apply_weights) PGOC(weights_begin(&fresh_plane));
  ch_host.resize((size_t)std::max(pgo::run_bytes(w_u, w_const), pgo::run_bytes(w_poses, w_res)));
  // ---- the slot table, once per handle
  std::vector<uint8_t> img;
  if (!ch_tab_ready) {
    img.resize((size_t)LT.bytes());
    memcpy(t_rp.in(img.data()), rp.data(), (size_t)t_rp.bytes());
    if (n_slots) {
      memcpy(t_col.in(img.data()), col.data(), (size_t)t_col.bytes());
      memcpy(t_se.in(img.data()), se.data(), (size_t)t_se.bytes());
    }
    int32_t* loc = t_loc.in(img.data());
    for (int64_t k = 0; k < EL; ++k) loc[S.orig_edge[k]] = (int32_t)k;
    HIPC(hipMemcpyAsync(ch_tab.p, img.data(), img.size(), hipMemcpyHostToDevice, stream));
  }
  PGOC(support_trajectory_enqueue());
  // ---- a call's uploads: the weights and the mask, in one run
  char* work = static_cast<char*>(ch_work.p);
  {
    if (E) memcpy(ch_host.data(), u.data(), (size_t)w_u.bytes());   // (the image of the run: it starts at w_u)
    memcpy(ch_host.data() + (w_const.offset - w_u.offset), is_const.data(), (size_t)w_const.bytes());
    HIPC(hipMemcpyAsync(w_u.in(work), ch_host.data(), (size_t)pgo::run_bytes(w_u, w_const), hipMemcpyHostToDevice, stream));
    if (E) HIPC(hipMemsetAsync(w_rej.in(work), 0, (size_t)w_rej.bytes(), stream));
  }
  dev::ChordalArgs A;
  memset(&A, 0, sizeof A);
  A.g.mx = e_mx;
  A.g.my = e_my;
  A.g.mt = e_mt;
  A.g.loc = t_loc.in(ch_tab.p);
  A.g.poses = poses;
  PGOC(perm_device(&A.g.perm));   // (coarsen_tables made it)
  A.g.is_const = w_const.in(work);
  A.g.T = ls_traj;
  A.rp = t_rp.in(ch_tab.p);
  A.col = t_col.in(ch_tab.p);
  A.se = t_se.in(ch_tab.p);
  A.ea = cs_ea();
  A.eb = cs_eb();
  A.eloc = cs_eloc();
  A.u = w_u.in(work);
  A.rej = w_rej.in(work);
  A.val = w_val.in(work);
  A.b = w_b.in(work);
  A.x = w_x.in(work);
  A.r = w_r.in(work);
  A.z = w_z.in(work);
  A.p = w_p.in(work);
  A.q = w_q.in(work);
  A.zh = w_zh.in(work);
  A.d = w_d.in(work);
  A.theta = w_theta.in(work);
  A.ident = w_ident.in(work);
  A.part = w_part.in(work);
  A.st = w_st.in(work);
  A.poses_out = w_poses.in(work);
  A.res_out = w_res.in(work);
  A.w = e_w;
  A.h_poses = poses;
  A.n = (int32_t)N;
  A.n_edges = (int32_t)E;
  A.n_tiles = (int32_t)n_tiles;
  A.n_chunks = (int32_t)n_chunks;
  A.n_part = (int32_t)n_part;
  A.c0 = c0;
  A.rtol = o->rtol;
  A.mag_min = o->mag_min;
  A.reject_xy = o->reject_xy;
  A.reject_th = o->reject_th;
  const int g_tiles = launch_grid("chordal_grid", n_tiles), g_part = launch_grid("chordal_grid", n_part), g_edges = launch_grid("chordal_grid", n_chunks);
  dev::ChordalState st;
  auto fetch_state = [&]() -> int {
    HIPC(hipMemcpyAsync(&st, A.st, sizeof st, hipMemcpyDeviceToHost, stream));
    return sync();
  };
  // one stage: assemble, r0 = b - H x0, then slices of check_every iterations (three launches each) between reads of the state
  auto solve_stage = [&](int stage, pgo_chordal_solve* R) -> int {
    A.stage = stage;
    A.it = 0;
    HIPC(hipMemsetAsync(A.st, 0, sizeof(dev::ChordalState), stream));
    hipLaunchKernelGGL(dev::k_chordal_assemble<>, dim3(g_tiles), dim3(dev::WG), 0, stream, A);
    PGOC(check_launch("k_chordal_assemble"));
    hipLaunchKernelGGL(dev::k_chordal_spmv<>, dim3(g_tiles), dim3(dev::WG), 0, stream, A, (const pgo::Cx*)A.x, A.q);
    PGOC(check_launch("k_chordal_spmv"));
    hipLaunchKernelGGL(dev::k_chordal_residual<>, dim3(g_tiles), dim3(dev::WG), 0, stream, A);
    PGOC(check_launch("k_chordal_residual"));
    hipLaunchKernelGGL(dev::k_chordal_begin<>, dim3(1), dim3(dev::WG), 0, stream, A);
    PGOC(check_launch("k_chordal_begin"));
    int32_t it = 0;
    PGOC(fetch_state());
    while (!st.done[it & 1] && it < o->max_iters) {
      const int32_t stop = (int32_t)std::min<int64_t>((int64_t)it + o->check_every, o->max_iters);
      for (; it < stop; ++it) {
        A.it = it;
        hipLaunchKernelGGL(dev::k_chordal_spmv<>, dim3(g_tiles), dim3(dev::WG), 0, stream, A, (const pgo::Cx*)A.p, A.q);
        hipLaunchKernelGGL(dev::k_chordal_update<>, dim3(g_tiles), dim3(dev::WG), 0, stream, A);
        hipLaunchKernelGGL(dev::k_chordal_direction<>, dim3(g_tiles), dim3(dev::WG), 0, stream, A);
      }
      PGOC(check_launch("the chordal PCG slice"));
      PGOC(fetch_state());
    }
    R->iters[stage] = st.iters;
    R->converged[stage] = st.done[it & 1] ? 1 : 0;
    R->rel_residual[stage] = st.bb > 0.0 ? std::sqrt(st.rr / st.bb) : std::sqrt(st.rr);
    return PGO_OK;
  };
  pgo_chordal_summary sum;
  memset(&sum, 0, sizeof sum);
  for (int32_t round = 0; round <= o->rounds; ++round) {
    pgo_chordal_solve& R = sum.solve[round];
    PGOC(solve_stage(0, &R));
    hipLaunchKernelGGL(dev::k_chordal_headings<>, dim3(g_tiles), dim3(dev::WG), 0, stream, A);
    PGOC(check_launch("k_chordal_headings"));
    PGOC(solve_stage(1, &R));
    A.reject = round < o->rounds ? 1 : 0;
    hipLaunchKernelGGL(dev::k_chordal_finish<>, dim3(g_part), dim3(dev::WG), 0, stream, A);
    PGOC(check_launch("k_chordal_finish"));
    hipLaunchKernelGGL(dev::k_chordal_fold<>, dim3(1), dim3(dev::WG), 0, stream, A);
    PGOC(check_launch("k_chordal_fold"));
    PGOC(fetch_state());
    ls_traj_ready = true;   // (synchronised: T and the slot table are on the device whatever follows)
    ch_tab_ready = true;
    R.n_degenerate = (int32_t)st.n_degenerate;
    R.min_mag = st.min_mag;
    R.n_rejected = (int32_t)st.n_new;
    sum.n_solves = round + 1;
    sum.n_rejected += R.n_rejected;
    sum.n_degenerate = R.n_degenerate;
    sum.min_mag = R.min_mag;
    if (st.n_bad > 0.0) return not_finite_solution(who);
    if (opt.verbose)
      printf("chordal solve %d  rotations %d it (rel %.3e)  positions %d it (rel %.3e)  min |z| %.3e  degenerate %d  rejected %d\n", round + 1, R.iters[0],
             R.rel_residual[0], R.iters[1], R.rel_residual[1], R.min_mag, R.n_degenerate, R.n_rejected);
    if (R.n_rejected == 0) break;
    // what the rejections left must still hang on a constant pose
    HIPC(hipMemcpyAsync(u.data(), A.u, (size_t)w_u.bytes(), hipMemcpyDeviceToHost, stream));
    PGOC(sync());
    loose = pgo::chordal_unanchored(N, E, cs_ea_h.data(), cs_eb_h.data(), u.data(), is_const.data());
    if (loose >= 0) return unanchored(who, loose);
  }
  // ---- the handle's own state, last
  std::vector<double> ones;
  if (o->apply_weights && EL > 0) {
    if (fresh_plane) PGOC(weights_ones(&ones));
    hipLaunchKernelGGL(dev::k_chordal_apply<>, dim3(g_edges), dim3(dev::WG), 0, stream, A);
    PGOC(check_launch("k_chordal_apply"));
  }
  if (o->commit) {
    hipLaunchKernelGGL(dev::k_chordal_commit<>, dim3(g_tiles), dim3(dev::WG), 0, stream, A);
    PGOC(check_launch("k_chordal_commit"));
  }
  if (poses_out || res_out) HIPC(hipMemcpyAsync(ch_host.data(), A.poses_out, (size_t)pgo::run_bytes(w_poses, w_res), hipMemcpyDeviceToHost, stream));
  PGOC(sync());   // (`ones` dies with this scope)
  if (o->apply_weights && EL > 0) w_set = true;
  if (o->apply_weights || o->commit) solve_is_stale();
  if (poses_out) memcpy(poses_out, ch_host.data(), (size_t)w_poses.bytes());   // (the image of the run: it starts at w_poses)
  if (res_out && E) memcpy(res_out, ch_host.data() + (w_res.offset - w_poses.offset), (size_t)w_res.bytes());
  sum.seconds = wall_s() - t_begin;
  if (summary) *summary = sum;
  return PGO_OK;
}

extern "C" {

void pgo_chordal_options_default(pgo_chordal_options* o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->rtol = 1e-8;
  o->mag_min = 1e-3;
  o->reject_xy = 2.0;
  o->reject_th = 0.35;
  o->max_iters = 20000;
  o->check_every = 50;
  o->rounds = 0;
  o->commit = 0;
  o->apply_weights = 0;
}

int pgo_chordal_plan(int32_t n_poses, int32_t n_edges, const int32_t* ia, const int32_t* ib, const double* meas, const double* w,
                     const uint8_t* constant, const double* poses, const pgo_chordal_options* o, double* poses_out, double* res_out, double* w_out,
                     pgo_chordal_summary* summary) {
  const std::string who = "pgo_chordal_plan";
  if (n_edges < 0 || !ia || !ib || !meas || !poses || !poses_out || !res_out || !summary) return fail(PGO_ERR_INVALID_ARG, who + ": null pointer or negative count");
  if (n_poses < 2) return fail(PGO_ERR_INVALID_ARG, who + ": n_poses must be >= 2");
  PGOC(check_options(who, o));
  const int64_t N = n_poses, E = n_edges, P = pgo::SUPPORT_POSE;
  const double t_begin = wall_s();
  for (int64_t e = 0; e < E; ++e) {
    if (ia[e] < 0 || ia[e] >= N || ib[e] < 0 || ib[e] >= N) return fail(PGO_ERR_INVALID_ARG, who + ": edge " + std::to_string(e) + ": endpoint out of range");
    if (w && !(std::isfinite(w[e]) && w[e] >= 0.0 && w[e] <= 1.0))
      return fail(PGO_ERR_INVALID_ARG, who + ": edge " + std::to_string(e) + ": the weight must be finite and in [0, 1]");
  }
  std::vector<int32_t> chain;
  const int32_t gap = pgo::pick_chain_edges(n_poses, E, ia, ib, &chain);
  if (gap >= 0) return no_chain(who, gap);
  std::vector<double> u((size_t)E);
  std::vector<uint8_t> is_const((size_t)N, 0), must((size_t)E, 0);
  for (int64_t i = 0; i + 1 < N; ++i) must[chain[i]] = 1;
  for (int64_t e = 0; e < E; ++e) {
    u[e] = ia[e] != ib[e] ? (w ? w[e] : 1.0) : 0.0;
    if ((u[e] > 0.0 || must[e]) && !pgo::coarsen_finite3(meas[3 * e], meas[3 * e + 1], meas[3 * e + 2])) return not_finite(who, e);
  }
  int32_t c0 = -1;
  for (int64_t i = 0; i < N; ++i) {
    is_const[i] = constant ? constant[i] != 0 : i == 0;
    if (is_const[i] && c0 < 0) c0 = (int32_t)i;
  }
  if (c0 < 0) return unanchored(who, 0);
  std::vector<double> T((size_t)(N * P));
  pgo::support_trajectory_serial(N, chain.data(), ia, meas, T.data());
  int32_t where = -1;
  const int st = pgo::chordal_serial(N, E, ia, ib, meas, poses, is_const.data(), chain.data(), T.data(), o, u.data(), poses_out, res_out, summary, &where);
  if (st == PGO_ERR_UNSUPPORTED) return unanchored(who, where);
  if (st != PGO_OK) return not_finite_solution(who);
  if (w_out)
    for (int64_t e = 0; e < E; ++e) w_out[e] = u[e] > 0.0 ? u[e] : ((w ? w[e] : 1.0) > 0.0 && ia[e] != ib[e] ? 0.0 : (w ? w[e] : 1.0));
  summary->seconds = wall_s() - t_begin;
  return PGO_OK;
}

int pgo_chordal_init(pgo_t* h, const pgo_chordal_options* opt, double* poses_out_or_null, double* res_out_or_null, pgo_chordal_summary* summary_or_null) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_chordal_init: null handle");
  return h->chordal_init(opt, poses_out_or_null, res_out_or_null, summary_or_null);
}

}  // extern "C"
