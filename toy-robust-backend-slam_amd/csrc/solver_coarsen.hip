// Hierarchical initialisation (include/pgo.h, "hierarchical initialisation"): pgo_coarsen and pgo_prolong -- the host halves --
// and the serial host statement of the same operators, pgo_coarsen_plan and pgo_prolong_eval (coarsen.h).  The measurements stay
// where they are, in the handle's local edge order; the host builds, once per handle, the tables that let the kernels of
// coarsen.hip.h walk the caller's numbering, and one copy-out ends pgo_coarsen.  pgo_coarsen touches neither the LM state, the
// record buffer nor the poses; pgo_prolong writes the poses as pgo_set_poses does.  pgo_coarsen_info / pgo_coarsen_info_plan are
// the same calls with the information matrices carried through the composition (pairs, coarsen.h): one host half and one plan
// serve both, the kernels are siblings, and pgo_coarsen launches none of the new ones.
#include "solver_handle.hip.h"
#include "coarsen.hip.h"

namespace {
// cs_comp = C | Cend, as pgo_coarsen writes and pgo_prolong reads them
struct Composites {
  pgo::Layout L;
  pgo::Span<double> C, Cend;
  Composites(int64_t N, int64_t K) : C(L.add<double>(3 * N)), Cend(L.add<double>(3 * (K - 1))) {}
};
// cs_cov = the covariances of C | of Cend, as pgo_coarsen_info writes them
struct CompositeCovs {
  pgo::Layout L;
  pgo::Span<double> C, Cend;
  CompositeCovs(int64_t N, int64_t K) : C(L.add<double>(6 * N)), Cend(L.add<double>(6 * (K - 1))) {}
};
int not_pd(const std::string& who, int64_t e) {
  return fail(PGO_ERR_NUMERIC, who + ": the information matrix of edge " + std::to_string(e) + " is not finite and positive definite");
}

int check_sizes(const std::string& who, int64_t N, int32_t stride) {
  if (stride < PGO_COARSEN_MIN_STRIDE || stride > PGO_COARSEN_MAX_STRIDE)
    return fail(PGO_ERR_INVALID_ARG, who + ": stride must be " + std::to_string(PGO_COARSEN_MIN_STRIDE) + ".." + std::to_string(PGO_COARSEN_MAX_STRIDE));
  if (N <= stride) return fail(PGO_ERR_INVALID_ARG, who + ": " + std::to_string(N) + " poses give one key pose at stride " + std::to_string(stride) + " (n_poses must exceed the stride)");
  return PGO_OK;
}
// is caller's edge e kept on the coarse graph?  (not a chain edge, ends in two segments)
inline bool kept(const std::vector<int32_t>& chain, const int32_t* ia, const int32_t* ib, int64_t e, int32_t S) {
  const int32_t lo_p = std::min(ia[e], ib[e]);
  if (std::max(ia[e], ib[e]) == lo_p + 1 && chain[lo_p] == (int32_t)e) return false;
  return ia[e] / S != ib[e] / S;
}
}  // namespace

// the tables in the caller's numbering, once per handle
int pgo_handle::coarsen_tables(const char* who, bool all_finite) {
  if (cs_ready) return all_finite && cs_bad >= 0 ? not_finite(who, cs_bad) : PGO_OK;
  const int64_t N = S.n_poses, EL = S.n_edges_local, E = n_edges_total;   // (one rank: every edge is local)
  if (EL != E) return fail(PGO_ERR_UNSUPPORTED, std::string(who) + ": one rank only");
  std::vector<int32_t> inv;   // internal position -> caller's pose
  if (!perm.empty()) {
    inv.resize((size_t)N);
    for (int64_t i = 0; i < N; ++i) inv[perm[i]] = (int32_t)i;
  }
  std::vector<int32_t> ea((size_t)E), eb((size_t)E), loc((size_t)E), chain;
  std::vector<uint8_t> kd((size_t)E);
  int64_t bad = -1;
  for (int64_t k = 0; k < EL; ++k) {
    const int64_t e = S.orig_edge[k];
    ea[e] = inv.empty() ? S.ia[k] : inv[S.ia[k]];
    eb[e] = inv.empty() ? S.ib[k] : inv[S.ib[k]];
    loc[e] = (int32_t)k;
    kd[e] = kind_local[k];
    if (!pgo::coarsen_finite3(S.mx[k], S.my[k], S.mt[k]) && (bad < 0 || e < bad)) bad = e;
  }
  if (bad >= 0 && all_finite) return not_finite(who, bad);
  const int32_t gap = pgo::pick_chain_edges((int32_t)N, E, ea.data(), eb.data(), &chain);
  if (gap >= 0) return no_chain(who, gap);
  std::vector<int32_t> tab((size_t)(N + 3 * E) + (size_t)((E + 3) / 4), 0);
  for (int64_t i = 0; i + 1 < N; ++i) {
    const int32_t e = chain[i];
    tab[i] = (loc[e] << 1) | (ea[e] != (int32_t)i ? 1 : 0);
    loc[e] = -1;
  }
  memcpy(tab.data() + N, ea.data(), (size_t)E * 4);
  memcpy(tab.data() + N + E, eb.data(), (size_t)E * 4);
  memcpy(tab.data() + N + 2 * E, loc.data(), (size_t)E * 4);
  memcpy(tab.data() + N + 3 * E, kd.data(), (size_t)E);
  if (!cs_tab) PGOC(dalloc(&cs_tab, (int64_t)tab.size()));
  PGOC(perm_device());
  PGOC(upload(cs_tab, tab));
  PGOC(sync());   // (`tab` dies with this scope)
  cs_ea_h.swap(ea);
  cs_eb_h.swap(eb);
  cs_loc_h.swap(loc);
  cs_bad = bad;
  cs_ready = true;
  return PGO_OK;
}

// cs_wbad[e]: the information matrix of caller's edge e fails gate_chol3.  Once per handle, on the host, from the planes the
// handle holds on the device (it keeps no host copy of them).
int pgo_handle::coarsen_info_check() {
  if (cs_wbad_ready) return PGO_OK;
  const int64_t EL = S.n_edges_local;
  cs_wbad.assign((size_t)n_edges_total, 0);
  if (e_info && EL) {
    std::vector<double> planes((size_t)(6 * EL));
    HIPC(hipMemcpyAsync(planes.data(), e_info, planes.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    PGOC(sync());
    for (int64_t k = 0; k < EL; ++k) {
      double w[6], o[6];
      for (int c = 0; c < 6; ++c) w[c] = planes[(size_t)(c * EL + k)];
      cs_wbad[(size_t)S.orig_edge[k]] = !pgo::cov_invert(w, o);
    }
  }
  cs_wbad_ready = true;
  return PGO_OK;
}

int pgo_handle::coarsen(int32_t stride, pgo_graph** coarse_out, int32_t* origin, int32_t origin_cap, int32_t* n_coarse_edges, bool with_info,
                        double* cov) {
  const char* who = with_info ? "pgo_coarsen_info" : "pgo_coarsen";
  PGOC(requires(who, ONE_RANK | NOT_BATCH));
  if (!coarse_out) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": null pointer");
  const int64_t N = S.n_poses, E = n_edges_total;
  PGOC(check_sizes(who, N, stride));
  HIPC(hipSetDevice(device));
  PGOC(coarsen_tables(who));
  const int64_t K = (N + stride - 1) / stride;
  int64_t Ec = K - 1;
  for (int64_t e = 0; e < E; ++e) Ec += cs_loc_h[e] >= 0 && cs_ea_h[e] / stride != cs_eb_h[e] / stride;
  if (n_coarse_edges) *n_coarse_edges = (int32_t)Ec;
  if ((origin || cov) && origin_cap < Ec)
    return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": the coarse graph has " + std::to_string(Ec) + " edges, origin holds " + std::to_string(origin_cap));
  if (with_info) {   // every edge this stride uses: the chain edges and the kept ones (a dropped edge may hold anything)
    PGOC(coarsen_info_check());
    for (int64_t e = 0; e < E; ++e)
      if (cs_wbad[e] && (cs_loc_h[e] < 0 || cs_ea_h[e] / stride != cs_eb_h[e] / stride)) return not_pd(who, e);
  }
  // ---- buffers, before anything is enqueued: comp = C | Cend;  work = cnt | off | key poses | meas | ia | ib | origin | kind
  const int64_t nc = (E + dev::COARSEN_CHUNK - 1) / dev::COARSEN_CHUNK;
  const Composites comp(N, K);
  pgo::Layout LW;
  const auto w_cnt = LW.add<int32_t>(nc), w_off = LW.add<int32_t>(nc);
  const auto w_key = LW.add<double>(3 * K), w_meas = LW.add<double>(3 * Ec);   // (the copy-out: w_key to w_kind)
  const auto w_cov = LW.add<double>(with_info ? 6 * Ec : 0), w_info = LW.add<double>(with_info ? 6 * Ec : 0);
  const auto w_ia = LW.add<int32_t>(Ec), w_ib = LW.add<int32_t>(Ec), w_org = LW.add<int32_t>(Ec);
  const auto w_kind = LW.add<uint8_t>(Ec);
  PGOC(reserve(cs_comp, comp.L.bytes()));
  PGOC(reserve(cs_work, LW.bytes()));
  const CompositeCovs ccov(N, K);
  if (with_info) PGOC(reserve(cs_cov, ccov.L.bytes()));
  dev::CoarsenInfoArgs AI;
  dev::CoarsenArgs& A = AI.a;
  PGOC(perm_device(&A.perm));   // (coarsen_tables made it)
  std::unique_ptr<pgo_graph> G(new pgo_graph);
  cs_host.resize((size_t)LW.bytes());
  cs_stride = 0;   // (C and Cend are being rewritten)
  A.mx = e_mx;
  A.my = e_my;
  A.mt = e_mt;
  A.poses = poses;
  A.chain = cs_chain();
  A.ea = cs_ea();
  A.eb = cs_eb();
  A.eloc = cs_eloc();
  A.ekind = cs_ekind();
  A.n = (int32_t)N;
  A.n_edges = (int32_t)E;
  A.stride = stride;
  A.n_key = (int32_t)K;
  A.n_chunks = (int32_t)nc;
  A._pad = 0;
  A.C = comp.C.in(cs_comp.p);
  A.Cend = comp.Cend.in(cs_comp.p);
  A.cnt = w_cnt.in(cs_work.p);
  A.off = w_off.in(cs_work.p);
  A.o_key = w_key.in(cs_work.p);
  A.o_meas = w_meas.in(cs_work.p);
  A.o_ia = w_ia.in(cs_work.p);
  A.o_ib = w_ib.in(cs_work.p);
  A.o_origin = w_org.in(cs_work.p);
  A.o_kind = w_kind.in(cs_work.p);
  AI.info = e_info;
  AI.n_local = S.n_edges_local;
  AI.Ccov = with_info ? ccov.C.in(cs_cov.p) : nullptr;
  AI.Cendcov = with_info ? ccov.Cend.in(cs_cov.p) : nullptr;
  AI.o_cov = w_cov.in(cs_work.p);
  AI.o_info = w_info.in(cs_work.p);
  const int g_seg = launch_grid("coarsen_grid", (K + dev::WG / 64 - 1) / (dev::WG / 64)), g_chunk = launch_grid("coarsen_grid", nc);
  if (with_info) switch ((stride + 63) / 64) {
    case 1: hipLaunchKernelGGL(dev::k_chain_compose_info<1>, dim3(g_seg), dim3(dev::WG), 0, stream, AI); break;
    case 2: hipLaunchKernelGGL(dev::k_chain_compose_info<2>, dim3(g_seg), dim3(dev::WG), 0, stream, AI); break;
    case 3: hipLaunchKernelGGL(dev::k_chain_compose_info<3>, dim3(g_seg), dim3(dev::WG), 0, stream, AI); break;
    default: hipLaunchKernelGGL(dev::k_chain_compose_info<4>, dim3(g_seg), dim3(dev::WG), 0, stream, AI); break;
  }
  else switch ((stride + 63) / 64) {
    case 1: hipLaunchKernelGGL(dev::k_chain_compose<1>, dim3(g_seg), dim3(dev::WG), 0, stream, A); break;
    case 2: hipLaunchKernelGGL(dev::k_chain_compose<2>, dim3(g_seg), dim3(dev::WG), 0, stream, A); break;
    case 3: hipLaunchKernelGGL(dev::k_chain_compose<3>, dim3(g_seg), dim3(dev::WG), 0, stream, A); break;
    default: hipLaunchKernelGGL(dev::k_chain_compose<4>, dim3(g_seg), dim3(dev::WG), 0, stream, A); break;
  }
  PGOC(check_launch("k_chain_compose"));
  hipLaunchKernelGGL(dev::k_coarsen_count<>, dim3(g_chunk), dim3(dev::WG), 0, stream, A);
  PGOC(check_launch("k_coarsen_count"));
  hipLaunchKernelGGL(dev::k_coarsen_scan<>, dim3(1), dim3(dev::WG), 0, stream, A);
  PGOC(check_launch("k_coarsen_scan"));
  if (with_info) hipLaunchKernelGGL(dev::k_coarsen_edges_info<>, dim3(g_chunk), dim3(dev::WG), 0, stream, AI);
  else hipLaunchKernelGGL(dev::k_coarsen_edges<>, dim3(g_chunk), dim3(dev::WG), 0, stream, A);
  PGOC(check_launch("k_coarsen_edges"));
  // ---- one copy-out
  HIPC(hipMemcpyAsync(w_key.in(cs_host.data()), A.o_key, (size_t)pgo::run_bytes(w_key, w_kind), hipMemcpyDeviceToHost, stream));
  PGOC(sync());
  cs_stride = stride;
  pgo::Graph& g = G->g;
  g.pose_id.resize((size_t)K);
  for (int64_t k = 0; k < K; ++k) g.pose_id[k] = (int32_t)k;
  const double *hk = w_key.in(cs_host.data()), *hm = w_meas.in(cs_host.data());
  const int32_t *ha = w_ia.in(cs_host.data()), *hbb = w_ib.in(cs_host.data()), *ho = w_org.in(cs_host.data());
  const uint8_t* hkd = w_kind.in(cs_host.data());
  g.pose.assign(hk, hk + 3 * K);
  g.ea.assign(ha, ha + Ec);
  g.eb.assign(hbb, hbb + Ec);
  g.meas.assign(hm, hm + 3 * Ec);
  g.kind.assign(hkd, hkd + Ec);
  g.info.resize((size_t)(6 * Ec));   // (pgo_coarsen: unit information)
  for (int64_t e = 0; e < Ec; ++e) {
    double* q = &g.info[(size_t)(6 * e)];
    q[0] = q[3] = q[5] = 1.0;
    q[1] = q[2] = q[4] = 0.0;
    g.n_kind[g.kind[e] <= 2 ? g.kind[e] : 2]++;
  }
  if (with_info) {
    const double* hi = w_info.in(cs_host.data());
    for (int64_t i = 0; i < 6 * Ec; ++i)
      if (!pgo::gate_finite(hi[i]))   // (the inputs were positive definite: rounding on an extreme condition number)
        return fail(PGO_ERR_NUMERIC, std::string(who) + ": the covariance of coarse edge " + std::to_string(i / 6) + " is not positive definite");
    g.info.assign(hi, hi + 6 * Ec);
    if (cov) memcpy(cov, w_cov.in(cs_host.data()), (size_t)(6 * Ec) * 8);
  }
  if (origin) memcpy(origin, ho, (size_t)Ec * 4);
  *coarse_out = G.release();
  return PGO_OK;
}

int pgo_handle::prolong(int32_t stride, const double* X) {
  const char* who = "pgo_prolong";
  PGOC(requires(who, ONE_RANK | NOT_BATCH));
  if (!X) return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": null pointer");
  const int64_t N = S.n_poses;
  PGOC(check_sizes(who, N, stride));
  if (cs_stride != stride)
    return fail(PGO_ERR_INVALID_ARG, std::string(who) + ": no composites of stride " + std::to_string(stride) + " (call pgo_coarsen with this stride first)");
  const int64_t K = (N + stride - 1) / stride;
  for (int64_t k = 0; k < K; ++k)
    if (!pgo::coarsen_finite3(X[3 * k], X[3 * k + 1], X[3 * k + 2]))
      return fail(PGO_ERR_NUMERIC, std::string(who) + ": coarse pose " + std::to_string(k) + " is not finite");
  HIPC(hipSetDevice(device));
  const Composites comp(N, K);
  pgo::Layout LW;   // work = the coarse poses
  const auto w_x = LW.add<double>(3 * K);
  PGOC(reserve(cs_work, LW.bytes()));
  dev::ProlongArgs A;
  PGOC(perm_device(&A.perm));   // (pgo_coarsen made it)
  HIPC(hipMemcpyAsync(w_x.in(cs_work.p), X, (size_t)w_x.bytes(), hipMemcpyHostToDevice, stream));
  A.X = w_x.in(cs_work.p);
  A.C = comp.C.in(cs_comp.p);
  A.Cend = comp.Cend.in(cs_comp.p);
  A.constant = fixed_mask;
  A.poses = poses;
  A.n = (int32_t)N;
  A.stride = stride;
  A.n_key = (int32_t)K;
  A.fixed_internal = fixed_internal;
  const int grid = launch_grid("coarsen_grid", (N + dev::WG - 1) / dev::WG);
  hipLaunchKernelGGL(dev::k_prolong<>, dim3(grid), dim3(dev::WG), 0, stream, A);
  PGOC(check_launch("k_prolong"));
  solve_is_stale();   // as pgo_set_poses
  return sync();   // (the caller's X may die after the call)
}

namespace {
// pgo_coarsen_plan (with_info false: the last six arguments play no part) and pgo_coarsen_info_plan
int coarsen_plan(const std::string& who, int32_t n_poses, int32_t n_edges, const int32_t* ia, const int32_t* ib, const double* meas,
                 const uint8_t* kind, int32_t stride, int32_t* n_coarse_poses, int32_t edge_cap, int32_t* cia, int32_t* cib, double* cmeas,
                 uint8_t* ckind, int32_t* corigin, int32_t* n_coarse_edges, double* C_or_null, double* Cend_or_null, bool with_info,
                 const double* info6, double* cinfo, double* ccov, double* Ccov_or_null, double* Cendcov_or_null) {
  if (n_poses < 0 || n_edges < 0 || (n_edges && (!ia || !ib || !meas || !kind)) || !n_coarse_poses || !n_coarse_edges || edge_cap < 0 ||
      (edge_cap && (!cia || !cib || !cmeas || !ckind || !corigin)))
    return fail(PGO_ERR_INVALID_ARG, who + ": bad argument");
  PGOC(check_sizes(who, n_poses, stride));
  const int64_t N = n_poses, E = n_edges, S = stride, K = (N + S - 1) / S;
  for (int64_t e = 0; e < E; ++e)
    if (ia[e] < 0 || ia[e] >= N || ib[e] < 0 || ib[e] >= N) return fail(PGO_ERR_INVALID_ARG, who + ": edge " + std::to_string(e) + ": endpoint out of range");
  for (int64_t e = 0; e < E; ++e)
    if (!pgo::coarsen_finite3(meas[3 * e], meas[3 * e + 1], meas[3 * e + 2])) return not_finite(who, e);
  std::vector<int32_t> chain;
  const int32_t gap = pgo::pick_chain_edges(n_poses, E, ia, ib, &chain);
  if (gap >= 0) return no_chain(who, gap);
  int64_t Ec = K - 1;
  for (int64_t e = 0; e < E; ++e) Ec += kept(chain, ia, ib, e, stride);
  *n_coarse_poses = (int32_t)K;
  *n_coarse_edges = (int32_t)Ec;
  if (Ec > edge_cap)
    return fail(PGO_ERR_INVALID_ARG, who + ": the coarse graph has " + std::to_string(Ec) + " edges, the lists hold " + std::to_string(edge_cap));
  std::vector<double> Cv((size_t)(3 * N)), Ce((size_t)(3 * std::max<int64_t>(K - 1, 1))), Cw, Cew;
  if (with_info) {
    if (info6)   // every edge this stride uses: the chain edges and the kept ones (a dropped edge may hold anything)
      for (int64_t e = 0; e < E; ++e) {
        const int32_t lo_p = std::min(ia[e], ib[e]);
        double o[6];
        if ((kept(chain, ia, ib, e, stride) || (std::max(ia[e], ib[e]) == lo_p + 1 && chain[lo_p] == (int32_t)e)) && !pgo::cov_invert(info6 + 6 * e, o))
          return not_pd(who, e);
      }
    Cw.resize((size_t)(6 * N));
    Cew.resize((size_t)(6 * std::max<int64_t>(K - 1, 1)));
    (void)pgo::coarsen_composites_info_serial(N, S, chain.data(), ia, meas, info6, Cv.data(), Ce.data(), Cw.data(), Cew.data());
  } else {
    pgo::coarsen_composites_serial(N, S, chain.data(), ia, meas, Cv.data(), Ce.data());
  }
  // the covariance and the information of coarse edge `slot`, to whichever list there is; false: lost to rounding
  auto put = [&](int64_t slot, const double* cov) {
    double w[6];
    pgo::coarsen_info_of(cov, w);
    if (ccov) memcpy(ccov + 6 * slot, cov, 48);
    if (cinfo) memcpy(cinfo + 6 * slot, w, 48);
    return pgo::gate_finite(w[0]);
  };
  for (int64_t k = 0; k + 1 < K; ++k) {
    if (with_info && !put(k, &Cew[(size_t)(6 * k)]))
      return fail(PGO_ERR_NUMERIC, who + ": the covariance of coarse edge " + std::to_string(k) + " is not positive definite");
    cia[k] = (int32_t)k;
    cib[k] = (int32_t)k + 1;
    cmeas[3 * k] = Ce[3 * k];
    cmeas[3 * k + 1] = Ce[3 * k + 1];
    cmeas[3 * k + 2] = pgo::coarsen_wrap(Ce[3 * k + 2]);
    ckind[k] = PGO_EDGE_ODOMETRY;
    corigin[k] = -1;
  }
  int64_t slot = K - 1;
  for (int64_t e = 0; e < E; ++e) {
    if (!kept(chain, ia, ib, e, stride)) continue;
    const double *ca = &Cv[(size_t)(3 * ia[e])], *cb = &Cv[(size_t)(3 * ib[e])];
    if (with_info) {
      pgo::Se2Cov Pa, Pb;
      Pa.m = pgo::se2_make(ca[0], ca[1], ca[2]);
      Pb.m = pgo::se2_make(cb[0], cb[1], cb[2]);
      memcpy(Pa.v, &Cw[(size_t)(6 * ia[e])], 48);
      memcpy(Pb.v, &Cw[(size_t)(6 * ib[e])], 48);
      double cov[6];
      (void)pgo::coarsen_transport_pair(Pa, meas[3 * e], meas[3 * e + 1], meas[3 * e + 2], info6 ? info6 + 6 * e : nullptr, Pb, cmeas + 3 * slot, cov);
      if (!put(slot, cov))
        return fail(PGO_ERR_NUMERIC, who + ": the covariance of coarse edge " + std::to_string(slot) + " is not positive definite");
    } else {
      pgo::coarsen_transport(pgo::se2_make(ca[0], ca[1], ca[2]), meas[3 * e], meas[3 * e + 1], meas[3 * e + 2], pgo::se2_make(cb[0], cb[1], cb[2]),
                             cmeas + 3 * slot);
    }
    cia[slot] = ia[e] / stride;
    cib[slot] = ib[e] / stride;
    ckind[slot] = kind[e];
    corigin[slot] = (int32_t)e;
    ++slot;
  }
  if (C_or_null) memcpy(C_or_null, Cv.data(), (size_t)(3 * N) * 8);
  if (Cend_or_null) memcpy(Cend_or_null, Ce.data(), (size_t)(3 * (K - 1)) * 8);
  if (with_info && Ccov_or_null) memcpy(Ccov_or_null, Cw.data(), (size_t)(6 * N) * 8);
  if (with_info && Cendcov_or_null) memcpy(Cendcov_or_null, Cew.data(), (size_t)(6 * (K - 1)) * 8);
  return PGO_OK;
}
}  // namespace

extern "C" {

int pgo_coarsen_plan(int32_t n_poses, int32_t n_edges, const int32_t* ia, const int32_t* ib, const double* meas, const uint8_t* kind,
                     int32_t stride, int32_t* n_coarse_poses, int32_t edge_cap, int32_t* cia, int32_t* cib, double* cmeas,
                     uint8_t* ckind, int32_t* corigin, int32_t* n_coarse_edges, double* C_or_null, double* Cend_or_null) {
  return coarsen_plan("pgo_coarsen_plan", n_poses, n_edges, ia, ib, meas, kind, stride, n_coarse_poses, edge_cap, cia, cib, cmeas, ckind, corigin,
                      n_coarse_edges, C_or_null, Cend_or_null, false, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int pgo_coarsen_info_plan(int32_t n_poses, int32_t n_edges, const int32_t* ia, const int32_t* ib, const double* meas, const uint8_t* kind,
                          const double* info6_or_null, int32_t stride, int32_t* n_coarse_poses, int32_t edge_cap, int32_t* cia, int32_t* cib,
                          double* cmeas, uint8_t* ckind, int32_t* corigin, double* cinfo_or_null, double* ccov_or_null, int32_t* n_coarse_edges,
                          double* C_or_null, double* Cend_or_null, double* Ccov_or_null, double* Cendcov_or_null) {
  return coarsen_plan("pgo_coarsen_info_plan", n_poses, n_edges, ia, ib, meas, kind, stride, n_coarse_poses, edge_cap, cia, cib, cmeas, ckind, corigin,
                      n_coarse_edges, C_or_null, Cend_or_null, true, info6_or_null, cinfo_or_null, ccov_or_null, Ccov_or_null, Cendcov_or_null);
}

int pgo_prolong_eval(int32_t n_poses, int32_t stride, const double* C, const double* Cend, const double* coarse_xyt, double* out_xyt) {
  const std::string who = "pgo_prolong_eval";
  if (n_poses < 0 || !C || !Cend || !coarse_xyt || !out_xyt) return fail(PGO_ERR_INVALID_ARG, who + ": bad argument");
  PGOC(check_sizes(who, n_poses, stride));
  pgo::coarsen_prolong_serial(n_poses, stride, C, Cend, coarse_xyt, out_xyt);
  return PGO_OK;
}

int pgo_coarsen(pgo_t* h, int32_t stride, pgo_graph** coarse_out, int32_t* origin_or_null, int32_t origin_cap, int32_t* n_coarse_edges_or_null) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_coarsen: null handle");
  return h->coarsen(stride, coarse_out, origin_or_null, origin_cap, n_coarse_edges_or_null);
}

int pgo_coarsen_info(pgo_t* h, int32_t stride, pgo_graph** coarse_out, int32_t* origin_or_null, double* cov_or_null, int32_t cap,
                     int32_t* n_coarse_edges_or_null) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_coarsen_info: null handle");
  return h->coarsen(stride, coarse_out, origin_or_null, cap, n_coarse_edges_or_null, true, cov_or_null);
}

int pgo_prolong(pgo_t* h, int32_t stride, const double* coarse_xyt) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_prolong: null handle");
  return h->prolong(stride, coarse_xyt);
}

}  // extern "C"
