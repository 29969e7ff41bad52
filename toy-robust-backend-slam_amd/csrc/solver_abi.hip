// The [gpu] part of the C-ABI (include/pgo.h): handle life cycle, evaluation, solves, results, test hooks, and the debug /
// kernel-bench entry points the parity tests and bench.py use.
#include "solver_handle.hip.h"

// every argument is checked before anything changes; then the class bits of the local edges' flags are rewritten and the
// running solve (if any) is stale: pgo_lm_step refuses until pgo_lm_begin, and the next linearisation uses the new losses
int pgo_handle::set_losses(int32_t n_classes, const pgo_loss* losses, const uint8_t* edge_class) {
  if (n_classes < 1 || n_classes > pgo::MAX_LOSS_CLASSES) return fail(PGO_ERR_INVALID_ARG, "pgo_set_losses: n_classes must be 1..4");
  if (!losses) return fail(PGO_ERR_INVALID_ARG, "pgo_set_losses: null losses");
  for (int32_t k = 0; k < n_classes; ++k)
    if (!pgo::loss_valid(losses[k]))
      return fail(PGO_ERR_INVALID_ARG, "pgo_set_losses: class " + std::to_string(k) + ": unknown type or a scale that is not finite and > 0");
  if (edge_class)
    for (int64_t e = 0; e < n_edges_total; ++e)
      if (edge_class[e] >= n_classes)
        return fail(PGO_ERR_INVALID_ARG, "pgo_set_losses: edge " + std::to_string(e) + ": class " + std::to_string(edge_class[e]) + " >= n_classes");
  const int32_t t0 = losses[0].type;
  loss_n = n_classes;
  loss_general = !(n_classes == 1 && (t0 == PGO_LOSS_TRIVIAL || t0 == PGO_LOSS_HUBER));
  loss_huber = (n_classes == 1 && t0 == PGO_LOSS_HUBER) ? losses[0].a : 0.0;
  for (int k = 0; k < pgo::MAX_LOSS_CLASSES; ++k) {
    const pgo_loss& l = losses[std::min<int32_t>(k, n_classes - 1)];
    loss_cls[k] = pgo::make_loss_class(l.type, l.a);
  }
  const int64_t EL = S.n_edges_local;
  for (int64_t k = 0; k < EL; ++k) {
    const int c = edge_class ? edge_class[S.orig_edge[k]] : std::min<int>(kind_local[k], n_classes - 1);
    S.flags[k] = (uint8_t)((S.flags[k] & (3u | dev::EDGE_INACTIVE)) | ((unsigned)c << 2));   // (bit 4: pgo_set_active's mask stays)
  }
  solve_is_stale();
  if (EL == 0) return PGO_OK;
  HIPC(hipSetDevice(device));
  PGOC(upload(e_flags, S.flags));
  return sync();
}

// pgo_set_active / pgo_batch_set_active.  edge_active: the caller's edge order (a batch: the union's, which is the problems'
// edges concatenated); pose_constant: the caller's pose order (a batch: the union's rows).  Everything is resolved on the host
// before anything changes; then bit 4 of the local edges' flags and the constant-row mask are rewritten, the list of dead
// coarse aggregates follows the resolved constant set, the direct solve steps aside while an edge of its chain is inactive,
// and the running solve (if any) is stale.  Both NULL: the handle is as it was created.
int pgo_handle::set_active(const uint8_t* edge_active, const uint8_t* pose_constant) {
  PGOC(requires("pgo_set_active", METHOD_01 | ONE_RANK));
  HIPC(hipSetDevice(device));
  const int64_t EL = S.n_edges_local, N = S.n_poses;   // (one rank: every edge is local, every row owned)
  const bool restore = !edge_active && !pose_constant;
  // resolved sets
  std::vector<uint8_t> cst;
  int32_t n_act = 0, n_cst = 0;
  bool anchor = false, chain_cut = false;
  {
    std::vector<uint8_t> used((size_t)N, 0);
    for (int64_t k = 0; k < EL; ++k)
      if (!edge_active || edge_active[S.orig_edge[k]]) {
        used[S.ia[k]] = used[S.ib[k]] = 1;
        ++n_act;
      }
    cst.assign((size_t)N, 0);
    if (!fixed_mask_h.empty()) cst = fixed_mask_h;   // a batch: every problem's anchor and the padding rows
    if (fixed_internal >= 0) cst[fixed_internal] = 1;
    for (int64_t i = 0; i < N; ++i) {
      const int64_t r = perm.empty() ? i : (int64_t)perm[i];
      if (pose_constant && pose_constant[i]) {
        cst[r] = 1;
        anchor = true;
      }
      if (!used[r]) cst[r] = 1;
    }
    for (int64_t i = 0; i < N; ++i) n_cst += cst[i];
  }
  if (edge_active && (direct() || takeover() || dl_ready || act_chain_cut)) {
    // the direct solve's chain: the first local edge between every pair of consecutive poses (direct_chain_lists)
    std::vector<uint8_t> seen((size_t)N, 0);
    for (int64_t k = 0; k < EL && !chain_cut; ++k) {
      const int32_t lo_p = std::min(S.ia[k], S.ib[k]), hi_p = std::max(S.ia[k], S.ib[k]);
      if (hi_p == lo_p + 1 && !seen[lo_p]) {
        seen[lo_p] = 1;
        chain_cut = !edge_active[S.orig_edge[k]];
      }
    }
  }
  std::vector<int32_t> dead;
  int32_t* dead_buf = nullptr;
  const bool coarse_built = co_built() && !co_multi();
  // device buffers this call may need, before anything changes
  if (!restore && !batch_mode && !act_mask) PGOC(dalloc(&act_mask, N));
  if (coarse_built) {
    std::vector<uint8_t> keep;
    keep.swap(act_const_h);
    if (!restore) act_const_h = cst;
    coarse_dead_list(&dead);
    act_const_h.swap(keep);
    if ((int)dead.size() > co_dead_cap) PGOC(dalloc(&dead_buf, CO().co_nagg));   // (once per handle: every later list fits)
  }
  // apply
  if (dead_buf) {
    co_dead = dead_buf;
    co_dead_cap = CO().co_nagg;
  }
  for (int64_t k = 0; k < EL; ++k) {
    const bool on = !edge_active || edge_active[S.orig_edge[k]];
    S.flags[k] = (uint8_t)((S.flags[k] & ~dev::EDGE_INACTIVE) | (on ? 0u : dev::EDGE_INACTIVE));
  }
  act_edges = edge_active != nullptr && n_act < EL;
  act_anchor = anchor;
  n_active_edges = n_act;
  n_constant_poses = n_cst;
  if (restore) {
    act_const_h.clear();
    if (!batch_mode) fixed_mask = nullptr;
  } else {
    act_const_h = cst;
    if (!batch_mode) fixed_mask = act_mask;
  }
  act_chain_cut = chain_cut;   // (direct(), takeover(): PCG while the chain is cut)
  solve_is_stale();
  if (EL > 0) PGOC(upload(e_flags, S.flags));
  if (fixed_mask) PGOC(upload(fixed_mask, restore ? fixed_mask_h : act_const_h));
  if (coarse_built) {
    co_ndead = (int)dead.size();
    PGOC(upload(co_dead, dead));
  }
  return sync();   // (`dead` dies with this scope)
}

// ====================================================================== C-ABI
int pgo::require_device(int device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) return fail(PGO_ERR_NO_DEVICE, "no HIP device visible (this backend has no CPU path)");
  if (device < 0 || device >= n) return fail(PGO_ERR_INVALID_ARG, "device index out of range");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(PGO_ERR_HIP, "hipGetDeviceProperties");
  if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
    return fail(PGO_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
  return PGO_OK;
}

extern "C" {

void pgo_options_default(pgo_options* o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->method = 1;
  o->max_iters = 50;
  o->fixed_pose = 0;
  o->jacobi_scaling = 1;
  o->phi = 0.5;
  o->huber_delta = 0.01;
  o->ftol = 1e-6;
  o->gtol = 1e-10;
  o->ptol = 1e-8;
  o->radius0 = 1e4;
  o->max_radius = 1e16;
  o->min_radius = 1e-32;
  o->min_relative_decrease = 1e-3;
  o->min_lm_diagonal = 1e-6;
  o->max_lm_diagonal = 1e32;
  o->pcg_rtol = 1e-10;
  o->pcg_max_iters = 50000;
  o->pcg_check_every = 50;
  o->verbose = 0;
  o->use_graphs = 1;
  o->sc_prior_lambda = 1.0;
  o->pose_ordering = -1;
  o->pcg_chain_len = -1;
  o->halo_exchange = 0;  // all-gather (has run through RCCL, capturable); 1 = point-to-point exchange of the referenced rows:
                         // opt-in like halo_overlap until a multi-GPU run has checked it against the all-gather (bench.py does
                         // that check itself when it runs on several GPUs and then times the verified p2p path)
  o->halo_overlap = 0;   // opt-in: the two-stream schedule has never run against a real peer (no multi-GPU lease yet)
  o->linear_solver = 0;  // auto: the direct chain + low-rank solve on small chain-like graphs in the exact mode, else PCG
  o->pcg_coarse_poses = -1;  // auto: a rigid-body coarse level for exact-mode PCG solves of graphs of >= 512 poses
}

int pgo_create(pgo_t** h, int32_t n_poses, const double* poses, int32_t n_edges, const int32_t* ia, const int32_t* ib,
               const double* meas, const uint8_t* kind, const pgo_options* opt, pgo_comm* comm, int device) {
  return pgo_create_weighted(h, n_poses, poses, n_edges, ia, ib, meas, nullptr, kind, opt, comm, device);
}

int pgo_create_weighted(pgo_t** h, int32_t n_poses, const double* poses, int32_t n_edges, const int32_t* ia,
                        const int32_t* ib, const double* meas, const double* info6_or_null, const uint8_t* kind,
                        const pgo_options* opt, pgo_comm* comm, int device) {
  if (!h || !poses || n_poses <= 0 || n_edges < 0 || (n_edges && (!ia || !ib || !meas || !kind)))
    return fail(PGO_ERR_INVALID_ARG, "pgo_create: bad argument");
  pgo_options o;
  if (opt) o = *opt;
  else pgo_options_default(&o);
  if (o.method < 0 || o.method > 2)
    return fail(PGO_ERR_UNSUPPORTED, "only METHOD 0 (plain), 1 (DCS) and 2 (switchable constraints) are implemented (reference main.cpp:54-56)");
  if (o.fixed_pose >= n_poses) return fail(PGO_ERR_INVALID_ARG, "fixed_pose out of range");
  // every endpoint is checked HERE -- before the device is touched and before anything indexes by it
  // (resolve_chain_len, compute_pose_order and build_shard_structure all do)
  for (int32_t e = 0; e < n_edges; ++e) {
    if (ia[e] < 0 || ia[e] >= n_poses || ib[e] < 0 || ib[e] >= n_poses)
      return fail(PGO_ERR_INVALID_ARG, "edge " + std::to_string(e) + ": endpoint out of range");
    if (ia[e] == ib[e])
      return fail(PGO_ERR_INVALID_ARG, "edge " + std::to_string(e) + ": self loop (Ceres rejects duplicate parameter blocks)");
  }
  PGOC(require_device(device));
  std::unique_ptr<pgo_handle> H(new pgo_handle);
  H->opt = o;
  H->comm = comm;
  H->device = device;
  PGOC(H->create(n_poses, poses, n_edges, ia, ib, meas, info6_or_null, kind));
  *h = H.release();
  return PGO_OK;
}

int pgo_create_from_graph(pgo_t** h, const pgo_graph* g, const pgo_options* opt, pgo_comm* comm, int device) {
  if (!g) return fail(PGO_ERR_INVALID_ARG, "pgo_create_from_graph: null graph");
  const pgo::Graph& G = g->g;
  return pgo_create_weighted(h, G.n_poses(), G.pose.data(), G.n_edges(), G.ea.data(), G.eb.data(), G.meas.data(),
                             G.info.size() == (size_t)6 * G.n_edges() ? G.info.data() : nullptr, G.kind.data(), opt, comm, device);
}

void pgo_destroy(pgo_t* h) { delete h; }

int pgo_set_poses(pgo_t* h, const double* poses) {
  if (!h || !poses) return fail(PGO_ERR_INVALID_ARG, "pgo_set_poses: null");
  HIPC(hipSetDevice(h->device));
  h->solve_is_stale();
  return h->upload_pose_vector(h->poses, poses);
}

int pgo_get_poses(pgo_t* h, double* out) {
  if (!h || !out) return fail(PGO_ERR_INVALID_ARG, "pgo_get_poses: null");
  HIPC(hipSetDevice(h->device));
  return h->download_pose_vector(out, h->poses);
}

int pgo_get_switches(pgo_t* h, double* switches, double* js_out) {
  if (!h || !switches) return fail(PGO_ERR_INVALID_ARG, "pgo_get_switches: null");
  if (h->comm && h->comm->world > 1) return fail(PGO_ERR_UNSUPPORTED, "pgo_get_switches: world == 1 only");
  HIPC(hipSetDevice(h->device));
  const int64_t EL = h->S.n_edges_local;
  if (!h->has_sw) {
    for (int64_t k = 0; k < EL; ++k) switches[h->S.orig_edge[k]] = 1.0;
    if (js_out) memset(js_out, 0, (size_t)3 * EL * sizeof(double));
    return PGO_OK;
  }
  std::vector<double> v((size_t)EL), j((size_t)3 * EL);
  HIPC(hipMemcpyAsync(v.data(), h->sw, v.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPC(hipMemcpyAsync(j.data(), h->sw_js, j.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  PGOC(h->sync());
  for (int64_t k = 0; k < EL; ++k) {
    const int64_t e = h->S.orig_edge[k];
    const bool robust = h->S.flags[k] & 1;
    switches[e] = robust ? v[k] : 1.0;
    if (js_out)
      for (int c = 0; c < 3; ++c) js_out[3 * e + c] = robust ? j[3 * k + c] : 0.0;
  }
  return PGO_OK;
}

int pgo_eval(pgo_t* h, const double* poses_or_null, int apply_loss, double* cost, double* r_out, double* J_out) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_eval: null handle");
  HIPC(hipSetDevice(h->device));
  const bool want_jac = r_out || J_out;
  if (want_jac && h->comm && h->comm->world > 1) return fail(PGO_ERR_UNSUPPORTED, "pgo_eval: r/J outputs need world == 1");
  const double* x = h->poses;
  if (poses_or_null) {
    PGOC(h->upload_pose_vector(h->cand, poses_or_null));
    x = h->cand;
  }
  if (want_jac) h->solve_is_stale();  // the record buffer is about to be overwritten
  PGOC(h->eval_enqueue(x, h->sw, apply_loss, want_jac, 0));
  PGOC(h->fetch_scal(0, 2));
  if (cost) *cost = h->h_scal[0];
  if (want_jac) {
    const int64_t EL = h->S.n_edges_local;
    const int RN = h->rec_doubles, R0 = h->info_mode ? 12 : 10;
    std::vector<double> rec((size_t)EL * RN);
    HIPC(hipMemcpyAsync(rec.data(), h->jr, rec.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    PGOC(h->sync());
    for (int64_t k = 0; k < EL; ++k) {
      const int64_t e = h->S.orig_edge[k];
      const double* R = &rec[(size_t)k * RN];
      if (J_out) {  // expand the implied second block: d e/d P2 = [-A[:,0] | -A[:,1] | (0,0,g2)']
        double* Jo = J_out + 18 * e;
        for (int i = 0; i < 3; ++i) {
          Jo[6 * i + 0] = R[3 * i];
          Jo[6 * i + 1] = R[3 * i + 1];
          Jo[6 * i + 2] = R[3 * i + 2];
          Jo[6 * i + 3] = -R[3 * i];
          Jo[6 * i + 4] = -R[3 * i + 1];
          Jo[6 * i + 5] = h->info_mode ? R[9 + i] : ((i == 2) ? R[9] : 0.0);
        }
      }
      if (r_out) memcpy(r_out + 3 * e, R + R0, 3 * sizeof(double));
    }
  }
  if (h->h_scal[1] > 0.0) return fail(PGO_ERR_NUMERIC, "non-finite residual or Jacobian");
  return PGO_OK;
}

int pgo_loss_evaluate(const pgo_loss* l, double s, double rho[3]) {
  if (!l || !rho) return fail(PGO_ERR_INVALID_ARG, "pgo_loss_evaluate: null");
  if (!pgo::loss_valid(*l)) return fail(PGO_ERR_INVALID_ARG, "pgo_loss_evaluate: unknown type or a scale that is not finite and > 0");
  pgo::loss_rho(pgo::make_loss_class(l->type, l->a), s, rho);
  return PGO_OK;
}

int pgo_set_losses(pgo_t* h, int32_t n_classes, const pgo_loss* losses, const uint8_t* edge_class) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_set_losses: null handle");
  return h->set_losses(n_classes, losses, edge_class);
}

int pgo_set_active(pgo_t* h, const uint8_t* edge_active, const uint8_t* pose_constant) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_set_active: null handle");
  return h->set_active(edge_active, pose_constant);
}

int pgo_edge_chi2(pgo_t* h, const double* poses_or_null, double* chi2_out) {
  if (!h || !chi2_out) return fail(PGO_ERR_INVALID_ARG, "pgo_edge_chi2: null");
  if (!h->e_info) return fail(PGO_ERR_INVALID_ARG, "pgo_edge_chi2: the handle was created without information matrices");
  HIPC(hipSetDevice(h->device));
  const int64_t E = h->n_edges_total, EL = h->S.n_edges_local;
  if (E == 0) return PGO_OK;
  if (!h->chi2_buf) {
    PGOC(h->dalloc(&h->chi2_buf, E));
    PGOC(h->dalloc(&h->e_orig, std::max<int64_t>(EL, 1)));
    PGOC(h->upload(h->e_orig, h->S.orig_edge));
  }
  const double* x = h->poses;
  if (poses_or_null) {
    PGOC(h->upload_pose_vector(h->cand, poses_or_null));
    x = h->cand;
  }
  HIPC(hipMemsetAsync(h->chi2_buf, 0, (size_t)E * sizeof(double), h->stream));
  if (EL > 0) {
    dev::EdgeArgs A = h->edge_args(x, nullptr, 0);
    const int grid = (int)std::min<int64_t>((EL + dev::WG - 1) / dev::WG, 8192);
    hipLaunchKernelGGL(dev::k_edge_chi2<>, dim3(grid), dim3(dev::WG), 0, h->stream, A, (const int32_t*)h->e_orig, h->chi2_buf);
    PGOC(h->check_launch("k_edge_chi2"));
  }
  if (h->multi_rank()) {  // every edge is counted on exactly one rank (flags bit1): the sum assembles the vector
    for (int64_t off = 0; off < E; off += (1 << 16)) {  // 512 KiB pieces (fits a slot of the shm test back-end)
      const int n = (int)std::min<int64_t>(E - off, 1 << 16);
      if (h->comm->allreduce(h->chi2_buf + off, n, false, h->stream) != 0) return fail(PGO_ERR_COMM, "pgo_edge_chi2: all-reduce failed");
    }
  }
  HIPC(hipMemcpyAsync(chi2_out, h->chi2_buf, (size_t)E * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return h->sync();
}

int pgo_lm_begin(pgo_t* h) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_lm_begin: null handle");
  return h->lm_begin();
}

int pgo_lm_step(pgo_t* h, int32_t n_iters, int32_t* done, pgo_summary* s) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_lm_step: null handle");
  if (!h->lm_active || !h->lin_valid) return fail(PGO_ERR_INVALID_ARG, "pgo_lm_step: call pgo_lm_begin first");
  HIPC(hipSetDevice(h->device));
  bool stop = h->lm_done;
  for (int32_t k = 0; k < n_iters && !stop; ++k) PGOC(h->lm_iteration(&stop));
  h->lm_done = stop;
  if (done) *done = stop ? 1 : 0;
  h->fill_summary(s);
  return PGO_OK;
}

int pgo_solve(pgo_t* h, pgo_summary* s) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_solve: null handle");
  PGOC(h->lm_begin());
  bool stop = false;
  while (!stop) PGOC(h->lm_iteration(&stop));
  h->lm_done = true;
  h->fill_summary(s);
  return PGO_OK;
}

// Many independent solves at once (the reference's layer managers call ceres::Solve on a full-graph copy
// or a window per candidate layer / edge, src/simple_layer_manager.cpp:457-622, src/layer_manager.cpp:104-179): every
// handle owns its stream, device buffers and captured hipGraph, so `max_concurrency` host threads drive that many LM
// solves concurrently and the launch-/latency-bound small problems overlap on the device.
int pgo_solve_batch(pgo_t* const* handles, int32_t n, pgo_summary* summaries, int32_t max_concurrency) {
  if (n < 0 || (n > 0 && !handles)) return fail(PGO_ERR_INVALID_ARG, "pgo_solve_batch: bad argument");
  for (int32_t i = 0; i < n; ++i) {
    if (!handles[i]) return fail(PGO_ERR_INVALID_ARG, "pgo_solve_batch: null handle " + std::to_string(i));
    if (handles[i]->comm) return fail(PGO_ERR_UNSUPPORTED, "pgo_solve_batch: handles with a communicator solve collectively, one at a time");
    for (int32_t j = 0; j < i; ++j)
      if (handles[j] == handles[i]) return fail(PGO_ERR_INVALID_ARG, "pgo_solve_batch: handle " + std::to_string(i) + " listed twice");
  }
  if (n == 0) return PGO_OK;
  const int n_thr = std::max(1, std::min<int>(n, max_concurrency > 0 ? max_concurrency : 8));
  std::atomic<int32_t> next(0);
  std::mutex mu;
  int first_status = PGO_OK;
  std::string first_msg;
  auto worker = [&] {
    for (;;) {
      const int32_t i = next.fetch_add(1);
      if (i >= n) return;
      pgo_summary tmp;
      const int st = pgo_solve(handles[i], summaries ? &summaries[i] : &tmp);
      if (st != PGO_OK) {
        std::lock_guard<std::mutex> lk(mu);
        if (first_status == PGO_OK) {
          first_status = st;
          first_msg = "problem " + std::to_string(i) + ": " + pgo_last_error();  // the worker's thread-local text
        }
      }
    }
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < n_thr; ++t) pool.emplace_back(worker);
  worker();
  for (auto& th : pool) th.join();
  if (first_status != PGO_OK) return fail(first_status, first_msg);
  return PGO_OK;
}

int pgo_get_info(const pgo_t* h, pgo_handle_info* out) {
  if (!h || !out) return fail(PGO_ERR_INVALID_ARG, "pgo_get_info: null");
  memset(out, 0, sizeof *out);
  out->n_poses = h->S.n_poses;
  out->n_edges = (int32_t)h->n_edges_total;
  out->world = h->comm ? h->comm->world : 1;
  out->rank = h->comm ? h->comm->rank : 0;
  out->row_lo = h->S.lo;
  out->row_hi = h->S.hi;
  out->n_edges_local = h->S.n_edges_local;
  out->n_tiles = h->S.n_tiles();
  out->n_incidences = h->S.n_inc_real;
  out->pcg_block_poses = h->plan.own.grp_B;
  out->pcg_chain_len = h->plan.all.chain_len;
  out->chain_kernel = h->plan.all.chain_chunk;
  out->pose_ordering = h->perm.empty() ? 0 : 1;
  out->halo_exchange = h->plan.all.use_halo ? 1 : 0;
  out->halo_overlap = h->plan.own.overlap ? 1 : 0;
  out->halo_send_rows = (int64_t)h->S.halo_send_row.size();
  out->halo_recv_rows = (int64_t)h->S.halo_recv_row.size();
  out->device_bytes = h->device_bytes;
  out->host_enqueue_us_per_pcg_iter = h->n_enqueued > 0 ? 1e6 * h->t_enqueue / (double)h->n_enqueued : 0.0;
  out->pcg_graph_replay = (h->cg_graph_exec != nullptr && !h->graph_failed) ? 1 : 0;
  out->linear_solver = h->direct() ? 2 : 1;
  out->direct_rank = h->direct() ? h->plan.dl.dl_K : 0;
  out->direct_fallbacks = h->dl_fallbacks;
  out->direct_switched_at = h->dl_switched_at;
  out->pcg_single_reduction = h->plan.all.use_sr ? 1 : 0;
  out->pcg_coarse_poses = h->coarse_on() ? h->CO().co_agg : 0;
  out->pcg_coarse_rank = h->coarse_on() ? h->CO().co_K : 0;
  out->pcg_coarse_off_iters = h->co_off_iters;
  out->direct_separators = h->direct() ? h->plan.dl.dl_nsep : 0;
  out->direct_segments = h->direct() ? h->plan.dl.dl_nseg : 0;
  out->direct_refine_kernel = h->direct() ? (h->dl_pre2 ? 1 : 2) : 0;
  out->n_active_edges = h->n_active_edges;
  out->n_constant_poses = h->n_constant_poses;
  return PGO_OK;
}

}  // extern "C"

extern "C" {

int32_t pgo_num_iter_records(const pgo_t* h) { return h ? (int32_t)h->recs.size() : 0; }
int pgo_get_iter_records(const pgo_t* h, pgo_iter_record* out, int32_t cap) {
  if (!h || !out) return fail(PGO_ERR_INVALID_ARG, "pgo_get_iter_records: null");
  int32_t n = std::min<int32_t>(cap, (int32_t)h->recs.size());
  memcpy(out, h->recs.data(), (size_t)n * sizeof(pgo_iter_record));
  return PGO_OK;
}

// ------------------------------------------------------------ debug / bench
int pgo_debug_normal_eq(pgo_t* h, double* g_out, double* hdiag_out) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_debug_normal_eq: null handle");
  if (h->comm && h->comm->world > 1) return fail(PGO_ERR_UNSUPPORTED, "world == 1 only");
  HIPC(hipSetDevice(h->device));
  h->lm_active = false;
  PGOC(h->launch_jacobi_scale(0));
  int st = h->linearize(false);
  h->lin_valid = false;
  PGOC(st);
  const int64_t N = h->S.n_loc;
  std::vector<double> g_tmp;
  if (g_out) {
    g_tmp.resize((size_t)3 * N);
    HIPC(hipMemcpyAsync(g_tmp.data(), h->gs, g_tmp.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  std::vector<double> planes;
  if (hdiag_out) {
    planes.resize((size_t)6 * N);
    HIPC(hipMemcpyAsync(planes.data(), h->hd, planes.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  PGOC(h->sync());
  auto internal = [&](int64_t i) { return h->perm.empty() ? i : (int64_t)h->perm[i]; };
  if (g_out)
    for (int64_t i = 0; i < N; ++i) memcpy(g_out + 3 * i, &g_tmp[(size_t)3 * internal(i)], 3 * sizeof(double));
  if (hdiag_out) {
    static const int map9[9] = {0, 1, 2, 1, 3, 4, 2, 4, 5};
    for (int64_t i = 0; i < N; ++i)
      for (int c = 0; c < 9; ++c) hdiag_out[9 * i + c] = planes[(size_t)map9[c] * N + internal(i)];
  }
  return PGO_OK;
}

int pgo_debug_spmv(pgo_t* h, const double* x, double* yout) {
  if (!h || !x || !yout) return fail(PGO_ERR_INVALID_ARG, "pgo_debug_spmv: null");
  if (h->comm && h->comm->world > 1) return fail(PGO_ERR_UNSUPPORTED, "world == 1 only");
  HIPC(hipSetDevice(h->device));
  PGOC(h->upload_pose_vector(h->y, x));
  PGOC(h->scatter_owned(h->y));
  PGOC(h->spmv_enqueue(h->p_full, h->ap, h->part[0], 0, nullptr));
  return h->download_pose_vector(yout, h->ap);
}

// The debug / bench hooks below set up the LM diagonal for the current radius and the preconditioner on the current
// linearisation, as the next LM iteration does (after an accepted step H is new and the factors are not; after a rejected one the
// radius changed) -- the preconditioner also on a handle on the direct solve, which does not factorise it per LM iteration:
// prepare_system(radius, true).  Every buffer written there is rewritten from H and the radius by the next iteration's
// prepare_system() before it is read: a solve is not affected.
int pgo_debug_system_spmv(pgo_t* h, const double* x, double* yout, double* d2_out) {
  if (!h || !x || !yout) return fail(PGO_ERR_INVALID_ARG, "pgo_debug_system_spmv: null");
  if (h->comm && h->comm->world > 1) return fail(PGO_ERR_UNSUPPORTED, "world == 1 only");
  if (!h->lin_valid) return fail(PGO_ERR_INVALID_ARG, "pgo_debug_system_spmv: call pgo_lm_begin first");
  HIPC(hipSetDevice(h->device));
  PGOC(h->prepare_system(h->tr.radius, true));
  PGOC(h->upload_pose_vector(h->ap, x));   // ap: scratch input
  PGOC(h->scatter_owned(h->ap));
  PGOC(h->spmv_enqueue(h->p_full, h->ap, h->part[0], 1, nullptr));
  PGOC(h->download_pose_vector(yout, h->ap));
  return d2_out ? h->download_pose_vector(d2_out, h->d2) : PGO_OK;
}

// z = M^-1 r with the preconditioner the next LM iteration applies (whatever family the handle resolved to), through the
// PCG start-up kernel: for the restatement and property tests.  Needs at least one LM iteration; world == 1, or several ranks
// with the second preconditioner level (a collective call: every rank passes the whole r and receives z on its own rows).
int pgo_debug_precond(pgo_t* h, const double* r_in, double* z_out) {
  if (!h || !r_in || !z_out) return fail(PGO_ERR_INVALID_ARG, "pgo_debug_precond: null");
  if (h->comm && h->comm->world > 1 && !h->co_multi()) return fail(PGO_ERR_UNSUPPORTED, "world == 1 only (several ranks: with pcg_coarse_poses > 0)");
  if (!h->lin_valid || h->iter < 1) return fail(PGO_ERR_INVALID_ARG, "pgo_debug_precond: run at least one LM iteration first");
  HIPC(hipSetDevice(h->device));
  PGOC(h->upload_pose_vector(h->ap, r_in, h->S.lo, h->S.n_loc));   // ap: scratch input (the owned rows)
  PGOC(h->prepare_system(h->tr.radius, true));
  // (several ranks: r_c through the all-reduce, the replicated coarse solve, the own rows of P e_c)
  PGOC(h->precondition(h->ap, nullptr, nullptr, h->co_multi() ? h->co_dotp : h->part[3]));
  return h->download_pose_vector(z_out, h->z, h->S.lo, h->S.n_loc);   // (several ranks: the peers' rows stay 0)
}

// y = (H + D'D)^-1 b through direct_enqueue(), the launch sequence an LM iteration on the direct solve runs (eagerly: a
// graph captured for LM keeps its own arguments and is neither used nor touched).  direct_enqueue() writes y, r, ap, the
// gather vector and scal[8..9]; they are saved and put back, so that the LM loop finds what it left.
int pgo_debug_direct_solve(pgo_t* h, const double* b_in, int32_t refine_steps, double* y_out) {
  if (!h || !b_in || !y_out) return fail(PGO_ERR_INVALID_ARG, "pgo_debug_direct_solve: null");
  if (refine_steps < -1 || refine_steps > 3) return fail(PGO_ERR_INVALID_ARG, "pgo_debug_direct_solve: refine_steps is -1 (the handle's own) or 0 .. 3");
  if (!h->direct() || !h->dl_ready) return fail(PGO_ERR_UNSUPPORTED, "pgo_debug_direct_solve: the handle is not on the direct solve");
  if (!h->lin_valid) return fail(PGO_ERR_INVALID_ARG, "pgo_debug_direct_solve: call pgo_lm_begin first");
  HIPC(hipSetDevice(h->device));
  const size_t n3 = (size_t)3 * h->S.n_loc, npf = (size_t)dev::PS * h->n_full;   // (one rank, identity ordering: n_loc = N)
  const size_t off_r = n3, off_ap = 2 * n3, off_pf = 3 * n3, off_scal = off_pf + npf, off_b = off_scal + N_SCAL;
  double* save = nullptr;
  if (hipMalloc((void**)&save, (off_b + n3) * sizeof(double)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(PGO_ERR_NOMEM, "pgo_debug_direct_solve: hipMalloc");
  }
  auto run = [&]() -> int {
    const hipMemcpyKind d2d = hipMemcpyDeviceToDevice;
    HIPC(hipMemcpyAsync(save, h->y, n3 * sizeof(double), d2d, h->stream));
    HIPC(hipMemcpyAsync(save + off_r, h->r, n3 * sizeof(double), d2d, h->stream));
    HIPC(hipMemcpyAsync(save + off_ap, h->ap, n3 * sizeof(double), d2d, h->stream));
    HIPC(hipMemcpyAsync(save + off_pf, h->p_full, npf * sizeof(double), d2d, h->stream));
    HIPC(hipMemcpyAsync(save + off_scal, h->scal, N_SCAL * sizeof(double), d2d, h->stream));
    HIPC(hipMemcpyAsync(save + off_b, b_in, n3 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    PGOC(h->prepare_system(h->tr.radius));
    PGOC(h->direct_enqueue(save + off_b, refine_steps < 0 ? h->plan.dl.dl_refine : refine_steps));
    HIPC(hipMemcpyAsync(y_out, h->y, n3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPC(hipMemcpyAsync(h->y, save, n3 * sizeof(double), d2d, h->stream));
    HIPC(hipMemcpyAsync(h->r, save + off_r, n3 * sizeof(double), d2d, h->stream));
    HIPC(hipMemcpyAsync(h->ap, save + off_ap, n3 * sizeof(double), d2d, h->stream));
    HIPC(hipMemcpyAsync(h->p_full, save + off_pf, npf * sizeof(double), d2d, h->stream));
    HIPC(hipMemcpyAsync(h->scal, save + off_scal, N_SCAL * sizeof(double), d2d, h->stream));
    return h->sync();
  };
  const int st = run();
  if (st != PGO_OK) (void)hipStreamSynchronize(h->stream);
  (void)hipFree(save);
  return st;
}

static int time_launches(pgo_handle* h, int reps, const std::function<void()>& launch, double* ms_avg) {
  hipEvent_t e0, e1;
  HIPC(hipEventCreate(&e0));
  HIPC(hipEventCreate(&e1));
  launch();  // one untimed launch
  HIPC(hipEventRecord(e0, h->stream));
  for (int i = 0; i < reps; ++i) launch();
  HIPC(hipEventRecord(e1, h->stream));
  HIPC(hipEventSynchronize(e1));
  float ms = 0;
  HIPC(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *ms_avg = (double)ms / reps;
  return h->check_launch("bench launch");
}

int pgo_bench_eval(pgo_t* h, int reps, int with_jacobian, pgo_kernel_stats* out) {
  if (!h || !out || reps < 1) return fail(PGO_ERR_INVALID_ARG, "pgo_bench_eval: bad argument");
  HIPC(hipSetDevice(h->device));
  double ms = 0;
  PGOC(time_launches(h, reps, [&] { h->launch_eval(h->poses, h->sw, 1, with_jacobian != 0); }, &ms));
  out->ms_avg = ms;
  out->units = h->S.n_edges_local;
  // 84 B read per edge + the record (here 112 B: DESIGN.md section 2); 84 + 8 without
  out->algorithmic_bytes = (double)h->S.n_edges_local * (with_jacobian ? 196.0 : 92.0);
  return PGO_OK;
}

int pgo_bench_assemble(pgo_t* h, int reps, pgo_kernel_stats* out) {
  if (!h || !out || reps < 1) return fail(PGO_ERR_INVALID_ARG, "pgo_bench_assemble: bad argument");
  if (!h->lin_valid) return fail(PGO_ERR_INVALID_ARG, "pgo_bench_assemble: call pgo_lm_begin first");
  HIPC(hipSetDevice(h->device));
  double ms = 0;
  PGOC(time_launches(h, reps, [&] { (void)h->assemble_enqueue(); }, &ms));
  out->ms_avg = ms;
  out->units = h->S.n_edges_local;
  // every record read once (112 B/edge); per incidence 8 B indices + 72 B block written; per row 72 B out + 4 B
  // pointer + 24 B scale
  // chain preconditioner: + the 72-byte block (i, i-1) per row into the factorisation's input record
  out->algorithmic_bytes = 112.0 * h->S.n_edges_local + 80.0 * (double)h->S.n_inc_real + (100.0 + (h->plan.all.chain_len ? 72.0 : 0.0)) * h->S.n_loc;
  return PGO_OK;
}

int pgo_bench_spmv(pgo_t* h, int reps, pgo_kernel_stats* out) {
  if (!h || !out || reps < 1) return fail(PGO_ERR_INVALID_ARG, "pgo_bench_spmv: bad argument");
  if (!h->lin_valid) return fail(PGO_ERR_INVALID_ARG, "pgo_bench_spmv: call pgo_lm_begin first");
  HIPC(hipSetDevice(h->device));
  double ms = 0;
  PGOC(time_launches(h, reps, [&] { (void)h->spmv_enqueue(h->p_full, h->ap, h->part[0], 1, nullptr); }, &ms));
  out->ms_avg = ms;
  out->units = h->S.n_inc_real + h->S.n_loc;
  // 76 B per off-diagonal block (value + column) ; per row: 48 B diagonal planes + 24 B D'D + 4 B row
  // pointer + 24 B y + 24 B p; the product kernel k_spmv_p reads the diagonal with D'D folded in (k_prepare): 24 B less
  out->algorithmic_bytes = 76.0 * (double)h->S.n_inc_real + (h->plan.own.spmv_pipe ? 100.0 : 124.0) * h->S.n_loc;
  return PGO_OK;
}

// the preconditioner apply as the PCG start-up kernel issues it (z = M^-1 b; writes y, r, z, p): timing only
int pgo_bench_precond(pgo_t* h, int reps, pgo_kernel_stats* out) {
  if (!h || !out || reps < 1) return fail(PGO_ERR_INVALID_ARG, "pgo_bench_precond: bad argument");
  if (!h->lin_valid || h->iter < 1) return fail(PGO_ERR_INVALID_ARG, "pgo_bench_precond: run at least one LM iteration first");
  HIPC(hipSetDevice(h->device));
  PGOC(h->prepare_system(h->tr.radius, true));
  double ms = 0;
  const double nl = (double)h->S.n_loc;
  PGOC(time_launches(h, reps, [&] { (void)h->launch_cg_init(h->gs, nullptr, h->part[0], h->part[1]); }, &ms));
  if (h->plan.all.chain_len) out->algorithmic_bytes = (120.0 + 24.0 + 4 * 24.0) * nl;   // W, S^-1 planes + b read; y, r, z, p written
  else if (h->plan.own.grp_B > 1) out->algorithmic_bytes = (8.0 * 3 * h->plan.own.grp_nb + 24.0 + 4 * 24.0) * nl;
  else out->algorithmic_bytes = (48.0 + 24.0 + 4 * 24.0) * nl;
  out->ms_avg = ms;
  out->units = h->S.n_loc;
  return PGO_OK;
}

}  // extern "C"

