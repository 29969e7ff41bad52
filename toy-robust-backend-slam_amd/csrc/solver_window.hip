// pgo_window_solve (include/pgo.h, "window solves"): the host half.  Every list of the call is checked and resolved here --
// caller's pose -> row of the handle's pose array, caller's edge -> local edge, endpoints -> list positions, and the
// contribution list of every 3x3 block of the window's J'J -- before anything is launched; then ONE launch of
// k_window_solve (window.hip.h), one workgroup per window, and one copy-out.
#include "solver_handle.hip.h"
#include "window.hip.h"

int pgo_handle::win_reserve(void** buf, int64_t* cap, int64_t bytes) {
  if (bytes <= *cap) return PGO_OK;
  const int64_t want = std::max<int64_t>(bytes, 2 * *cap);
  void* q = nullptr;
  hipError_t e = hipMalloc(&q, (size_t)want);
  if (e != hipSuccess) return fail(PGO_ERR_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
  if (*buf) {   // (the stream is idle: every call that uses the buffer ends with a synchronisation)
    allocs.erase(std::remove(allocs.begin(), allocs.end(), *buf), allocs.end());
    (void)hipFree(*buf);
    device_bytes -= *cap;
  }
  allocs.push_back(q);
  device_bytes += want;
  *buf = q;
  *cap = want;
  return PGO_OK;
}

int pgo_handle::window_solve(const char* who, int32_t nw, const int32_t* pose_ptr, const int32_t* pose_idx, const int32_t* edge_ptr,
                             const int32_t* edge_idx, const int32_t* anchor, int32_t max_iters, int32_t commit, double* poses_out,
                             pgo_window_result* results, pgo_iter_record* records) {
  const std::string W = std::string(who) + ": ";
  if (opt.method != 0 && opt.method != 1) return fail(PGO_ERR_UNSUPPORTED, W + "METHOD 0 and 1 only");
  if (opt.info_weighting || info_mode) return fail(PGO_ERR_UNSUPPORTED, W + "info_weighting is not supported");
  if (comm || force_collectives) return fail(PGO_ERR_UNSUPPORTED, W + "one rank without a communicator only");
  if (w_set)   // (k_window_solve evaluates the edges itself and does not read the plane)
    return fail(PGO_ERR_UNSUPPORTED, W + "not while edge weights are set (pgo_set_edge_weights(h, NULL) first)");
  if (nw < 0) return fail(PGO_ERR_INVALID_ARG, W + "n_windows < 0");
  if (nw == 0) return PGO_OK;
  if (!pose_ptr || !pose_idx || !edge_ptr || !edge_idx || !anchor || !results) return fail(PGO_ERR_INVALID_ARG, W + "null pointer");
  if (max_iters < 1 || max_iters > PGO_WINDOW_MAX_ITERS)
    return fail(PGO_ERR_INVALID_ARG, W + "max_iters must be 1.." + std::to_string(PGO_WINDOW_MAX_ITERS));
  if (pose_ptr[0] != 0 || edge_ptr[0] != 0) return fail(PGO_ERR_INVALID_ARG, W + "pose_ptr[0] and edge_ptr[0] must be 0");
  for (int32_t w = 0; w < nw; ++w)
    if (pose_ptr[w + 1] < pose_ptr[w] || edge_ptr[w + 1] < edge_ptr[w])
      return fail(PGO_ERR_INVALID_ARG, W + "window " + std::to_string(w) + ": pose_ptr / edge_ptr must not decrease");
  for (int32_t w = 0; w < nw; ++w) {
    const int32_t np = pose_ptr[w + 1] - pose_ptr[w], ne = edge_ptr[w + 1] - edge_ptr[w];
    if (np > PGO_WINDOW_MAX_POSES || ne > PGO_WINDOW_MAX_EDGES)
      return fail(PGO_ERR_UNSUPPORTED, W + "window " + std::to_string(w) + " has " + std::to_string(np) + " poses and " + std::to_string(ne) +
                                           " edges: above the cap of " + std::to_string(PGO_WINDOW_MAX_POSES) + " / " +
                                           std::to_string(PGO_WINDOW_MAX_EDGES) + " (use pgo_set_active)");
  }
  const int64_t N = S.n_poses, EL = S.n_edges_local, TP = pose_ptr[nw], TE = edge_ptr[nw];
  if (win_edge_local.empty() && EL > 0) {   // (one rank: every edge is local)
    win_edge_local.assign((size_t)n_edges_total, -1);
    for (int64_t k = 0; k < EL; ++k) win_edge_local[S.orig_edge[k]] = (int32_t)k;
  }
  if (win_pos.empty()) {
    win_pos.assign((size_t)N, -1);
    win_owner.assign((size_t)N, -1);
  }
  // ---- host image: desc | pidx | eloc | eab | blk | blk_ptr | ent  (blocks <= poses + edges, contributions <= 3 x edges)
  const int64_t o_desc = 0, o_pidx = o_desc + 8 * (int64_t)nw, o_eloc = o_pidx + TP, o_eab = o_eloc + TE, o_blk = o_eab + TE,
                o_bptr = o_blk + TP + TE, o_ent = o_bptr + TP + TE + 1, n_int = o_ent + 3 * TE;
  win_host.assign((size_t)n_int, 0);
  int32_t* M = win_host.data();
  int64_t n_blk = 0, n_ent = 0;
  int n3cap = 3;
  int status = PGO_OK;
  std::string msg;
  auto bad = [&](int32_t w, const std::string& what) {
    status = PGO_ERR_INVALID_ARG;
    msg = W + "window " + std::to_string(w) + ": " + what;
  };
  for (int32_t w = 0; w < nw && status == PGO_OK; ++w) {
    const int32_t p0 = pose_ptr[w], np = pose_ptr[w + 1] - p0, e0 = edge_ptr[w], ne = edge_ptr[w + 1] - e0;
    int32_t listed = 0;
    for (int32_t k = 0; k < np && status == PGO_OK; ++k) {
      const int32_t i = pose_idx[p0 + k];
      if (i < 0 || i >= N) {
        bad(w, "pose index " + std::to_string(i) + " out of range");
        break;
      }
      const int32_t row = perm.empty() ? i : perm[i];
      if (win_pos[row] >= 0) {
        bad(w, "pose " + std::to_string(i) + " is listed twice");
        break;
      }
      if (commit && win_owner[row] >= 0) {
        bad(w, "pose " + std::to_string(i) + " is also in window " + std::to_string(win_owner[row]) + " (commit needs disjoint lists)");
        break;
      }
      win_pos[row] = k;
      win_owner[row] = w;
      M[o_pidx + p0 + k] = row;
      listed = k + 1;
    }
    int32_t anchor_pos = -1;
    if (status == PGO_OK) {
      const int32_t a = anchor[w];
      if (a < 0 || a >= N || win_pos[perm.empty() ? a : perm[a]] < 0) bad(w, "the anchor " + std::to_string(a) + " is not in the pose list");
      else anchor_pos = win_pos[perm.empty() ? a : perm[a]];
    }
    win_sort.clear();
    for (int32_t k = 0; k < ne && status == PGO_OK; ++k) {
      const int32_t e = edge_idx[e0 + k];
      if (e < 0 || e >= n_edges_total || win_edge_local[e] < 0) {
        bad(w, "edge index " + std::to_string(e) + " out of range");
        break;
      }
      const int32_t l = win_edge_local[e], pa = win_pos[S.ia[l]], pb = win_pos[S.ib[l]];
      if (pa < 0 || pb < 0) {
        bad(w, "an endpoint of edge " + std::to_string(e) + " is not in the pose list");
        break;
      }
      M[o_eloc + e0 + k] = l;
      M[o_eab + e0 + k] = pa | (pb << 8);
      // contributions, keyed (block, listed edge): sorting keeps every block's contributions in list order
      const uint32_t hi = (uint32_t)std::max(pa, pb), lo = (uint32_t)std::min(pa, pb), side_hi = pa > pb ? 0u : 1u;
      win_sort.push_back((uint32_t)pa << 17 | (uint32_t)pa << 9 | (uint32_t)k << 1 | 0u);
      win_sort.push_back((uint32_t)pb << 17 | (uint32_t)pb << 9 | (uint32_t)k << 1 | 1u);
      win_sort.push_back(1u << 25 | hi << 17 | lo << 9 | (uint32_t)k << 1 | side_hi);
    }
    for (int32_t k = 0; k < listed; ++k) win_pos[M[o_pidx + p0 + k]] = -1;   // idle again, whatever happened
    if (status != PGO_OK) break;
    std::sort(win_sort.begin(), win_sort.end());
    int32_t* D = M + o_desc + 8 * (int64_t)w;
    D[0] = p0;
    D[1] = np;
    D[2] = e0;
    D[3] = ne;
    D[4] = anchor_pos;
    D[5] = (int32_t)n_blk;
    size_t c = 0;
    for (int32_t p = 0; p < np; ++p) {   // the diagonal blocks first, one per listed pose (empty: a pose without an edge)
      M[o_blk + n_blk] = p | (p << 8);
      M[o_bptr + n_blk] = (int32_t)n_ent;
      ++n_blk;
      for (; c < win_sort.size() && (win_sort[c] >> 17) == (uint32_t)p; ++c) M[o_ent + n_ent++] = (int32_t)(win_sort[c] & 511u);
    }
    while (c < win_sort.size()) {        // then the blocks (p, q), p > q, that an edge joins
      const uint32_t key = win_sort[c] >> 9;
      M[o_blk + n_blk] = (int32_t)((key >> 8) & 255u) | (int32_t)((key & 255u) << 8);
      M[o_bptr + n_blk] = (int32_t)n_ent;
      ++n_blk;
      for (; c < win_sort.size() && (win_sort[c] >> 9) == key; ++c) M[o_ent + n_ent++] = (int32_t)(win_sort[c] & 511u);
    }
    D[6] = (int32_t)n_blk - D[5];
    n3cap = std::max(n3cap, 3 * np);
  }
  M[o_bptr + n_blk] = (int32_t)n_ent;
  for (int64_t k = 0; k < TP; ++k) {   // (rows recorded so far; on an error the tail of the image is still 0)
    const int32_t row = M[o_pidx + k];
    if (row >= 0 && row < N) win_owner[row] = -1;
  }
  if (status != PGO_OK) return fail(status, msg);

  // ---- device
  HIPC(hipSetDevice(device));
  const int64_t rec_rows = (int64_t)max_iters + 1;
  auto up16 = [](int64_t b) { return (b + 15) / 16 * 16; };
  const int64_t b_rec = 0, b_out = b_rec + up16(TE * dev::WIN_REC * 8), b_res = b_out + up16(TP * 3 * 8),
                b_its = b_res + up16((int64_t)nw * (int64_t)sizeof(pgo_window_result)),
                b_all = b_its + (records ? up16((int64_t)nw * rec_rows * (int64_t)sizeof(pgo_iter_record)) : 0);
  PGOC(win_reserve(&win_in, &win_in_cap, n_int * 4));
  PGOC(win_reserve(&win_work, &win_work_cap, std::max<int64_t>(b_all, 16)));
  const size_t lds_max = (size_t)dev::win_lds_doubles(3 * PGO_WINDOW_MAX_POSES) * sizeof(double);
  if (!win_lds_set) {   // more than 64 KiB of LDS needs the kernel's dynamic-LDS attribute
    HIPC(hipFuncSetAttribute(reinterpret_cast<const void*>(&dev::k_window_solve<>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
    win_lds_set = true;
  }
  HIPC(hipMemcpyAsync(win_in, M, (size_t)n_int * 4, hipMemcpyHostToDevice, stream));
  char* wk = static_cast<char*>(win_work);
  if (records) HIPC(hipMemsetAsync(wk + b_its, 0, (size_t)(b_all - b_its), stream));
  const int32_t* I = static_cast<const int32_t*>(win_in);
  dev::WinArgs A;
  A.win = reinterpret_cast<const dev::WinDesc*>(I + o_desc);
  A.pidx = I + o_pidx;
  A.eloc = I + o_eloc;
  A.eab = I + o_eab;
  A.blk = I + o_blk;
  A.blk_ptr = I + o_bptr;
  A.ent = I + o_ent;
  A.poses = poses;
  A.mx = e_mx;
  A.my = e_my;
  A.mt = e_mt;
  A.flags = e_flags;
  A.phi = opt.phi;
  A.loss0 = loss_cls[0];
  A.loss1 = loss_cls[1];
  A.loss2 = loss_cls[2];
  A.loss3 = loss_cls[3];
  A.max_iters = max_iters;
  A.jacobi_scaling = opt.jacobi_scaling;
  A.commit = commit ? 1 : 0;
  A.n3cap = n3cap;
  A.ftol = opt.ftol;
  A.gtol = opt.gtol;
  A.ptol = opt.ptol;
  A.radius0 = opt.radius0;
  A.max_radius = opt.max_radius;
  A.min_radius = opt.min_radius;
  A.min_relative_decrease = opt.min_relative_decrease;
  A.min_lm_diagonal = opt.min_lm_diagonal;
  A.max_lm_diagonal = opt.max_lm_diagonal;
  A.rec = reinterpret_cast<double*>(wk + b_rec);
  A.poses_out = reinterpret_cast<double*>(wk + b_out);
  A.results = reinterpret_cast<pgo_window_result*>(wk + b_res);
  A.records = records ? reinterpret_cast<pgo_iter_record*>(wk + b_its) : nullptr;
  const size_t lds = (size_t)dev::win_lds_doubles(n3cap) * sizeof(double);
  hipLaunchKernelGGL(dev::k_window_solve<>, dim3(nw), dim3(dev::WIN_WG), lds, stream, A);
  PGOC(check_launch("k_window_solve"));
  if (poses_out && TP > 0) HIPC(hipMemcpyAsync(poses_out, wk + b_out, (size_t)TP * 3 * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPC(hipMemcpyAsync(results, wk + b_res, (size_t)nw * sizeof(pgo_window_result), hipMemcpyDeviceToHost, stream));
  if (records) HIPC(hipMemcpyAsync(records, wk + b_its, (size_t)nw * rec_rows * sizeof(pgo_iter_record), hipMemcpyDeviceToHost, stream));
  if (commit) {   // as pgo_set_poses: the running solve (if any) is stale
    lin_valid = false;
    lm_active = false;
  }
  return sync();
}

extern "C" int pgo_window_solve(pgo_t* h, int32_t n_windows, const int32_t* pose_ptr, const int32_t* pose_idx, const int32_t* edge_ptr,
                                const int32_t* edge_idx, const int32_t* anchor, int32_t max_iters, int32_t commit, double* poses_out,
                                pgo_window_result* results, pgo_iter_record* records) {
  if (!h) return fail(PGO_ERR_INVALID_ARG, "pgo_window_solve: null handle");
  if (h->batch_mode) return fail(PGO_ERR_INVALID_ARG, "pgo_window_solve: a batched handle takes pgo_batch_window_solve");
  return h->window_solve("pgo_window_solve", n_windows, pose_ptr, pose_idx, edge_ptr, edge_idx, anchor, max_iters, commit, poses_out,
                         results, records);
}
