// The direct linear solve for small chain-like graphs (kernels: direct.hip.h; choice and buffers: solver_create.hip).
#include "solver_handle.hip.h"

// The factorisation every solve starts with, for the system in hd / d2 (LM: the damped one; pgo_pose_covariance and
// pgo_edge_gate with solver = 1: D'D = 0): the chain's block LDL' and prefix products, Z = T^-1 V' and t = T^-1 rhs
// (the separators' columns and Schur complement with them), the capacitance matrix I + V Z with V t, its Cholesky
// factor and explicit inverse.  L receives the argument blocks of the launches for what follows.
int pgo_handle::direct_factor(const double* rhs, bool fine_prefix, DirectLaunch* L) {
  const int n = S.n_loc, K = plan.dl.dl_K, Kp = plan.dl.dl_Kp, nb = plan.dl.dl_Kp / 32;
  dev::DlrArgs& A = L->A;
  A.n = n;
  A.m = plan.dl.dl_m;
  A.K = K;
  A.Kp = Kp;
  A.ld = plan.dl.dl_ld;
  A.jr = jr;
  A.scale = scale;
  A.d2 = d2;
  A.e_ia = e_ia;
  A.e_ib = e_ib;
  A.chain_edge = dl_chain_edge;
  A.lr_edge = dl_lr_edge;
  A.va = dl_va;
  A.vb = dl_vb;
  A.trec = dl_trec;
  A.fac = dl_fac;
  A.vrec = dl_vrec;
  A.Z = dl_Z;
  A.cap = dl_cap;
  A.dwork = dl_dwork;
  A.cvec = dl_cvec;
  A.nsep = plan.dl.dl_nsep;
  for (int j = 0; j < dev::DLR_MAX_SEP; ++j) A.sep[j] = plan.dl.dl_sep[j];
  A.ksep = dl_ksep;
  A.sw_js = has_sw ? sw_js : nullptr;
  A.sw_c = has_sw ? sw_c : nullptr;
  A.rec_n = rec_doubles;
  A.rec_info = info_mode ? 1 : 0;
  A.prior = pri_n > 0 ? pri_dense : nullptr;
  hipLaunchKernelGGL(dev::k_dlr_setup<>, dim3((n + plan.dl.dl_m + 255) / 256), dim3(256), 0, stream, A);
  PGOC(check_launch("k_dlr_setup"));
  hipLaunchKernelGGL(dev::k_dlr_factor<>, dim3(plan.dl.dl_nsep + 1), dim3(64), 0, stream, (const double*)dl_trec, n, dl_fac, A);
  PGOC(check_launch("k_dlr_factor"));
  hipLaunchKernelGGL(dev::k_dlr_prefix<>, dim3(1), dim3(128), 0, stream, (const double*)dl_fac, n, plan.dl.dl_nseg, plan.dl.dl_seglen, dl_pre);
  PGOC(check_launch("k_dlr_prefix"));
  if (fine_prefix) {   // the refinement's single column: k_dlr_solve1
    hipLaunchKernelGGL(dev::k_dlr_prefix<>, dim3(1), dim3(512), 0, stream, (const double*)dl_fac, n, plan.dl.dl_nseg2, plan.dl.dl_seglen2, dl_pre2);
    PGOC(check_launch("k_dlr_prefix (fine segments)"));
  }
  dev::DlrColsArgs& C = L->C;
  C.fac = dl_fac;
  C.pre = dl_pre;
  C.n = n;
  C.ncols = K + 1 + plan.dl.dl_nU;
  C.K = K;
  C.vec_col = K;
  C.ld = plan.dl.dl_ld;
  C.ucol0 = K + 1;
  C.nsep = plan.dl.dl_nsep;
  for (int j = 0; j < dev::DLR_MAX_SEP; ++j) C.sep[j] = plan.dl.dl_sep[j];
  C.ksep = dl_ksep;
  C.nseg = plan.dl.dl_nseg;
  C.seglen = plan.dl.dl_seglen;
  C.vrec = dl_vrec;
  C.va = dl_va;
  C.vb = dl_vb;
  C.rhs_b = rhs;
  C.rhs_sub = nullptr;
  C.X = dl_Z;
  C.E = dl_E;
  C.E2 = dl_E2;
  PGOC(direct_sweep(C));
  // the couplings at the separators (k_dlr_sep_*): Y = the U columns of this solve, R once per factorisation
  dev::DlrSepArgs& SA = L->SA;
  SA.nsep = plan.dl.dl_nsep;
  SA.nU = plan.dl.dl_nU;
  SA.n = n;
  for (int j = 0; j < dev::DLR_MAX_SEP; ++j) SA.sep[j] = plan.dl.dl_sep[j];
  SA.ksep = dl_ksep;
  SA.Y = dl_Z + (K + 1);
  SA.yld = plan.dl.dl_ld;
  SA.Sinv = dl_R;
  SA.trec = dl_trec;
  SA.Wm = dl_Wm;
  if (plan.dl.dl_nsep > 0) {
    SA.X = dl_Z;
    SA.ld = plan.dl.dl_ld;
    SA.ncols = K + 1;
    hipLaunchKernelGGL(dev::k_dlr_sep_system<>, dim3(1), dim3(256), 0, stream, SA);
    PGOC(check_launch("k_dlr_sep_system"));
  }
  PGOC(direct_separator_fix(SA, dl_Z, plan.dl.dl_ld, K + 1));
  hipLaunchKernelGGL(dev::k_dlr_cap<>, dim3((std::max(Kp, K + 1) + 255) / 256, Kp), dim3(256), 0, stream, A);
  PGOC(check_launch("k_dlr_cap"));
  for (int kb = 0; kb < nb; ++kb) {
    hipLaunchKernelGGL(dev::k_chol_panel<>, dim3(std::max(1, nb - 1)), dim3(dev::CHOL_THREADS), dev::CHOL_LDS_BYTES, stream, dl_cap, dl_nm, dl_dwork, Kp, nb, kb);
    PGOC(check_launch("k_chol_panel"));
  }
  return PGO_OK;
}

// T^-1 on the columns of Q: the three sweeps (panel_rhs: the right-hand sides stand in Q.X -- k_dlr_fwd_panel)
int pgo_handle::direct_sweep(const dev::DlrColsArgs& Q, bool panel_rhs) {
  const dim3 grid((Q.ncols + 255) / 256, Q.nseg);
  if (panel_rhs) hipLaunchKernelGGL(dev::k_dlr_fwd_panel<>, grid, dim3(256), 0, stream, Q);
  else hipLaunchKernelGGL(dev::k_dlr_fwd<>, grid, dim3(256), 0, stream, Q);
  hipLaunchKernelGGL(dev::k_dlr_mid<>, grid, dim3(256), 0, stream, Q);
  hipLaunchKernelGGL(dev::k_dlr_fix<>, grid, dim3(256), 0, stream, Q);
  return check_launch("k_dlr_fwd / _mid / _fix");
}

// the separators' correction of the columns X [3n][ld] (Y and R of the factorisation in SA)
int pgo_handle::direct_separator_fix(const dev::DlrSepArgs& SA, double* X, int ld, int ncols) {
  if (plan.dl.dl_nsep == 0) return PGO_OK;
  dev::DlrSepArgs Q = SA;
  Q.X = X;
  Q.ld = ld;
  Q.ncols = ncols;
  hipLaunchKernelGGL(dev::k_dlr_sep_w<>, dim3((ncols + 255) / 256), dim3(256), 0, stream, Q);
  hipLaunchKernelGGL(dev::k_dlr_sep_apply<>, dim3((ncols + 255) / 256, (3 * (int)S.n_loc + 63) / 64), dim3(256), 0, stream, Q);
  return check_launch("k_dlr_sep_w / _apply");
}

// T <- (T + V'V)^-1 T for the P.ld columns of a panel, after direct_factor():  X0 = T^-1 B (sweeps on the pre-filled
// panel, separators),  G = V X0,  W = N'(N G),  X = X0 - Z W  (the three products on the matrix cores: k_dlr_gemm)
int pgo_handle::direct_panel_solve(const DirectLaunch& L, const DirectPanel& P) {
  const int n = S.n_loc, K = plan.dl.dl_K, Kp = plan.dl.dl_Kp;
  dev::DlrColsArgs C = L.C;
  C.ncols = P.ld;
  C.K = 0;
  C.vec_col = -1;
  C.ld = P.ld;
  C.nsep = 0;   // (no U columns: Y and R of the factorisation are reused)
  C.rhs_b = C.rhs_sub = nullptr;
  C.X = P.T;
  C.E = P.E;
  C.E2 = P.E2;
  PGOC(direct_sweep(C, true));
  dev::DlrSepArgs SA = L.SA;
  SA.Wm = P.Wm;
  PGOC(direct_separator_fix(SA, P.T, P.ld, P.ld));
  if (K == 0) return PGO_OK;
  hipLaunchKernelGGL(dev::k_dlr_vdot_panel<>, dim3((P.ld + 255) / 256, Kp), dim3(256), 0, stream, L.A, (const double*)P.T, P.ld, P.G);
  PGOC(check_launch("k_dlr_vdot_panel"));
  dev::DlrGemmArgs Q;
  Q.ldb = Q.ldc = P.ld;
  Q.K = Q.kvalid = Kp;
  const dim3 gk(P.ld / 64, (Kp + 63) / 64), gn(P.ld / 64, (3 * n + 63) / 64);
  Q.A = dl_nm;   // Y = N G
  Q.lda = Kp;
  Q.B = P.G;
  Q.C = P.Y;
  Q.M = Kp;
  Q.tri = 1;
  Q.sub = 0;
  hipLaunchKernelGGL(dev::k_dlr_gemm<0>, gk, dim3(256), 0, stream, Q);
  Q.B = P.Y;     // W = N' Y (into G)
  Q.C = P.G;
  Q.tri = 2;
  hipLaunchKernelGGL(dev::k_dlr_gemm<1>, gk, dim3(256), 0, stream, Q);
  Q.A = dl_Z;    // X = X0 - Z W
  Q.lda = plan.dl.dl_ld;
  Q.B = P.G;
  Q.C = P.T;
  Q.M = 3 * n;
  Q.kvalid = K;
  Q.tri = 0;
  Q.sub = 1;
  hipLaunchKernelGGL(dev::k_dlr_gemm<0>, gn, dim3(256), 0, stream, Q);
  return check_launch("k_dlr_gemm");
}

// (H + D'D) y = rhs by Woodbury on chain + low rank, then refine steps of iterative refinement against the assembled
// matrix; leaves the true residual in r (the model-decrease identity of lm_iteration_tail reads it) and |r|^2, |rhs|^2 in
// scal[8..9].  LM passes gs and dl_refine; pgo_debug_direct_solve any right-hand side and 0..3 steps.
int pgo_handle::direct_enqueue(const double* rhs, int refine) {
  const int n = S.n_loc, K = plan.dl.dl_K, Kp = plan.dl.dl_Kp, nb = plan.dl.dl_Kp / 32;
  const bool one_launch = refine > 0 && dl_pre2 != nullptr;   // the refinement's single column: k_dlr_solve1
  DirectLaunch L;
  PGOC(direct_factor(rhs, one_launch, &L));
  const dev::DlrArgs& A = L.A;
  const dev::DlrColsArgs& C = L.C;
  const dev::DlrSepArgs& SA = L.SA;
  auto capacitance_solve = [&]() -> int {  // cvec <- (L L')^-1 cvec = N' (N cvec)
    hipLaunchKernelGGL(dev::k_tri_apply<>, dim3(nb), dim3(256), 0, stream, (const double*)dl_nm, Kp, nb, (const double*)dl_cvec, dl_cy, 0);
    hipLaunchKernelGGL(dev::k_tri_apply<>, dim3(nb), dim3(256), 0, stream, (const double*)dl_nm, Kp, nb, (const double*)dl_cy, dl_cvec, 1);
    return check_launch("k_tri_apply");
  };
  PGOC(capacitance_solve());
  hipLaunchKernelGGL(dev::k_dlr_combine<>, dim3((3 * n + 3) / 4), dim3(256), 0, stream, (const double*)dl_Z, plan.dl.dl_ld, K, (const double*)dl_cvec,
                     (const double*)dl_Z, plan.dl.dl_ld, K, 3 * n, y, 0);
  PGOC(check_launch("k_dlr_combine"));
  auto residual_product = [&]() -> int {  // ap = (H + D'D) y
    PGOC(scatter_owned(y));
    return spmv_enqueue(p_full, ap, part[0], 1, nullptr);
  };
  for (int it = 0; it < refine; ++it) {
    PGOC(residual_product());
    int xld = 64;   // layout of the single column in dl_x1: [3n][64] (batched kernels) or a plain vector (k_dlr_solve1)
    if (one_launch) {
      dev::DlrSolve1Args Q;
      Q.fac = dl_fac;
      Q.pre2 = dl_pre2;
      Q.n = n;
      Q.nseg = plan.dl.dl_nseg2;
      Q.seglen = plan.dl.dl_seglen2;
      Q.rhs_b = rhs;
      Q.rhs_sub = ap;
      Q.x = dl_x1;
      Q.nsep = plan.dl.dl_nsep;
      Q.nU = plan.dl.dl_nU;
      for (int j = 0; j < dev::DLR_MAX_SEP; ++j) Q.sep[j] = plan.dl.dl_sep[j];
      Q.ksep = dl_ksep;
      Q.trec = dl_trec;
      Q.Y = dl_Z + (K + 1);
      Q.yld = plan.dl.dl_ld;
      Q.Sinv = dl_R;
      hipLaunchKernelGGL(dev::k_dlr_solve1<>, dim3(1), dim3(256), 0, stream, Q);
      PGOC(check_launch("k_dlr_solve1"));
      xld = 1;
    } else {
      dev::DlrColsArgs C1 = C;
      C1.ncols = 1;
      C1.K = 0;
      C1.vec_col = 0;
      C1.ld = 64;
      C1.rhs_sub = ap;
      C1.X = dl_x1;
      C1.nsep = 0;   // (no U columns: Y and R of the main solve are reused)
      PGOC(direct_sweep(C1));
      PGOC(direct_separator_fix(SA, dl_x1, 64, 1));
    }
    hipLaunchKernelGGL(dev::k_dlr_vdot<>, dim3((Kp + 255) / 256), dim3(256), 0, stream, A, (const double*)dl_x1, xld, 0, dl_cvec);
    PGOC(check_launch("k_dlr_vdot"));
    PGOC(capacitance_solve());
    hipLaunchKernelGGL(dev::k_dlr_combine<>, dim3((3 * n + 3) / 4), dim3(256), 0, stream, (const double*)dl_Z, plan.dl.dl_ld, K, (const double*)dl_cvec,
                       (const double*)dl_x1, xld, 0, 3 * n, y, 1);
    PGOC(check_launch("k_dlr_combine"));
  }
  PGOC(residual_product());
  hipLaunchKernelGGL(dev::k_dlr_resid<>, dim3((3 * n + 255) / 256), dim3(256), 0, stream, (int64_t)3 * n, rhs, (const double*)ap, r);
  PGOC(check_launch("k_dlr_resid"));
  hipLaunchKernelGGL(dev::k_dot<>, dim3(plan.own.g_flat), dim3(dev::WG), 0, stream, (int64_t)3 * n, (const double*)r, (const double*)r, part[2]);
  hipLaunchKernelGGL(dev::k_dot<>, dim3(plan.own.g_flat), dim3(dev::WG), 0, stream, (int64_t)3 * n, rhs, rhs, part[4]);
  PGOC(check_launch("k_dot"));
  return reduce_to_scal({{part[2], plan.own.g_flat, 0}, {part[4], plan.own.g_flat, 0}}, 8);
}

// The ~130 launches of a direct solve are the same every time, but replaying them from a captured hipGraph was measured
// to gain nothing in GN it/s (the solve is bound by its dependent kernels, not by the host), while capture + instantiation
// cost ~5 ms, as much as five LM iterations of a fresh handle: they are launched eagerly.
int pgo_handle::direct_solve() {
  PGOC(direct_enqueue(gs, plan.dl.dl_refine));
  if (plan.dl.dl_fail_at > 0 && iter == plan.dl.dl_fail_at)   // test hook ("direct_fail_at"): a direct solve that returns NaNs
    HIPC(hipMemsetAsync(y, 0xFF, (size_t)3 * S.n_loc * sizeof(double), stream));
  return PGO_OK;
}

