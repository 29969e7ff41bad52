"""toy-robust-backend-slam_amd: MI355X-native 2D pose-graph backend (DCS path of
wei-ght/toy-robust-backend-slam), Python binding over the C-ABI in include/pgo.h.

This module is a thin ctypes layer: all computation happens in libpgo.so (hand-written HIP
kernels for gfx950).  There is no CPU fallback -- solver entry points raise PgoError when no
gfx950 device is visible or the library is missing.

Names follow the reference (DCS-ceres/include/g2o_util.h, main.cpp):
    ReadG2O(path)            load + classify a g2o file            g2o_util.h:23-89
    .add_random_C(n, seed)   inject bogus loops                    g2o_util.h:151-171
    .writePoseGraph_nodes / .writePoseGraph_edges                  g2o_util.h:93-112
    Solver(graph, options)   problem assembly + ceres::Solve       main.cpp:66-163
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _build

__all__ = ["PgoError", "Options", "Summary", "IterRecord", "ReadG2O", "Graph", "Solver", "Batch", "Comm", "lib", "build",
           "HandleInfo", "synth_manhattan", "solve_batch", "shard_plan", "shard_halo", "pose_order", "set_knob", "KernelStats", "SoloResult", "EXPORTS", "TERMINATION",
           "CovarianceOptions", "CovarianceReport", "Loss", "LOSS_TYPES", "active_plan", "EdgeGateResult", "gate_evaluate",
           "GateJointOptions", "GateJointResult", "GateJointSummary", "gate_joint_evaluate", "GATE_JOINT_MAX",
           "window_plan", "WindowResult", "WINDOW_MAX_POSES", "WINDOW_MAX_EDGES", "WINDOW_MAX_ITERS",
           "synth_manhattan_truth", "trajectory_error", "TrajOptions", "TrajError", "EdgeWeight", "SCORE_POSES_PER_WG",
           "coarsen_plan", "coarsen_info_plan", "prolong_eval", "COARSEN_MIN_STRIDE", "COARSEN_MAX_STRIDE",
           "gnc_weight_eval", "GncStats", "GncOptions", "GncRound", "GncSummary",
           "loop_support_plan", "LoopSupportOptions", "LoopSupportRecord", "LoopSupportStats", "LOOP_SUPPORT_MAX_WINDOW",
           "chordal_plan", "ChordalOptions", "ChordalSolve", "ChordalSummary", "CHORDAL_MAX_ROUNDS",
           "mixture_eval", "mixture_plan", "MixStats", "MixtureOptions", "MixtureRound", "MixtureSummary", "MIX_MAX_COMPONENTS",
           "prior_eval", "SampleOptions", "sample_noise_eval"]

EDGE_ODOMETRY, EDGE_CLOSURE, EDGE_BOGUS = 0, 1, 2
TERMINATION = {1: "CONVERGENCE_FTOL", 2: "CONVERGENCE_GTOL", 3: "CONVERGENCE_PTOL", 4: "NO_CONVERGENCE",
               5: "MIN_RADIUS", 6: "FAILURE", 0: "RUNNING"}

# every symbol include/pgo.h declares (tests check the library exports each one)
EXPORTS = [
    "pgo_strerror", "pgo_last_error", "pgo_version",
    "pgo_g2o_load", "pgo_g2o_parse", "pgo_graph_from_arrays", "pgo_graph_free",
    "pgo_graph_num_poses", "pgo_graph_num_edges", "pgo_graph_num_edges_of_kind", "pgo_graph_pose_ids",
    "pgo_graph_poses", "pgo_graph_edge_a", "pgo_graph_edge_b", "pgo_graph_edge_meas", "pgo_graph_edge_info",
    "pgo_graph_edge_kind", "pgo_inject_outliers", "pgo_write_nodes", "pgo_write_edges", "pgo_write_g2o",
    "pgo_synth_manhattan", "pgo_options_default",
    "pgo_comm_unique_id", "pgo_comm_create_rccl", "pgo_comm_create_shm", "pgo_comm_destroy",
    "pgo_create", "pgo_create_weighted", "pgo_create_from_graph", "pgo_destroy", "pgo_eval", "pgo_edge_chi2", "pgo_solve", "pgo_solve_batch",
    "pgo_batch_create", "pgo_batch_destroy", "pgo_batch_size", "pgo_batch_solve", "pgo_batch_get_poses", "pgo_batch_set_poses",
    "pgo_batch_num_iter_records", "pgo_batch_get_iter_records", "pgo_lm_begin", "pgo_lm_step",
    "pgo_num_iter_records", "pgo_get_iter_records", "pgo_get_info", "pgo_get_poses", "pgo_set_poses", "pgo_get_switches",
    "pgo_write_switches",
    "pgo_bench_eval", "pgo_bench_assemble", "pgo_bench_spmv", "pgo_bench_precond", "pgo_debug_precond", "pgo_debug_spmv", "pgo_debug_system_spmv", "pgo_debug_direct_solve", "pgo_debug_normal_eq",
    "pgo_batch_debug_solve",
    "pgo_debug_set_knob",
    "pgo_shard_plan", "pgo_shard_halo", "pgo_pose_order",
    "pgo_covariance_options_default", "pgo_pose_covariance",
    "pgo_loss_evaluate", "pgo_set_losses", "pgo_batch_set_losses",
    "pgo_set_active", "pgo_batch_set_active", "pgo_active_plan",
    "pgo_gate_evaluate", "pgo_edge_gate",
    "pgo_gate_joint_options_default", "pgo_gate_joint_evaluate", "pgo_edge_gate_joint",
    "pgo_window_plan", "pgo_window_solve", "pgo_batch_window_solve",
    "pgo_synth_manhattan_truth", "pgo_traj_options_default", "pgo_trajectory_error_eval", "pgo_trajectory_error", "pgo_edge_weights",
    "pgo_coarsen_plan", "pgo_prolong_eval", "pgo_coarsen", "pgo_prolong", "pgo_coarsen_info_plan", "pgo_coarsen_info",
    "pgo_set_edge_weights", "pgo_get_edge_weights", "pgo_gnc_options_default", "pgo_gnc_weight_eval", "pgo_gnc_update", "pgo_gnc_solve",
    "pgo_loop_support_options_default", "pgo_loop_support_plan", "pgo_loop_support",
    "pgo_chordal_options_default", "pgo_chordal_plan", "pgo_chordal_init",
    "pgo_mixture_options_default", "pgo_mixture_eval", "pgo_mixture_plan", "pgo_set_mixtures", "pgo_set_mixture_null",
    "pgo_mixture_select", "pgo_get_mixture_selection", "pgo_mixture_solve",
    "pgo_set_priors", "pgo_num_priors", "pgo_get_prior_residuals", "pgo_prior_eval",
    "pgo_sample_options_default", "pgo_sample_noise_eval", "pgo_posterior_sample", "pgo_debug_sample_rhs",
]
MIX_MAX_COMPONENTS = 8   # PGO_MIX_MAX_COMPONENTS
CHORDAL_MAX_ROUNDS = 8   # PGO_CHORDAL_MAX_ROUNDS
LOOP_SUPPORT_MAX_WINDOW = 256   # PGO_LOOP_SUPPORT_MAX_WINDOW
COARSEN_MIN_STRIDE, COARSEN_MAX_STRIDE = 2, 256   # PGO_COARSEN_*_STRIDE (include/pgo.h)
SCORE_POSES_PER_WG = 512   # PGO_SCORE_POSES_PER_WG
WINDOW_MAX_POSES, WINDOW_MAX_EDGES, WINDOW_MAX_ITERS = 64, 256, 32   # PGO_WINDOW_MAX_* (include/pgo.h)
GATE_JOINT_MAX = 256   # PGO_GATE_JOINT_MAX
LOSS_TYPES = {"trivial": 0, "huber": 1, "softlone": 2, "cauchy": 3, "arctan": 4, "tukey": 5}   # pgo_loss_type


class PgoError(RuntimeError):
    def __init__(self, status: int, detail: str):
        self.status = status
        super().__init__(f"pgo status {status}: {detail}")


class Options(C.Structure):
    """mirror of pgo_options (include/pgo.h)"""
    _fields_ = [("method", C.c_int32), ("max_iters", C.c_int32), ("fixed_pose", C.c_int32),
                ("jacobi_scaling", C.c_int32),
                ("phi", C.c_double), ("huber_delta", C.c_double), ("ftol", C.c_double), ("gtol", C.c_double),
                ("ptol", C.c_double), ("radius0", C.c_double), ("max_radius", C.c_double), ("min_radius", C.c_double),
                ("min_relative_decrease", C.c_double), ("min_lm_diagonal", C.c_double),
                ("max_lm_diagonal", C.c_double), ("pcg_rtol", C.c_double),
                ("pcg_max_iters", C.c_int32), ("pcg_check_every", C.c_int32), ("verbose", C.c_int32),
                ("use_graphs", C.c_int32), ("pcg_block_poses", C.c_int32), ("halo_exchange", C.c_int32), ("sc_prior_lambda", C.c_double), ("pose_ordering", C.c_int32), ("info_weighting", C.c_int32),
                ("pcg_chain_len", C.c_int32), ("halo_overlap", C.c_int32), ("linear_solver", C.c_int32), ("pcg_coarse_poses", C.c_int32)]

    def __init__(self, **kw):
        super().__init__()
        lib().pgo_options_default(C.byref(self))
        for k, v in kw.items():
            if not hasattr(self, k):
                raise TypeError(f"unknown option {k}")
            setattr(self, k, v)


class IterRecord(C.Structure):
    _fields_ = [("iter", C.c_int32), ("step_ok", C.c_int32), ("cost", C.c_double), ("cost_change", C.c_double),
                ("gradient_max_norm", C.c_double), ("step_norm", C.c_double), ("relative_decrease", C.c_double),
                ("radius", C.c_double), ("pcg_iters", C.c_int32), ("_pad", C.c_int32),
                ("pcg_rel_residual", C.c_double), ("seconds", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "_pad"}


class Summary(C.Structure):
    _fields_ = [("termination", C.c_int32), ("iterations", C.c_int32), ("successful_steps", C.c_int32),
                ("total_pcg_iters", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("seconds_total", C.c_double), ("seconds_eval", C.c_double), ("seconds_assemble", C.c_double),
                ("seconds_linear", C.c_double), ("seconds_candidate", C.c_double)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["termination_name"] = TERMINATION.get(self.termination, "?")
        return d


class HandleInfo(C.Structure):
    """mirror of pgo_handle_info"""
    _fields_ = [("n_poses", C.c_int32), ("n_edges", C.c_int32), ("world", C.c_int32), ("rank", C.c_int32),
                ("row_lo", C.c_int32), ("row_hi", C.c_int32), ("n_edges_local", C.c_int32), ("n_tiles", C.c_int32),
                ("n_incidences", C.c_int64), ("pcg_block_poses", C.c_int32), ("pcg_chain_len", C.c_int32),
                ("chain_kernel", C.c_int32), ("pose_ordering", C.c_int32), ("halo_exchange", C.c_int32),
                ("halo_overlap", C.c_int32), ("halo_send_rows", C.c_int64), ("halo_recv_rows", C.c_int64),
                ("device_bytes", C.c_int64), ("host_enqueue_us_per_pcg_iter", C.c_double), ("pcg_graph_replay", C.c_int32),
                ("linear_solver", C.c_int32), ("direct_rank", C.c_int32), ("direct_fallbacks", C.c_int32), ("direct_switched_at", C.c_int32), ("pcg_coarse_poses", C.c_int32), ("pcg_coarse_rank", C.c_int32),
                ("pcg_single_reduction", C.c_int32), ("pcg_coarse_off_iters", C.c_int32),
                ("direct_separators", C.c_int32), ("direct_segments", C.c_int32), ("direct_refine_kernel", C.c_int32),
                ("n_active_edges", C.c_int32), ("n_constant_poses", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class SoloResult(C.Structure):
    """mirror of pgo_solo_result"""
    _fields_ = [("rz", C.c_double), ("bb", C.c_double), ("rr", C.c_double), ("ydotg", C.c_double), ("yHy", C.c_double),
                ("step2", C.c_double), ("iters", C.c_int32), ("done", C.c_int32)]

    def as_dict(self):
        return {f[0]: getattr(self, f[0]) for f in self._fields_}


class KernelStats(C.Structure):
    _fields_ = [("ms_avg", C.c_double), ("algorithmic_bytes", C.c_double), ("units", C.c_int64)]


class CovarianceOptions(C.Structure):
    """mirror of pgo_covariance_options (defaults: pgo_covariance_options_default)"""
    _fields_ = [("rtol", C.c_double), ("max_iters", C.c_int32), ("poses_per_pass", C.c_int32), ("cross", C.c_int32),
                ("solver", C.c_int32)]

    def __init__(self, **kw):
        super().__init__()
        lib().pgo_covariance_options_default(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("unknown covariance option " + k)
            setattr(self, k, v)


class SampleOptions(C.Structure):
    """mirror of pgo_sample_options (defaults: pgo_sample_options_default)"""
    _fields_ = [("rtol", C.c_double), ("max_iters", C.c_int32), ("samples_per_pass", C.c_int32), ("solver", C.c_int32),
                ("first_sample", C.c_int32), ("seed", C.c_uint64)]

    def __init__(self, **kw):
        super().__init__()
        lib().pgo_sample_options_default(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("unknown sample option " + k)
            setattr(self, k, v)


class Loss(C.Structure):
    """mirror of pgo_loss: Loss("cauchy", 0.1) is ceres::CauchyLoss(0.1); names: LOSS_TYPES.  Loss("trivial") is no loss
    (Ceres' NULL loss; the scale is ignored)."""
    _fields_ = [("type", C.c_int32), ("_pad", C.c_int32), ("a", C.c_double)]

    def __init__(self, name: str = "trivial", a: float = 0.0):
        if name not in LOSS_TYPES:
            raise ValueError(f"unknown loss {name!r} (one of {', '.join(LOSS_TYPES)})")
        super().__init__(LOSS_TYPES[name], 0, float(a))
        self.name = name

    def evaluate(self, s: float):
        """LossFunction::Evaluate: np.array([rho(s), rho'(s), rho''(s)]) (pgo_loss_evaluate, host only)"""
        rho = np.zeros(3)
        _check(lib().pgo_loss_evaluate(C.byref(self), float(s), _dp(rho)))
        return rho

    def __repr__(self):
        return f"Loss({self.name!r}, {self.a!r})"


def _loss_args(losses, edge_class, n_edges):
    """(n, pgo_loss array, edge class pointer or None, keep-alive) for pgo_set_losses / pgo_batch_set_losses"""
    ls = [losses] if isinstance(losses, Loss) else list(losses)
    if not all(isinstance(x, Loss) for x in ls):
        raise TypeError("losses: a Loss or a list of Loss")
    arr = (Loss * max(len(ls), 1))(*ls)
    if edge_class is None:
        return len(ls), arr, None, None
    cls = np.ascontiguousarray(edge_class, np.uint8).reshape(-1)
    if cls.size != n_edges:
        raise ValueError(f"edge_class: {cls.size} entries for {n_edges} edges")
    return len(ls), arr, _bp(cls), cls


class CovarianceReport(C.Structure):
    _fields_ = [("columns", C.c_int32), ("passes", C.c_int32), ("pcg_iters_max", C.c_int32), ("pcg_iters_total", C.c_int32),
                ("max_rel_residual", C.c_double), ("seconds", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class EdgeGateResult(C.Structure):
    """mirror of pgo_edge_gate_result: one candidate of Solver.gate"""
    _fields_ = [("r", C.c_double * 3), ("J", C.c_double * 18), ("P", C.c_double * 9), ("chi2", C.c_double),
                ("chi2_marginal", C.c_double), ("info_gain", C.c_double), ("status", C.c_int32), ("_pad", C.c_int32)]


class GateJointOptions(C.Structure):
    """mirror of pgo_gate_joint_options (defaults: pgo_gate_joint_options_default)"""
    _fields_ = [("chi2_gate", C.c_double), ("min_info_gain", C.c_double)]

    def __init__(self, **kw):
        super().__init__()
        lib().pgo_gate_joint_options_default(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("unknown joint gate option " + k)
            if v is not None:
                setattr(self, k, v)


class GateJointResult(C.Structure):
    """mirror of pgo_gate_joint_result: one candidate of Solver.gate_joint / gate_joint_evaluate"""
    _fields_ = [("r_cond", C.c_double * 3), ("P_cond", C.c_double * 9), ("chi2_cond", C.c_double), ("info_gain_cond", C.c_double),
                ("accepted", C.c_int32), ("status", C.c_int32)]


class GateJointSummary(C.Structure):
    _fields_ = [("n_accepted", C.c_int32), ("_pad", C.c_int32), ("chi2_joint", C.c_double), ("info_gain_joint", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "_pad"}


class WindowResult(C.Structure):
    """mirror of pgo_window_result: one window of Solver.window_solve / Batch.window_solve"""
    _fields_ = [("termination", C.c_int32), ("iterations", C.c_int32), ("successful_steps", C.c_int32),
                ("n_records", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["termination_name"] = TERMINATION.get(self.termination, "?")
        return d


class TrajOptions(C.Structure):
    """mirror of pgo_traj_options (defaults: pgo_traj_options_default)"""
    _fields_ = [("align", C.c_int32), ("rpe_delta", C.c_int32)]

    def __init__(self, **kw):
        super().__init__()
        lib().pgo_traj_options_default(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("unknown trajectory-error option " + k)
            setattr(self, k, int(v))


class TrajError(C.Structure):
    """mirror of pgo_traj_error: the result of trajectory_error / Solver.trajectory_error"""
    _fields_ = [("n_poses", C.c_int32), ("n_pairs", C.c_int32), ("ate_max_pose", C.c_int32), ("rpe_max_pose", C.c_int32),
                ("align_x", C.c_double), ("align_y", C.c_double), ("align_phi", C.c_double),
                ("ate_rmse", C.c_double), ("ate_mean", C.c_double), ("ate_max", C.c_double),
                ("rot_rmse", C.c_double), ("rot_max", C.c_double),
                ("rpe_trans_rmse", C.c_double), ("rpe_trans_max", C.c_double), ("rpe_rot_rmse", C.c_double), ("rpe_rot_max", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class EdgeWeight(C.Structure):
    """mirror of pgo_edge_weight: one edge of Solver.edge_weights"""
    _fields_ = [("s_plain", C.c_double), ("scale", C.c_double), ("rho1", C.c_double), ("weight", C.c_double), ("cost", C.c_double),
                ("active", C.c_int32), ("_pad", C.c_int32)]


class GncStats(C.Structure):
    """mirror of pgo_gnc_stats: what Solver.gnc_update measured over the selected edges"""
    _fields_ = [("s_max", C.c_double), ("weighted_sum", C.c_double), ("n_selected", C.c_int32), ("n_nonbinary", C.c_int32),
                ("n_zero", C.c_int32), ("n_nonfinite", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class GncOptions(C.Structure):
    """mirror of pgo_gnc_options (defaults: pgo_gnc_options_default; cbar has none)"""
    _fields_ = [("cbar", C.c_double), ("mu_factor", C.c_double), ("inner_iters", C.c_int32), ("final_iters", C.c_int32),
                ("max_rounds", C.c_int32), ("_pad", C.c_int32), ("select", C.POINTER(C.c_uint8))]

    def __init__(self, cbar, **kw):
        super().__init__()
        lib().pgo_gnc_options_default(C.byref(self))
        self.cbar = float(cbar)
        for k, v in kw.items():
            if k not in ("mu_factor", "inner_iters", "final_iters", "max_rounds"):
                raise TypeError("unknown gnc option " + k)
            setattr(self, k, v)


class GncRound(C.Structure):
    _fields_ = [("mu", C.c_double), ("weighted_cost", C.c_double), ("n_nonbinary", C.c_int32), ("n_zero", C.c_int32),
                ("lm_iterations", C.c_int32), ("lm_termination", C.c_int32), ("seconds", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class GncSummary(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("hit_max_rounds", C.c_int32), ("n_selected", C.c_int32), ("n_zero", C.c_int32),
                ("rmax2", C.c_double), ("mu0", C.c_double), ("mu_last", C.c_double), ("seconds_total", C.c_double),
                ("final_solve", Summary)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "final_solve"}
        d["final_solve"] = self.final_solve.as_dict()
        return d


class MixStats(C.Structure):
    """mirror of pgo_mix_stats: what Solver.mixture_select measured over the mixture edges"""
    _fields_ = [("n_mix", C.c_int32), ("n_changed", C.c_int32), ("n_nonfinite", C.c_int32), ("n_inactive", C.c_int32),
                ("offset", C.c_double), ("mix_cost", C.c_double), ("count", C.c_int32 * 8)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "count"}
        d["count"] = list(self.count)
        return d


class MixtureOptions(C.Structure):
    """mirror of pgo_mixture_options (defaults: pgo_mixture_options_default)"""
    _fields_ = [("inner_iters", C.c_int32), ("final_iters", C.c_int32), ("max_rounds", C.c_int32), ("_pad", C.c_int32)]

    def __init__(self, **kw):
        super().__init__()
        lib().pgo_mixture_options_default(C.byref(self))
        for k, v in kw.items():
            if k not in ("inner_iters", "final_iters", "max_rounds"):
                raise TypeError("unknown mixture option " + k)
            setattr(self, k, v)


class MixtureRound(C.Structure):
    _fields_ = [("objective", C.c_double), ("n_changed", C.c_int32), ("lm_iterations", C.c_int32), ("lm_termination", C.c_int32),
                ("_pad", C.c_int32), ("count", C.c_int32 * 8), ("seconds", C.c_double)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n not in ("count", "_pad")}
        d["count"] = list(self.count)
        return d


class MixtureSummary(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("hit_max_rounds", C.c_int32), ("n_mix", C.c_int32), ("n_would_change", C.c_int32),
                ("objective", C.c_double), ("offset", C.c_double), ("seconds_total", C.c_double), ("final_solve", Summary)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if n != "final_solve"}
        d["final_solve"] = self.final_solve.as_dict()
        return d


class LoopSupportOptions(C.Structure):
    """mirror of pgo_loop_support_options (defaults: pgo_loop_support_options_default)"""
    _fields_ = [("window", C.c_int32), ("min_support", C.c_int32), ("apply", C.c_int32), ("_pad", C.c_int32),
                ("tol_xy", C.c_double), ("tol_th", C.c_double)]

    def __init__(self, **kw):
        super().__init__()
        lib().pgo_loop_support_options_default(C.byref(self))
        for k, v in kw.items():
            if k not in ("window", "min_support", "apply", "tol_xy", "tol_th"):
                raise TypeError("unknown loop support option " + k)
            setattr(self, k, v)


class LoopSupportRecord(C.Structure):
    """mirror of pgo_loop_support: one edge of loop_support_plan / Solver.loop_support"""
    _fields_ = [("selected", C.c_int32), ("n_pairs", C.c_int32), ("n_consistent", C.c_int32), ("best", C.c_int32),
                ("q_min", C.c_double)]


class LoopSupportStats(C.Structure):
    _fields_ = [("n_pairs_total", C.c_int64), ("n_selected", C.c_int32), ("n_supported", C.c_int32), ("max_pairs", C.c_int32),
                ("_pad", C.c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "_pad"}


_CHORDAL_OPTS = ("rtol", "mag_min", "reject_xy", "reject_th", "max_iters", "check_every", "rounds", "commit", "apply_weights")


class ChordalOptions(C.Structure):
    """mirror of pgo_chordal_options (defaults: pgo_chordal_options_default)"""
    _fields_ = [("rtol", C.c_double), ("mag_min", C.c_double), ("reject_xy", C.c_double), ("reject_th", C.c_double),
                ("max_iters", C.c_int32), ("check_every", C.c_int32), ("rounds", C.c_int32), ("commit", C.c_int32),
                ("apply_weights", C.c_int32), ("_pad", C.c_int32)]

    def __init__(self, **kw):
        super().__init__()
        lib().pgo_chordal_options_default(C.byref(self))
        for k, v in kw.items():
            if k not in _CHORDAL_OPTS:
                raise TypeError("unknown chordal option " + k)
            setattr(self, k, int(v) if k in _CHORDAL_OPTS[4:] else float(v))


class ChordalSolve(C.Structure):
    """mirror of pgo_chordal_solve: one solve of both stages ([0] rotations, [1] positions)"""
    _fields_ = [("iters", C.c_int32 * 2), ("converged", C.c_int32 * 2), ("rel_residual", C.c_double * 2), ("min_mag", C.c_double),
                ("n_degenerate", C.c_int32), ("n_rejected", C.c_int32)]

    def as_dict(self):
        return {"iters": list(self.iters), "converged": list(self.converged), "rel_residual": list(self.rel_residual),
                "min_mag": self.min_mag, "n_degenerate": self.n_degenerate, "n_rejected": self.n_rejected}


class ChordalSummary(C.Structure):
    _fields_ = [("n_solves", C.c_int32), ("n_rejected", C.c_int32), ("n_degenerate", C.c_int32), ("_pad", C.c_int32),
                ("min_mag", C.c_double), ("seconds", C.c_double), ("solve", ChordalSolve * (8 + 1))]

    def as_dict(self):
        return {"n_solves": self.n_solves, "n_rejected": self.n_rejected, "n_degenerate": self.n_degenerate, "min_mag": self.min_mag,
                "seconds": self.seconds, "solves": [self.solve[k].as_dict() for k in range(self.n_solves)]}


_LIB = None


def build(force: bool = False, verbose: bool = False) -> str:
    return _build.build_lib(force=force, verbose=verbose)


def lib():
    """Load libpgo.so (building it first if the sources are newer).  Fails loudly."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = _build.LIB
    if _build.needs_build():
        try:
            path = _build.build_lib()
        except RuntimeError as e:  # no hipcc on this box: a present library is still usable, but say that it is stale
            if not os.path.exists(path):
                raise ImportError(f"libpgo.so is missing and could not be built: {e}") from e
            import warnings
            warnings.warn(f"{path} is OLDER than its sources and hipcc is not available to rebuild it ({e}); "
                          "running the stale library", RuntimeWarning)
        # a compile error (CalledProcessError) propagates: never fall back to a stale binary after a failed build
    L = C.CDLL(path)
    vp, dp, ip, bp = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    L.pgo_strerror.restype = C.c_char_p
    L.pgo_strerror.argtypes = [C.c_int]
    L.pgo_last_error.restype = C.c_char_p
    L.pgo_version.restype = C.c_char_p
    L.pgo_g2o_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.pgo_g2o_parse.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(vp)]
    L.pgo_graph_from_arrays.argtypes = [C.c_int32, dp, C.c_int32, ip, ip, dp, dp, bp, C.POINTER(vp)]
    L.pgo_graph_free.argtypes = [vp]
    L.pgo_graph_free.restype = None
    for f in ("pgo_graph_num_poses", "pgo_graph_num_edges"):
        getattr(L, f).argtypes = [vp]
        getattr(L, f).restype = C.c_int32
    L.pgo_graph_num_edges_of_kind.argtypes = [vp, C.c_int]
    L.pgo_graph_num_edges_of_kind.restype = C.c_int32
    for f, rt in (("pgo_graph_pose_ids", ip), ("pgo_graph_poses", dp), ("pgo_graph_edge_a", ip),
                  ("pgo_graph_edge_b", ip), ("pgo_graph_edge_meas", dp), ("pgo_graph_edge_info", dp),
                  ("pgo_graph_edge_kind", bp)):
        getattr(L, f).argtypes = [vp]
        getattr(L, f).restype = rt
    L.pgo_inject_outliers.argtypes = [vp, C.c_int32, C.c_int64]
    L.pgo_write_nodes.argtypes = [vp, C.c_char_p, C.c_int]
    L.pgo_write_edges.argtypes = [vp, C.c_char_p]
    L.pgo_write_g2o.argtypes = [vp, C.c_char_p]
    L.pgo_synth_manhattan.argtypes = [C.c_int32, C.c_double, C.c_double, C.c_uint64, C.POINTER(vp)]
    L.pgo_options_default.argtypes = [C.POINTER(Options)]
    L.pgo_options_default.restype = None
    L.pgo_comm_unique_id.argtypes = [bp]
    L.pgo_comm_create_rccl.argtypes = [bp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.pgo_comm_create_shm.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.pgo_comm_destroy.argtypes = [vp]
    L.pgo_comm_destroy.restype = None
    L.pgo_create.argtypes = [C.POINTER(vp), C.c_int32, dp, C.c_int32, ip, ip, dp, bp, C.POINTER(Options), vp, C.c_int]
    L.pgo_create_weighted.argtypes = [C.POINTER(vp), C.c_int32, dp, C.c_int32, ip, ip, dp, dp, bp, C.POINTER(Options), vp, C.c_int]
    L.pgo_create_from_graph.argtypes = [C.POINTER(vp), vp, C.POINTER(Options), vp, C.c_int]
    L.pgo_edge_chi2.argtypes = [vp, dp, dp]
    L.pgo_solve_batch.argtypes = [C.POINTER(vp), C.c_int32, C.POINTER(Summary), C.c_int32]
    L.pgo_destroy.argtypes = [vp]
    L.pgo_destroy.restype = None
    L.pgo_batch_create.argtypes = [C.POINTER(vp), C.c_int32, C.POINTER(vp), C.POINTER(Options), C.c_int]
    L.pgo_batch_destroy.argtypes = [vp]
    L.pgo_batch_destroy.restype = None
    L.pgo_batch_size.argtypes = [vp]
    L.pgo_batch_size.restype = C.c_int32
    L.pgo_batch_solve.argtypes = [vp, C.POINTER(Summary)]
    L.pgo_batch_get_poses.argtypes = [vp, C.c_int32, dp]
    L.pgo_batch_set_poses.argtypes = [vp, C.c_int32, dp]
    L.pgo_batch_num_iter_records.argtypes = [vp, C.c_int32]
    L.pgo_batch_num_iter_records.restype = C.c_int32
    L.pgo_batch_get_iter_records.argtypes = [vp, C.c_int32, C.POINTER(IterRecord), C.c_int32]
    L.pgo_eval.argtypes = [vp, dp, C.c_int, dp, dp, dp]
    L.pgo_solve.argtypes = [vp, C.POINTER(Summary)]
    L.pgo_lm_begin.argtypes = [vp]
    L.pgo_lm_step.argtypes = [vp, C.c_int32, ip, C.POINTER(Summary)]
    L.pgo_num_iter_records.argtypes = [vp]
    L.pgo_num_iter_records.restype = C.c_int32
    L.pgo_get_iter_records.argtypes = [vp, C.POINTER(IterRecord), C.c_int32]
    L.pgo_get_info.argtypes = [vp, C.POINTER(HandleInfo)]
    L.pgo_get_poses.argtypes = [vp, dp]
    L.pgo_set_poses.argtypes = [vp, dp]
    L.pgo_get_switches.argtypes = [vp, dp, dp]
    L.pgo_write_switches.argtypes = [vp, C.c_char_p, dp]
    L.pgo_bench_eval.argtypes = [vp, C.c_int, C.c_int, C.POINTER(KernelStats)]
    L.pgo_bench_assemble.argtypes = [vp, C.c_int, C.POINTER(KernelStats)]
    L.pgo_bench_spmv.argtypes = [vp, C.c_int, C.POINTER(KernelStats)]
    L.pgo_bench_precond.argtypes = [vp, C.c_int, C.POINTER(KernelStats)]
    L.pgo_debug_precond.argtypes = [vp, dp, dp]
    L.pgo_debug_spmv.argtypes = [vp, dp, dp]
    L.pgo_debug_system_spmv.argtypes = [vp, dp, dp, dp]
    L.pgo_debug_direct_solve.argtypes = [vp, dp, C.c_int32, dp]
    L.pgo_debug_normal_eq.argtypes = [vp, dp, dp]
    L.pgo_batch_debug_solve.argtypes = [vp, C.c_double, C.c_int32, C.c_double, dp, dp, C.POINTER(SoloResult)]
    L.pgo_shard_plan.argtypes = [C.c_int32, C.c_int32, ip, ip, C.c_int, C.c_int, C.c_int, ip, ip, ip, ip]
    L.pgo_shard_halo.argtypes = [C.c_int32, C.c_int32, ip, ip, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64),
                                 C.POINTER(C.c_int64)]
    L.pgo_pose_order.argtypes = [C.c_int32, C.c_int32, ip, ip, C.c_int32, ip]
    L.pgo_debug_set_knob.argtypes = [C.c_char_p, C.c_longlong]
    L.pgo_covariance_options_default.argtypes = [C.POINTER(CovarianceOptions)]
    L.pgo_covariance_options_default.restype = None
    L.pgo_pose_covariance.argtypes = [vp, C.c_int32, ip, C.POINTER(CovarianceOptions), dp, C.POINTER(CovarianceReport)]
    L.pgo_sample_options_default.argtypes = [C.POINTER(SampleOptions)]
    L.pgo_sample_options_default.restype = None
    L.pgo_sample_noise_eval.argtypes = [C.c_uint64, C.c_int32, C.c_int64, C.c_int32, dp]
    L.pgo_posterior_sample.argtypes = [vp, C.c_int32, C.POINTER(SampleOptions), dp, dp, C.POINTER(CovarianceReport)]
    L.pgo_debug_sample_rhs.argtypes = [vp, C.c_uint64, C.c_int32, dp, dp]
    L.pgo_loss_evaluate.argtypes = [C.POINTER(Loss), C.c_double, dp]
    L.pgo_set_losses.argtypes = [vp, C.c_int32, C.POINTER(Loss), bp]
    L.pgo_batch_set_losses.argtypes = [vp, C.c_int32, C.POINTER(Loss), bp]
    L.pgo_set_active.argtypes = [vp, bp, bp]
    L.pgo_batch_set_active.argtypes = [vp, bp, bp]
    L.pgo_active_plan.argtypes = [C.c_int32, C.c_int32, ip, ip, bp, bp, C.c_int32, bp, ip, ip]
    L.pgo_gate_evaluate.argtypes = [dp, dp, dp, dp]
    L.pgo_edge_gate.argtypes = [vp, C.c_int32, ip, ip, dp, dp, C.POINTER(CovarianceOptions), C.POINTER(EdgeGateResult),
                                C.POINTER(CovarianceReport)]
    L.pgo_gate_joint_options_default.argtypes = [C.POINTER(GateJointOptions)]
    L.pgo_gate_joint_options_default.restype = None
    L.pgo_gate_joint_evaluate.argtypes = [C.c_int32, dp, dp, dp, ip, C.POINTER(C.c_int8), C.POINTER(GateJointOptions),
                                          C.POINTER(GateJointResult), C.POINTER(GateJointSummary)]
    L.pgo_edge_gate_joint.argtypes = [vp, C.c_int32, ip, ip, dp, dp, C.POINTER(C.c_int8), C.POINTER(GateJointOptions),
                                      C.POINTER(CovarianceOptions), C.POINTER(EdgeGateResult), C.POINTER(GateJointResult), dp,
                                      C.POINTER(GateJointSummary), C.POINTER(CovarianceReport)]
    L.pgo_window_plan.argtypes = [C.c_int32, C.c_int32, ip, ip, bp, C.c_int32, ip, C.c_int32, C.c_int32, ip, ip, C.c_int32, ip, ip, ip]
    L.pgo_window_solve.argtypes = [vp, C.c_int32, ip, ip, ip, ip, ip, C.c_int32, C.c_int32, dp, C.POINTER(WindowResult),
                                   C.POINTER(IterRecord)]
    L.pgo_batch_window_solve.argtypes = [vp, C.c_int32, ip, ip, ip, ip, ip, ip, C.c_int32, C.c_int32, dp, C.POINTER(WindowResult),
                                         C.POINTER(IterRecord)]
    L.pgo_synth_manhattan_truth.argtypes = [C.c_int32, C.c_uint64, dp]
    L.pgo_traj_options_default.argtypes = [C.POINTER(TrajOptions)]
    L.pgo_traj_options_default.restype = None
    L.pgo_trajectory_error_eval.argtypes = [C.c_int32, dp, dp, bp, C.POINTER(TrajOptions), C.POINTER(TrajError), dp]
    L.pgo_trajectory_error.argtypes = [vp, dp, bp, C.POINTER(TrajOptions), C.POINTER(TrajError), dp]
    L.pgo_edge_weights.argtypes = [vp, dp, C.POINTER(EdgeWeight)]
    L.pgo_coarsen_plan.argtypes = [C.c_int32, C.c_int32, ip, ip, dp, bp, C.c_int32, ip, C.c_int32, ip, ip, dp, bp, ip, ip, dp, dp]
    L.pgo_prolong_eval.argtypes = [C.c_int32, C.c_int32, dp, dp, dp, dp]
    L.pgo_coarsen_info_plan.argtypes = [C.c_int32, C.c_int32, ip, ip, dp, bp, dp, C.c_int32, ip, C.c_int32, ip, ip, dp, bp, ip, dp, dp, ip,
                                        dp, dp, dp, dp]
    L.pgo_coarsen_info.argtypes = [vp, C.c_int32, C.POINTER(vp), ip, dp, C.c_int32, ip]
    L.pgo_coarsen.argtypes = [vp, C.c_int32, C.POINTER(vp), ip, C.c_int32, ip]
    L.pgo_prolong.argtypes = [vp, C.c_int32, dp]
    L.pgo_set_edge_weights.argtypes = [vp, dp]
    L.pgo_get_edge_weights.argtypes = [vp, dp]
    L.pgo_gnc_options_default.argtypes = [C.POINTER(GncOptions)]
    L.pgo_gnc_options_default.restype = None
    L.pgo_gnc_weight_eval.argtypes = [C.c_double, C.c_double, C.c_int32, dp, dp]
    L.pgo_gnc_update.argtypes = [vp, C.c_double, C.c_double, bp, C.POINTER(GncStats)]
    L.pgo_gnc_solve.argtypes = [vp, C.POINTER(GncOptions), C.POINTER(GncSummary), C.POINTER(GncRound), C.c_int32]
    L.pgo_loop_support_options_default.argtypes = [C.POINTER(LoopSupportOptions)]
    L.pgo_loop_support_options_default.restype = None
    L.pgo_loop_support_plan.argtypes = [C.c_int32, C.c_int32, ip, ip, dp, bp, bp, C.POINTER(LoopSupportOptions), C.POINTER(LoopSupportRecord),
                                        C.POINTER(LoopSupportStats), dp]
    L.pgo_loop_support.argtypes = [vp, C.POINTER(LoopSupportOptions), bp, C.POINTER(LoopSupportRecord), C.POINTER(LoopSupportStats)]
    L.pgo_chordal_options_default.argtypes = [C.POINTER(ChordalOptions)]
    L.pgo_chordal_options_default.restype = None
    L.pgo_chordal_plan.argtypes = [C.c_int32, C.c_int32, ip, ip, dp, dp, bp, dp, C.POINTER(ChordalOptions), dp, dp, dp, C.POINTER(ChordalSummary)]
    L.pgo_chordal_init.argtypes = [vp, C.POINTER(ChordalOptions), dp, dp, C.POINTER(ChordalSummary)]
    L.pgo_mixture_options_default.argtypes = [C.POINTER(MixtureOptions)]
    L.pgo_mixture_options_default.restype = None
    L.pgo_mixture_eval.argtypes = [C.c_int32, dp, dp, C.POINTER(Loss), ip, dp, dp]
    L.pgo_mixture_plan.argtypes = [C.c_int32, dp, C.c_int32, ip, ip, C.c_int32, ip, ip, dp, C.c_int32, C.POINTER(Loss), bp, ip, bp, ip, dp,
                                   C.POINTER(MixStats)]
    L.pgo_set_mixtures.argtypes = [vp, C.c_int32, ip, ip, dp]
    L.pgo_set_mixture_null.argtypes = [vp, bp, C.c_double, C.c_double]
    L.pgo_mixture_select.argtypes = [vp, C.c_int32, C.POINTER(MixStats), ip, dp]
    L.pgo_get_mixture_selection.argtypes = [vp, ip]
    L.pgo_mixture_solve.argtypes = [vp, C.POINTER(MixtureOptions), C.POINTER(MixtureSummary), C.POINTER(MixtureRound), C.c_int32]
    L.pgo_set_priors.argtypes = [vp, C.c_int32, ip, dp, dp, C.POINTER(Loss)]
    L.pgo_num_priors.argtypes = [vp]
    L.pgo_num_priors.restype = C.c_int32
    L.pgo_get_prior_residuals.argtypes = [vp, dp, dp, dp]
    L.pgo_prior_eval.argtypes = [dp, dp, dp, C.POINTER(Loss), dp, dp, dp]
    _LIB = L
    return L


def _check(status: int):
    if status != 0:
        L = lib()
        detail = (L.pgo_last_error() or b"").decode() or (L.pgo_strerror(status) or b"").decode()
        raise PgoError(status, detail)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _bp(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


class _View(np.ndarray):
    """ndarray view into memory owned by a Graph; keeps the Graph alive while the view (or a slice) lives"""
    _owner = None


class Graph:
    """Host-side pose graph (owns a pgo_graph*).  Arrays are exposed as numpy views."""

    def __init__(self, handle):
        self._h = C.c_void_p(handle) if not isinstance(handle, C.c_void_p) else handle

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().pgo_graph_free(self._h)
                self._h = None
        except Exception:
            pass

    # ---- constructors
    @classmethod
    def load(cls, path: str) -> "Graph":
        h = C.c_void_p()
        _check(lib().pgo_g2o_load(os.fsencode(path), C.byref(h)))
        return cls(h)

    @classmethod
    def parse(cls, text) -> "Graph":
        if isinstance(text, str):
            text = text.encode()
        h = C.c_void_p()
        _check(lib().pgo_g2o_parse(text, len(text), C.byref(h)))
        return cls(h)

    @classmethod
    def from_arrays(cls, poses, ia, ib, meas, kind, info=None) -> "Graph":
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
        ia = np.ascontiguousarray(ia, np.int32)
        ib = np.ascontiguousarray(ib, np.int32)
        meas = np.ascontiguousarray(meas, np.float64).reshape(-1, 3)
        kind = np.ascontiguousarray(kind, np.uint8)
        info_a = np.ascontiguousarray(info, np.float64).reshape(-1, 6) if info is not None else None
        h = C.c_void_p()
        _check(lib().pgo_graph_from_arrays(len(poses), _dp(poses), len(ia), _ip(ia), _ip(ib), _dp(meas), _dp(info_a),
                                           _bp(kind), C.byref(h)))
        return cls(h)

    # ---- sizes (reference: cout lines at main.cpp:60-63)
    @property
    def n_poses(self) -> int:
        return lib().pgo_graph_num_poses(self._h)

    @property
    def n_edges(self) -> int:
        return lib().pgo_graph_num_edges(self._h)

    def n_edges_of_kind(self, kind: int) -> int:
        return lib().pgo_graph_num_edges_of_kind(self._h, kind)

    def _view(self, fn, shape, dtype):
        n = int(np.prod(shape))
        if n == 0:
            return np.zeros(shape, dtype)
        ptr = fn(self._h)
        v = np.ctypeslib.as_array(ptr, shape=(n,)).reshape(shape).view(_View)
        v._owner = self
        return v

    @property
    def pose_ids(self):
        return self._view(lib().pgo_graph_pose_ids, (self.n_poses,), np.int32)

    @property
    def poses(self):  # mutable view: Node::p
        return self._view(lib().pgo_graph_poses, (self.n_poses, 3), np.float64)

    @property
    def ia(self):
        return self._view(lib().pgo_graph_edge_a, (self.n_edges,), np.int32)

    @property
    def ib(self):
        return self._view(lib().pgo_graph_edge_b, (self.n_edges,), np.int32)

    @property
    def meas(self):
        return self._view(lib().pgo_graph_edge_meas, (self.n_edges, 3), np.float64)

    @property
    def info(self):
        return self._view(lib().pgo_graph_edge_info, (self.n_edges, 6), np.float64)

    @property
    def kind(self):
        return self._view(lib().pgo_graph_edge_kind, (self.n_edges,), np.uint8)

    # ---- reference-named operations
    def add_random_C(self, count: int, seed: int = -1):
        _check(lib().pgo_inject_outliers(self._h, count, seed))

    def writePoseGraph_nodes(self, path: str, precision: int = 0):
        _check(lib().pgo_write_nodes(self._h, os.fsencode(path), precision))

    def writePoseGraph_edges(self, path: str):
        _check(lib().pgo_write_edges(self._h, os.fsencode(path)))

    def writePoseGraph_switches(self, path: str, switches):
        sw = np.ascontiguousarray(switches, np.float64)
        _check(lib().pgo_write_switches(self._h, os.fsencode(path), _dp(sw)))

    def write_g2o(self, path: str):
        _check(lib().pgo_write_g2o(self._h, os.fsencode(path)))


def ReadG2O(path: str) -> Graph:
    """ReadG2O g2o_manager(path) -- reference main.cpp:49"""
    return Graph.load(path)


def synth_manhattan(n_poses: int, edges_per_pose: float = 4.0, outlier_frac: float = 0.10,
                    seed: int = 20260410) -> Graph:
    h = C.c_void_p()
    _check(lib().pgo_synth_manhattan(n_poses, edges_per_pose, outlier_frac, seed, C.byref(h)))
    return Graph(h)


def synth_manhattan_truth(n_poses: int, seed: int = 20260410):
    """pgo_synth_manhattan_truth (host only): the (n, 3) ground-truth poses of synth_manhattan(n_poses, *, *, seed), in the frame
    of pose 0 -- comparable with the graph's dead-reckoned poses and with any solve that keeps pose 0 constant"""
    out = np.zeros((max(int(n_poses), 0), 3))
    _check(lib().pgo_synth_manhattan_truth(n_poses, seed, _dp(out)))
    return out


def _traj_call(fn, head, n, ref, mask, align, rpe_delta, per_pose):
    ref = np.ascontiguousarray(ref, np.float64).reshape(-1, 3)
    if len(ref) != n:
        raise ValueError(f"trajectory_error: the reference has {len(ref)} poses, the estimate {n}")
    m = _mask(mask, n, "mask")
    o = TrajOptions(align=int(align), rpe_delta=int(rpe_delta))
    out = TrajError()
    pp = np.zeros((n, 2)) if per_pose else None
    _check(fn(*head, _dp(ref), _bp(m) if m is not None else None, C.byref(o), C.byref(out), _dp(pp)))
    return (out.as_dict(), pp) if per_pose else out.as_dict()


def trajectory_error(est, ref, mask=None, align=False, rpe_delta=1, per_pose=False):
    """pgo_trajectory_error_eval (host only): ATE / RPE of the (n, 3) estimate against the reference over the poses whose
    mask entry is truthy (None: all).  align=True fits the estimate onto the reference first (rigid, no scale); RPE runs over
    the pairs (i, i + rpe_delta), 0 = none.  Returns the dict of TrajError (and the (n, 2) per-pose array (trans, |rot|) with
    per_pose=True)."""
    est = np.ascontiguousarray(est, np.float64).reshape(-1, 3)
    return _traj_call(lib().pgo_trajectory_error_eval, (len(est), _dp(est)), len(est), ref, mask, align, rpe_delta, per_pose)


def gnc_weight_eval(cbar, mu, s):
    """pgo_gnc_weight_eval (host only): the GNC-TLS weights gnc_tls_weight(cbar^2, mu, s) of csrc/gnc.h for an array of plain
    squared residuals s; a non-finite s gives 0"""
    s = np.ascontiguousarray(s, np.float64)
    out = np.zeros(s.shape)
    _check(lib().pgo_gnc_weight_eval(float(cbar), float(mu), s.size, _dp(s.reshape(-1)), _dp(out.reshape(-1))))
    return out


def _mix_table(edge, comp_ptr, comps):
    """a mixture table as the C-ABI takes it: edge [n] and comp_ptr [n + 1] as int32, comps as an (n_comp, 5) array of
    (x, y, theta, weight, info_scale) rows (pgo_mix_component)"""
    edge = np.ascontiguousarray(edge, np.int32).reshape(-1)
    comp_ptr = np.ascontiguousarray(comp_ptr, np.int32).reshape(-1)
    comps = np.ascontiguousarray(comps, np.float64).reshape(-1, 5)
    if comp_ptr.size != edge.size + 1 or (edge.size and int(comp_ptr.max()) > len(comps)):
        raise ValueError("mixtures: comp_ptr must have one entry per mixture edge plus one, within comps")
    return edge, comp_ptr, comps


def mixture_eval(comps, s, loss=None):
    """pgo_mixture_eval (host only): the max-mixture statement of csrc/mixture.h on one edge -- comps an (K, 5) array of
    (x, y, theta, weight, info_scale) rows, s the K plain squared residuals, loss a Loss (None: Trivial).  Returns (chosen,
    q_best, margin); chosen = -1 and NaN when no component is finite."""
    comps = np.ascontiguousarray(comps, np.float64).reshape(-1, 5)
    s = np.ascontiguousarray(s, np.float64).reshape(-1)
    if s.size != len(comps):
        raise ValueError("mixture_eval: one s per component")
    k, qb, mg = np.zeros(1, np.int32), np.zeros(1), np.zeros(1)
    _check(lib().pgo_mixture_eval(len(comps), _dp(comps), _dp(s), C.byref(loss) if loss is not None else None, _ip(k), _dp(qb), _dp(mg)))
    return int(k[0]), float(qb[0]), float(mg[0])


def prior_eval(pose, mean, info, loss=None):
    """pgo_prior_eval (host only): the pose prior of csrc/prior.h at one pose -- pose and mean (x, y, theta), info the six values
    I11 I12 I13 I22 I23 I33 or a symmetric 3x3 matrix, loss a Loss (None: Trivial).  Returns (d, chi2, rho): the plain residual
    with the heading wrapped to [-pi, pi], d' info d, and rho, rho', rho'' of the loss at chi2."""
    pose = np.ascontiguousarray(pose, np.float64).reshape(3)
    mean = np.ascontiguousarray(mean, np.float64).reshape(3)
    info = _info6(info, 1).reshape(6)
    d, chi2, rho = np.zeros(3), np.zeros(1), np.zeros(3)
    _check(lib().pgo_prior_eval(_dp(pose), _dp(mean), _dp(info), C.byref(loss) if loss is not None else None, _dp(d), _dp(chi2), _dp(rho)))
    return d, float(chi2[0]), rho


def _info6(info, n):
    """(n, 6) information rows I11 I12 I13 I22 I23 I33 from (n, 6), or from (n, 3, 3) symmetric matrices (the upper triangle is read)"""
    a = np.asarray(info, np.float64)
    if a.size == 9 * n and a.shape[-2:] == (3, 3):
        a = a.reshape(n, 3, 3)[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]
    if a.size != 6 * n:
        raise ValueError(f"info: {n} rows of six values (I11 I12 I13 I22 I23 I33) or {n} 3x3 matrices")
    return np.ascontiguousarray(a.reshape(n, 6))


def mixture_plan(poses, ia, ib, edge, comp_ptr, comps, losses=None, mix_class=None, prev=None, active=None):
    """pgo_mixture_plan (host only), the serial statement of Solver.mixture_select: poses (N, 3), the edges' endpoints, the
    mixture table (edge, comp_ptr, comps as Solver.set_mixtures takes it), the loss classes (a Loss or a list; None: Trivial)
    with each MIXTURE edge's class (None: 0), the previous applied selection (None: none) and a mask over the mixture edges
    (None: all active).  Returns (chosen, q (n_mix, 2), stats dict)."""
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
    ia = np.ascontiguousarray(ia, np.int32)
    ib = np.ascontiguousarray(ib, np.int32)
    edge, comp_ptr, comps = _mix_table(edge, comp_ptr, comps)
    n = edge.size
    nl, larr = 1, None
    if losses is not None:
        nl, larr, _, _ = _loss_args(losses, None, 0)
    cls = np.ascontiguousarray(mix_class, np.uint8).reshape(-1) if mix_class is not None else None
    pv = np.ascontiguousarray(prev, np.int32).reshape(-1) if prev is not None else None
    act = _mask(active, n, "active")
    if any(a is not None and a.size != n for a in (cls, pv)):
        raise ValueError("mixture_plan: mix_class and prev have one entry per mixture edge")
    chosen, q, st = np.zeros(max(n, 1), np.int32), np.zeros((max(n, 1), 2)), MixStats()
    _check(lib().pgo_mixture_plan(len(poses), _dp(poses), len(ia), _ip(ia), _ip(ib), n, _ip(edge), _ip(comp_ptr), _dp(comps), nl, larr,
                                  _bp(cls) if cls is not None else None, _ip(pv) if pv is not None else None,
                                  _bp(act) if act is not None else None, _ip(chosen), _dp(q), C.byref(st)))
    return chosen[:n], q[:n], st.as_dict()


def _support_records(res, n):
    return np.ctypeslib.as_array(res)[:n].copy() if n else np.zeros(0, np.dtype(LoopSupportRecord))


def loop_support_plan(n_poses, ia, ib, meas, kind, select=None, window=32, tol_xy=0.1, tol_th=0.05, min_support=1, want_T=False):
    """pgo_loop_support_plan (host only), the serial statement of Solver.loop_support: every selected loop (default: the edges
    with kind != 0 that are not chain edges; else a mask over the edges) against its neighbours along the odometry chain --
    the selected loops whose ends lie within `window` poses of its own -- through the 4-cycle the two close with the odometry.
    Returns (records, stats): a structured array over the edges with the fields of LoopSupportRecord (selected, n_pairs,
    n_consistent, best, q_min) and the dict of LoopSupportStats; with want_T also the (n_poses, 3) odometry trajectory.
    The default tolerances fit synth_manhattan's odometry noise: a real dataset needs its own."""
    ia = np.ascontiguousarray(ia, np.int32)
    ib = np.ascontiguousarray(ib, np.int32)
    meas = np.ascontiguousarray(meas, np.float64).reshape(-1, 3)
    kind = np.ascontiguousarray(kind, np.uint8)
    if not (len(ia) == len(ib) == len(kind) == len(meas)):
        raise ValueError("loop_support_plan: ia, ib, meas and kind must have one entry per edge")
    m = _mask(select, len(ia), "select")
    o = LoopSupportOptions(window=int(window), tol_xy=float(tol_xy), tol_th=float(tol_th), min_support=int(min_support))
    res = (LoopSupportRecord * max(len(ia), 1))()
    st = LoopSupportStats()
    T = np.zeros((max(int(n_poses), 1), 3)) if want_T else None
    _check(lib().pgo_loop_support_plan(n_poses, len(ia), _ip(ia), _ip(ib), _dp(meas), _bp(kind), _bp(m) if m is not None else None,
                                       C.byref(o), res, C.byref(st), _dp(T)))
    rec = _support_records(res, len(ia))
    return (rec, st.as_dict(), T[:int(n_poses)]) if want_T else (rec, st.as_dict())


def chordal_plan(n_poses, ia, ib, meas, poses, w=None, constant=None, **opts):
    """pgo_chordal_plan (host only), the serial statement of Solver.chordal_init: chordal rotations, then positions given the
    rotations, each a Hermitian system solved by Jacobi-PCG from the odometry trajectory; no estimate plays a part except on
    the constant poses (constant: a mask over the poses, default pose 0), which keep their values in `poses`.  w: a weight in
    [0, 1] per edge (default 1; 0 = the edge is not there).  opts: the fields of ChordalOptions (rtol, max_iters, check_every,
    mag_min, rounds, reject_xy, reject_th).  Returns (poses (N, 3), res (E, 2): |position residual|, |heading residual| per
    edge, w_out (E): w with 0 on the edges the rounds rejected, summary dict)."""
    ia = np.ascontiguousarray(ia, np.int32)
    ib = np.ascontiguousarray(ib, np.int32)
    meas = np.ascontiguousarray(meas, np.float64).reshape(-1, 3)
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
    n, E = int(n_poses), len(ia)
    if not (len(ib) == len(meas) == E) or len(poses) != n:
        raise ValueError("chordal_plan: ia, ib and meas must have one entry per edge, poses one row per pose")
    if w is not None:
        w = np.ascontiguousarray(w, np.float64).reshape(-1)
        if len(w) != E:
            raise ValueError("chordal_plan: w must have one entry per edge")
    m = _mask(constant, n, "constant")
    o = ChordalOptions(**opts)
    out, res, w_out = np.zeros((max(n, 1), 3)), np.zeros((max(E, 1), 2)), np.zeros(max(E, 1))
    summ = ChordalSummary()
    _check(lib().pgo_chordal_plan(n, E, _ip(ia), _ip(ib), _dp(meas), _dp(w) if w is not None else None, _bp(m) if m is not None else None,
                                  _dp(poses), C.byref(o), _dp(out), _dp(res), _dp(w_out), C.byref(summ)))
    return out[:n], res[:E], w_out[:E], summ.as_dict()


def shard_plan(n_poses, ia, ib, world, rank, row_align=1):
    ia = np.ascontiguousarray(ia, np.int32)
    ib = np.ascontiguousarray(ib, np.int32)
    lo, hi, nl, nc = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    _check(lib().pgo_shard_plan(n_poses, len(ia), _ip(ia), _ip(ib), world, rank, row_align, C.byref(lo), C.byref(hi),
                                C.byref(nl), C.byref(nc)))
    return lo.value, hi.value, nl.value, nc.value


def _mask(a, n, what):
    """a byte mask of n entries (any array-like of truth values), or None"""
    if a is None:
        return None
    m = np.ascontiguousarray(np.asarray(a).reshape(-1) != 0, np.uint8)
    if m.size != n:
        raise ValueError(f"{what}: {m.size} entries, expected {n}")
    return m


def active_plan(n_poses, ia, ib, edge_active=None, pose_constant=None, fixed_pose=0):
    """pgo_active_plan (host only): what Solver.set_active / Batch.set_active resolve their masks to.
    Returns (constant[n_poses] uint8, n_active_edges, n_free_poses)."""
    ia = np.ascontiguousarray(ia, np.int32)
    ib = np.ascontiguousarray(ib, np.int32)
    ea = _mask(edge_active, len(ia), "edge_active")
    pc = _mask(pose_constant, n_poses, "pose_constant")
    const = np.zeros(max(n_poses, 0), np.uint8)
    na, nf = C.c_int32(), C.c_int32()
    _check(lib().pgo_active_plan(n_poses, len(ia), _ip(ia), _ip(ib), _bp(ea) if ea is not None else None,
                                 _bp(pc) if pc is not None else None, fixed_pose, _bp(const), C.byref(na), C.byref(nf)))
    return const, na.value, nf.value


def window_plan(n_poses, ia, ib, kind, focus_edges, radius, pose_cap=None, edge_cap=None):
    """pgo_window_plan (host only), the layer managers' window rule: the poses within `radius` of an end of a focus edge, the
    odometry edges among them, then the focus edges.  Returns (pose_idx, edge_idx, anchor) -- one window of
    Solver.window_solve.  pose_cap / edge_cap (default: no limit): a window above a cap raises PgoError, whose n_poses /
    n_edges attributes carry the counts."""
    ia = np.ascontiguousarray(ia, np.int32)
    ib = np.ascontiguousarray(ib, np.int32)
    kind = np.ascontiguousarray(kind, np.uint8)
    if not (len(ia) == len(ib) == len(kind)):
        raise ValueError("window_plan: ia, ib and kind must have one entry per edge")
    fe = np.ascontiguousarray(np.asarray(focus_edges, np.int64).reshape(-1), np.int32)
    pc = max(int(n_poses), 0) if pose_cap is None else int(pose_cap)
    ec = len(ia) if edge_cap is None else int(edge_cap)
    po, eo = np.zeros(max(pc, 1), np.int32), np.zeros(max(ec, 1), np.int32)
    npo, neo, an = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    st = lib().pgo_window_plan(n_poses, len(ia), _ip(ia), _ip(ib), _bp(kind), len(fe), _ip(fe), int(radius), pc, _ip(po), C.byref(npo),
                               ec, _ip(eo), C.byref(neo), C.byref(an))
    if st != 0:
        try:
            _check(st)
        except PgoError as e:
            e.n_poses, e.n_edges = npo.value, neo.value
            raise
    return po[:npo.value].copy(), eo[:neo.value].copy(), an.value


def coarsen_plan(n_poses, ia, ib, meas, kind, stride, edge_cap=None, want_composites=True):
    """pgo_coarsen_plan (host only), the serial statement of Solver.coarsen: key pose k = fine pose k * stride, the K - 1
    composites of the odometry chain, then every other edge with its ends in two segments carried to the key poses.
    Returns a dict: n_poses (K), ia, ib, meas (n, 3), kind, origin (-1 for a composite, else the fine edge) and, with
    want_composites, C (n_poses, 3) and Cend (K - 1, 3) -- what prolong_eval takes.  edge_cap (default: no limit): a coarse
    graph above it raises PgoError, whose n_poses / n_edges attributes carry the counts."""
    ia = np.ascontiguousarray(ia, np.int32)
    ib = np.ascontiguousarray(ib, np.int32)
    meas = np.ascontiguousarray(meas, np.float64).reshape(-1, 3)
    kind = np.ascontiguousarray(kind, np.uint8)
    if not (len(ia) == len(ib) == len(kind) == len(meas)):
        raise ValueError("coarsen_plan: ia, ib, meas and kind must have one entry per edge")
    cap = len(ia) if edge_cap is None else int(edge_cap)
    m = max(cap, 1)
    cia, cib, cm, ck, co = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros((m, 3)), np.zeros(m, np.uint8), np.zeros(m, np.int32)
    nK, nE = C.c_int32(-1), C.c_int32(-1)
    Cc = np.zeros((max(int(n_poses), 1), 3)) if want_composites else None
    Ce = np.zeros((max(int(n_poses), 1), 3)) if want_composites else None
    st = lib().pgo_coarsen_plan(n_poses, len(ia), _ip(ia), _ip(ib), _dp(meas), _bp(kind), int(stride), C.byref(nK), cap, _ip(cia),
                                _ip(cib), _dp(cm), _bp(ck), _ip(co), C.byref(nE), _dp(Cc), _dp(Ce))
    if st != 0:
        try:
            _check(st)
        except PgoError as e:
            e.n_poses, e.n_edges = nK.value, nE.value
            raise
    n, K = nE.value, nK.value
    out = {"n_poses": K, "ia": cia[:n].copy(), "ib": cib[:n].copy(), "meas": cm[:n].copy(), "kind": ck[:n].copy(),
           "origin": co[:n].copy()}
    if want_composites:
        out["C"], out["Cend"] = Cc[:int(n_poses)], Ce[:K - 1].copy()
    return out


def coarsen_info_plan(n_poses, ia, ib, meas, kind, stride, info=None, edge_cap=None, want_composites=True):
    """pgo_coarsen_info_plan (host only): coarsen_plan with the information matrices carried through the composition.  info
    (E, 6) in the order of info6, or None = unit matrices.  Returns coarsen_plan's dict with "info" and "cov" (n, 6) of the
    coarse edges and, with want_composites, "Ccov" (n_poses, 6) and "Cendcov" (K - 1, 6).  An information matrix of a chain
    edge or a kept edge that is not finite and positive definite raises PgoError (NUMERIC) naming the edge."""
    ia = np.ascontiguousarray(ia, np.int32)
    ib = np.ascontiguousarray(ib, np.int32)
    meas = np.ascontiguousarray(meas, np.float64).reshape(-1, 3)
    kind = np.ascontiguousarray(kind, np.uint8)
    if not (len(ia) == len(ib) == len(kind) == len(meas)):
        raise ValueError("coarsen_info_plan: ia, ib, meas and kind must have one entry per edge")
    if info is not None:
        info = np.ascontiguousarray(info, np.float64).reshape(-1, 6)
        if len(info) != len(ia):
            raise ValueError("coarsen_info_plan: info must be (n_edges, 6)")
    cap = len(ia) if edge_cap is None else int(edge_cap)
    m = max(cap, 1)
    cia, cib, cm, ck, co = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros((m, 3)), np.zeros(m, np.uint8), np.zeros(m, np.int32)
    ci, cc = np.zeros((m, 6)), np.zeros((m, 6))
    nK, nE = C.c_int32(-1), C.c_int32(-1)
    n1 = max(int(n_poses), 1)
    Cc, Ce, Cw, Cew = ((np.zeros((n1, 3)), np.zeros((n1, 3)), np.zeros((n1, 6)), np.zeros((n1, 6))) if want_composites
                       else (None, None, None, None))
    st = lib().pgo_coarsen_info_plan(n_poses, len(ia), _ip(ia), _ip(ib), _dp(meas), _bp(kind), _dp(info), int(stride), C.byref(nK), cap,
                                     _ip(cia), _ip(cib), _dp(cm), _bp(ck), _ip(co), _dp(ci), _dp(cc), C.byref(nE), _dp(Cc), _dp(Ce),
                                     _dp(Cw), _dp(Cew))
    if st != 0:
        try:
            _check(st)
        except PgoError as e:
            e.n_poses, e.n_edges = nK.value, nE.value
            raise
    n, K = nE.value, nK.value
    out = {"n_poses": K, "ia": cia[:n].copy(), "ib": cib[:n].copy(), "meas": cm[:n].copy(), "kind": ck[:n].copy(),
           "origin": co[:n].copy(), "info": ci[:n].copy(), "cov": cc[:n].copy()}
    if want_composites:
        out["C"], out["Cend"], out["Ccov"], out["Cendcov"] = Cc[:int(n_poses)], Ce[:K - 1].copy(), Cw[:int(n_poses)], Cew[:K - 1].copy()
    return out


def prolong_eval(n_poses, stride, C_, Cend, coarse_poses):
    """pgo_prolong_eval (host only): the coarse poses (K, 3) spread over the fine poses with the composites of coarsen_plan;
    key poses come back bitwise"""
    Cc = np.ascontiguousarray(C_, np.float64).reshape(-1, 3)
    Ce = np.ascontiguousarray(Cend, np.float64).reshape(-1, 3)
    X = np.ascontiguousarray(coarse_poses, np.float64).reshape(-1, 3)
    n, s = int(n_poses), int(stride)
    if COARSEN_MIN_STRIDE <= s <= COARSEN_MAX_STRIDE and n > s:   # (sizes the library refuses are left to it)
        K = (n + s - 1) // s
        if len(Cc) != n or len(Ce) != K - 1 or len(X) != K:
            raise ValueError(f"prolong_eval: C must be ({n}, 3), Cend ({K - 1}, 3) and the coarse poses ({K}, 3)")
    out = np.zeros((max(n, 0), 3))
    _check(lib().pgo_prolong_eval(n, s, _dp(Cc), _dp(Ce), _dp(X), _dp(out)))
    return out


def _window_args(windows, with_problem):
    """the CSR arrays of a list of windows, (pose_idx, edge_idx, anchor) or (problem, pose_idx, edge_idx, anchor) each"""
    off = 1 if with_problem else 0
    ps = [np.asarray(w[off], np.int64).reshape(-1) for w in windows]
    es = [np.asarray(w[off + 1], np.int64).reshape(-1) for w in windows]
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    pp = i32(np.concatenate([[0], np.cumsum([len(x) for x in ps])]))
    ep = i32(np.concatenate([[0], np.cumsum([len(x) for x in es])]))
    pi = i32(np.concatenate(ps + [np.zeros(1, np.int64)]))   # (one spare entry: never an empty array)
    ei = i32(np.concatenate(es + [np.zeros(1, np.int64)]))
    an = i32([int(w[off + 2]) for w in windows] + [0])
    pr = i32([int(w[0]) for w in windows] + [0]) if with_problem else None
    return pr, pp, pi, ep, ei, an


def _window_solve(fn, h, windows, with_problem, max_iters, commit, want_records):
    n = len(windows)
    pr, pp, pi, ep, ei, an = _window_args(windows, with_problem)
    out = np.zeros((max(int(pp[-1]), 1), 3))
    res = (WindowResult * max(n, 1))()
    rows = max(int(max_iters), 0) + 1
    recs = (IterRecord * max(n * rows, 1))() if want_records else None
    head = (h, n, _ip(pr)) if with_problem else (h, n)
    _check(fn(*head, _ip(pp), _ip(pi), _ip(ep), _ip(ei), _ip(an), int(max_iters), int(bool(commit)), _dp(out), res, recs))
    poses = [out[pp[w]:pp[w + 1]].copy() for w in range(n)]
    results = [res[w] for w in range(n)]
    if not want_records:
        return poses, results
    return poses, results, [[recs[w * rows + k].as_dict() for k in range(results[w].n_records)] for w in range(n)]


def sample_noise_eval(seed, stream, index, sample):
    """pgo_sample_noise_eval (host only): the standard normal triple of (seed, stream 0 = edges | 1 = priors, index, sample)"""
    z = np.zeros(3)
    _check(lib().pgo_sample_noise_eval(int(seed), int(stream), int(index), int(sample), _dp(z)))
    return z


def gate_evaluate(r, P, info=None):
    """pgo_gate_evaluate (host only), the 3x3 algebra of Solver.gate: (chi2, chi2_marginal, info_gain) from the residual r,
    the covariance P (3x3) of the predicted residual and the information (I11 I12 I13 I22 I23 I33), None = the identity"""
    r = np.ascontiguousarray(r, np.float64).reshape(3)
    P = np.ascontiguousarray(P, np.float64).reshape(9)
    w = np.ascontiguousarray(info, np.float64).reshape(6) if info is not None else None
    out = np.zeros(3)
    _check(lib().pgo_gate_evaluate(_dp(r), _dp(P), _dp(w), _dp(out)))
    return float(out[0]), float(out[1]), float(out[2])


def _force_arg(force, n):
    if force is None:
        return None, None
    f = np.ascontiguousarray(np.asarray(force, np.int64).reshape(-1).clip(-128, 127), np.int8)
    if f.size != n:
        raise ValueError("force: one entry per candidate (-1 = the tests, 0 = reject, 1 = accept)")
    return f, f.ctypes.data_as(C.POINTER(C.c_int8))


def _joint_dict(res, n, summ):
    a = np.ctypeslib.as_array(res)[:n]
    out = {"r_cond": a["r_cond"].copy(), "P_cond": a["P_cond"].reshape(n, 3, 3).copy(), "chi2_cond": a["chi2_cond"].copy(),
           "info_gain_cond": a["info_gain_cond"].copy(), "accepted": a["accepted"].copy(), "status": a["status"].copy()}
    out.update(summ.as_dict())
    return out


def gate_joint_evaluate(r, P, info=None, status=None, force=None, chi2_gate=None, min_info_gain=None):
    """pgo_gate_joint_evaluate (host only), the elimination of Solver.gate_joint: candidates decided one after the other, in
    the given order, on r (n, 3) and their joint covariance P (3n, 3n), each accepted one conditioning the rest.  info =
    (n, 6) or None (the identity), status = (n) 0 / 1 or None, force = (n) in {-1, 0, 1} or None (-1: the two tests).
    Returns a dict: r_cond (n, 3), P_cond (n, 3, 3), chi2_cond, info_gain_cond, accepted, status (n), and the summary
    n_accepted, chi2_joint, info_gain_joint."""
    r = np.ascontiguousarray(r, np.float64).reshape(-1)
    n = r.size // 3
    P = np.ascontiguousarray(P, np.float64).reshape(-1)
    w = np.ascontiguousarray(info, np.float64).reshape(-1, 6) if info is not None else None
    st = np.ascontiguousarray(np.asarray(status, np.int64).reshape(-1), np.int32) if status is not None else None
    if r.size != 3 * n or P.size != 9 * n * n or (w is not None and w.shape[0] != n) or (st is not None and st.size != n):
        raise ValueError("gate_joint_evaluate: r (n, 3), P (3n, 3n), info (n, 6) and status (n) required")
    f, fp = _force_arg(force, n)
    o = GateJointOptions(chi2_gate=chi2_gate, min_info_gain=min_info_gain)
    res = (GateJointResult * max(n, 1))()
    summ = GateJointSummary()
    _check(lib().pgo_gate_joint_evaluate(n, _dp(r), _dp(P), _dp(w), _ip(st) if st is not None else None, fp, C.byref(o), res, C.byref(summ)))
    return _joint_dict(res, n, summ)


def set_knob(name: str, value: int = -1):
    """test hook (pgo_debug_set_knob): process-wide, read when a handle is created; value < 0 = library default"""
    _check(lib().pgo_debug_set_knob(name.encode(), int(value)))


def pose_order(n_poses, ia, ib, segment=64):
    """perm[i] = internal position of pose i under the locality ordering (pgo_pose_order)"""
    ia = np.ascontiguousarray(ia, np.int32)
    ib = np.ascontiguousarray(ib, np.int32)
    perm = np.zeros(n_poses, np.int32)
    _check(lib().pgo_pose_order(n_poses, len(ia), _ip(ia), _ip(ib), segment, _ip(perm)))
    return perm


def shard_halo(n_poses, ia, ib, world, rank, row_align=1):
    """(send_rows[world], recv_rows[world]) of the point-to-point halo exchange plan"""
    ia = np.ascontiguousarray(ia, np.int32)
    ib = np.ascontiguousarray(ib, np.int32)
    snd, rcv = np.zeros(world, np.int64), np.zeros(world, np.int64)
    _check(lib().pgo_shard_halo(n_poses, len(ia), _ip(ia), _ip(ib), world, rank, row_align,
                                snd.ctypes.data_as(C.POINTER(C.c_int64)), rcv.ctypes.data_as(C.POINTER(C.c_int64))))
    return snd, rcv


class Comm:
    """One process per GPU.  kind='rccl' (production) or 'shm' (test backend, several ranks per GPU)."""

    def __init__(self, handle, rank, world):
        self._h, self.rank, self.world = handle, rank, world

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        _check(lib().pgo_comm_unique_id(buf))
        return bytes(buf)

    @classmethod
    def rccl(cls, uid: bytes, rank: int, world: int, device: int) -> "Comm":
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        h = C.c_void_p()
        _check(lib().pgo_comm_create_rccl(buf, rank, world, device, C.byref(h)))
        return cls(h, rank, world)

    @classmethod
    def shm(cls, name: str, rank: int, world: int, device: int = 0) -> "Comm":
        h = C.c_void_p()
        _check(lib().pgo_comm_create_shm(name.encode(), rank, world, device, C.byref(h)))
        return cls(h, rank, world)

    def close(self):
        if self._h:
            lib().pgo_comm_destroy(self._h)
            self._h = None


def solve_batch(solvers, max_concurrency: int = 8):
    """pgo_solve_batch: solve every Solver in the list (independent problems) concurrently; returns their summaries"""
    n = len(solvers)
    hs = (C.c_void_p * max(n, 1))(*[s._h for s in solvers])
    out = (Summary * max(n, 1))()
    _check(lib().pgo_solve_batch(hs, n, out, max_concurrency))
    return [out[i] for i in range(n)]


class Batch:
    """pgo_batch_*: ONE handle over the block-diagonal union of independent problems (the layer managers' many small
    ceres::Solve calls, reference src/simple_layer_manager.cpp:457-622); per-problem LM state, one workgroup per problem
    for the linear solves."""

    def __init__(self, graphs, options: "Options | None" = None, device: int = 0, losses=None, edge_class=None):
        self.graphs = list(graphs)
        self.options = options if options is not None else Options()
        n = len(self.graphs)
        hs = (C.c_void_p * max(n, 1))(*[g._h for g in self.graphs])
        self._h = C.c_void_p()
        _check(lib().pgo_batch_create(C.byref(self._h), n, hs, C.byref(self.options), device))
        self.n = n
        if losses is not None:
            self.set_losses(losses, edge_class)

    def set_losses(self, losses, edge_class=None):
        """pgo_batch_set_losses: losses = a Loss or a list of 1-4 (classes); edge_class over the problems' edges
        concatenated, or None (class = min(kind, n_classes - 1))"""
        n, arr, cls, keep = _loss_args(losses, edge_class, sum(g.n_edges for g in self.graphs))
        _check(lib().pgo_batch_set_losses(self._h, n, arr, cls))

    def set_active(self, edge_active=None, pose_constant=None):
        """pgo_batch_set_active: which edges / constant poses every problem has from now on.  Each argument: None, the
        concatenated mask over all problems, or a list with one mask (or None = all edges / no pose) per problem."""
        def cat(m, sizes, what):
            if m is None:
                return None
            if isinstance(m, (list, tuple)) and len(m) == self.n and any(x is None or np.ndim(x) > 0 for x in m):
                fill = 1 if what == "edge_active" else 0
                m = np.concatenate([np.full(k, fill, np.uint8) if x is None else _mask(x, k, what) for x, k in zip(m, sizes)])
            return _mask(m, sum(sizes), what)
        ea = cat(edge_active, [g.n_edges for g in self.graphs], "edge_active")
        pc = cat(pose_constant, [g.n_poses for g in self.graphs], "pose_constant")
        _check(lib().pgo_batch_set_active(self._h, _bp(ea) if ea is not None else None, _bp(pc) if pc is not None else None))

    def window_solve(self, windows, max_iters=2, commit=False, want_records=False):
        """pgo_batch_window_solve: windows = a list of (problem, pose_idx, edge_idx, anchor), indices in that problem's own
        numbering; otherwise Solver.window_solve"""
        return _window_solve(lib().pgo_batch_window_solve, self._h, windows, True, max_iters, commit, want_records)

    def close(self):
        if getattr(self, "_h", None):
            lib().pgo_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve(self):
        out = (Summary * max(self.n, 1))()
        _check(lib().pgo_batch_solve(self._h, out))
        return [out[i] for i in range(self.n)]

    def poses(self, k: int):
        out = np.zeros((self.graphs[k].n_poses, 3))
        _check(lib().pgo_batch_get_poses(self._h, k, _dp(out)))
        return out

    def set_poses(self, k: int, poses):
        p = np.ascontiguousarray(poses, np.float64)
        _check(lib().pgo_batch_set_poses(self._h, k, _dp(p)))

    def debug_solve(self, radius, max_it, rtol, rhs=None):
        """pgo_batch_debug_solve: the one-workgroup PCG solve of every problem at the current poses.  rhs: None (the scaled
        gradient), the concatenated right-hand side, or a list with one array of 3 n_k per problem.
        Returns (list of y arrays per problem, list of result dicts)."""
        sizes = [3 * g.n_poses for g in self.graphs]
        b = None
        if rhs is not None:
            if isinstance(rhs, (list, tuple)):
                rhs = np.concatenate([np.asarray(v, np.float64).reshape(-1) for v in rhs])
            b = np.ascontiguousarray(rhs, np.float64).reshape(-1)
            if b.size != sum(sizes):
                raise ValueError("rhs: 3 n_k doubles per problem")
        y = np.zeros(sum(sizes))
        res = (SoloResult * max(self.n, 1))()
        _check(lib().pgo_batch_debug_solve(self._h, float(radius), int(max_it), float(rtol), _dp(b) if b is not None else None,
                                           _dp(y), res))
        return np.split(y, np.cumsum(sizes)[:-1]), [res[i].as_dict() for i in range(self.n)]

    def iter_records(self, k: int):
        n = lib().pgo_batch_num_iter_records(self._h, k)
        arr = (IterRecord * max(n, 1))()
        _check(lib().pgo_batch_get_iter_records(self._h, k, arr, n))
        return [arr[i].as_dict() for i in range(n)]


class Solver:
    """Problem assembly + ceres::Solve replacement (reference main.cpp:66-163)."""

    def __init__(self, graph: Graph, options: Options | None = None, comm: Comm | None = None, device: int = 0,
                 losses=None, edge_class=None):
        self.graph = graph
        self.options = options if options is not None else Options()
        self.comm = comm
        self._h = C.c_void_p()
        _check(lib().pgo_create_from_graph(C.byref(self._h), graph._h, C.byref(self.options),
                                           comm._h if comm else None, device))
        self.n_poses, self.n_edges = graph.n_poses, graph.n_edges
        self._n_mix = 0   # the mixture edges in force (set_mixtures, set_mixture_null): the size of the per-mixture outputs
        if losses is not None:
            self.set_losses(losses, edge_class)

    def set_losses(self, losses, edge_class=None):
        """pgo_set_losses: losses = a Loss or a list of 1-4 (the loss classes); edge_class = each edge's class, or None
        (class = min(kind, n_classes - 1): one loss for all, odometry / loops, or by edge kind).  A solve begun with
        lm_begin is stale afterwards."""
        n, arr, cls, keep = _loss_args(losses, edge_class, self.n_edges)
        _check(lib().pgo_set_losses(self._h, n, arr, cls))

    def set_active(self, edge_active=None, pose_constant=None):
        """pgo_set_active: edge_active = a mask over the edges (truthy = a residual block; None = all), pose_constant = a
        mask over the poses (truthy = SetParameterBlockConstant; None = none).  Poses without an active edge are constant
        too.  set_active() restores the handle.  A solve begun with lm_begin is stale afterwards."""
        ea = _mask(edge_active, self.n_edges, "edge_active")
        pc = _mask(pose_constant, self.n_poses, "pose_constant")
        _check(lib().pgo_set_active(self._h, _bp(ea) if ea is not None else None, _bp(pc) if pc is not None else None))

    def close(self):
        if getattr(self, "_h", None):
            lib().pgo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def evaluate(self, poses=None, apply_loss=True, want_r=True, want_J=True):
        p = np.ascontiguousarray(poses, np.float64) if poses is not None else None
        r = np.zeros((self.n_edges, 3)) if want_r else None
        J = np.zeros((self.n_edges, 18)) if want_J else None
        cost = C.c_double()
        _check(lib().pgo_eval(self._h, _dp(p), int(apply_loss), C.byref(cost), _dp(r), _dp(J)))
        return cost.value, r, J

    def edge_chi2(self, poses=None):
        """r' Omega r of the plain residual per edge (compute_edge_mahalanobis, src/layer_manager.cpp:230-282)"""
        p = np.ascontiguousarray(poses, np.float64) if poses is not None else None
        out = np.zeros(self.n_edges)
        _check(lib().pgo_edge_chi2(self._h, _dp(p), _dp(out)))
        return out

    def solve(self) -> Summary:
        s = Summary()
        _check(lib().pgo_solve(self._h, C.byref(s)))
        return s

    def trajectory_error(self, ref, mask=None, align=False, rpe_delta=1, per_pose=False):
        """pgo_trajectory_error: the handle's current poses scored against the (N, 3) reference on the device; arguments and
        result as trajectory_error.  The handle is left as it was (it may run between lm_step slices)."""
        return _traj_call(lib().pgo_trajectory_error, (self._h,), self.n_poses, ref, mask, align, rpe_delta, per_pose)

    def edge_weights(self, poses=None):
        """pgo_edge_weights (METHOD 0 / 1): what DCS and the loss did to each edge at the current poses (or at `poses`) -- a
        structured array over the edges with the fields of EdgeWeight: s_plain, scale, rho1, weight, cost, active"""
        p = np.ascontiguousarray(poses, np.float64) if poses is not None else None
        if p is not None and p.size != 3 * self.n_poses:
            raise ValueError("edge_weights: poses must be (n_poses, 3)")
        res = (EdgeWeight * max(self.n_edges, 1))()
        _check(lib().pgo_edge_weights(self._h, _dp(p), res))
        return np.ctypeslib.as_array(res)[:self.n_edges].copy()

    def set_edge_weights(self, w=None):
        """pgo_set_edge_weights: a weight in [0, 1] per edge (caller's order) -- the edge counts w 1/2 rho(s), its rows are
        scaled by sqrt(w rho'(s)); None drops the plane and restores the handle.  A solve begun with lm_begin is stale
        afterwards."""
        if w is None:
            _check(lib().pgo_set_edge_weights(self._h, None))
            return
        a = np.ascontiguousarray(w, np.float64).reshape(-1)
        if a.size != self.n_edges:
            raise ValueError(f"set_edge_weights: {a.size} entries for {self.n_edges} edges")
        _check(lib().pgo_set_edge_weights(self._h, _dp(a)))

    def set_priors(self, poses, means, info, loss=None):
        """pgo_set_priors: absolute pose priors -- poses = the pose of each prior (at most one per pose), means (n, 3) = its
        (x, y, theta), info = (n, 6) rows I11 I12 I13 I22 I23 I33 or (n, 3, 3) symmetric positive SEMI-definite matrices
        (diag(a, a, 0) is a position-only fix), loss = ONE Loss for all priors (None: Trivial).  Each call replaces the whole
        set; no priors (or clear_priors) restores the handle.  A solve begun with lm_begin is stale afterwards."""
        idx = np.ascontiguousarray(poses, np.int32).reshape(-1)
        n = idx.size
        if n == 0:
            return self.clear_priors()
        z = np.ascontiguousarray(means, np.float64)
        if z.size != 3 * n:
            raise ValueError(f"set_priors: means must be ({n}, 3)")
        w = _info6(info, n)
        _check(lib().pgo_set_priors(self._h, n, _ip(idx), _dp(z), _dp(w), C.byref(loss) if loss is not None else None))

    def clear_priors(self):
        """pgo_set_priors(h, 0, ...): no priors -- a solve afterwards gives bitwise what a fresh handle gives"""
        _check(lib().pgo_set_priors(self._h, 0, None, None, None, None))

    @property
    def n_priors(self):
        return int(lib().pgo_num_priors(self._h))

    def prior_residuals(self, poses=None):
        """pgo_get_prior_residuals: (d (n, 3), chi2 (n,)) of the priors' plain residual at the current poses (or at `poses`),
        in the order the priors were given; computed on the device"""
        p = np.ascontiguousarray(poses, np.float64) if poses is not None else None
        if p is not None and p.size != 3 * self.n_poses:
            raise ValueError("prior_residuals: poses must be (n_poses, 3)")
        n = self.n_priors
        d, chi2 = np.zeros((n, 3)), np.zeros(n)
        _check(lib().pgo_get_prior_residuals(self._h, _dp(p), _dp(d), _dp(chi2)))
        return d, chi2

    def get_edge_weights(self):
        """pgo_get_edge_weights: the plane in the caller's edge order (all ones when none is set)"""
        out = np.zeros(self.n_edges)
        _check(lib().pgo_get_edge_weights(self._h, _dp(out)))
        return out

    def gnc_update(self, cbar, mu, select=None):
        """pgo_gnc_update at the current poses: the selected edges (default: the active edges with kind != 0; else a mask over
        the edges) get the GNC-TLS weight for (cbar, mu); mu <= 0 measures only.  Returns the dict of GncStats."""
        m = _mask(select, self.n_edges, "select")
        st = GncStats()
        _check(lib().pgo_gnc_update(self._h, float(cbar), float(mu), _bp(m) if m is not None else None, C.byref(st)))
        return st.as_dict()

    def gnc_solve(self, cbar, select=None, **opts):
        """pgo_gnc_solve (METHOD 0): graduated non-convexity with the TLS surrogate from the current poses; opts: mu_factor,
        inner_iters, final_iters, max_rounds.  Returns (summary dict, list of round dicts); the weights stay on the handle
        (get_edge_weights)."""
        o = GncOptions(cbar, **opts)
        m = _mask(select, self.n_edges, "select")
        if m is not None:
            o.select = _bp(m)
        cap = max(int(o.max_rounds), 1)
        rounds = (GncRound * cap)()
        summ = GncSummary()
        _check(lib().pgo_gnc_solve(self._h, C.byref(o), C.byref(summ), rounds, cap))
        return summ.as_dict(), [rounds[k].as_dict() for k in range(min(summ.rounds, cap))]

    def set_mixtures(self, edge=None, comp_ptr=None, comps=None):
        """pgo_set_mixtures (METHOD 0): the max-mixture edges of the handle -- edge: strictly ascending edge indices (caller's
        order), comp_ptr: CSR offsets, comps: (n_comp, 5) rows (x, y, theta, weight, info_scale), 1 to 8 per edge.  No plane
        is touched until mixture_select(apply=True).  set_mixtures() clears: the measurements are restored, the former
        mixture edges' weights become 1."""
        if edge is None:
            _check(lib().pgo_set_mixtures(self._h, 0, None, None, None))
            self._n_mix = 0
            return
        edge, comp_ptr, comps = _mix_table(edge, comp_ptr, comps)
        _check(lib().pgo_set_mixtures(self._h, edge.size, _ip(edge), _ip(comp_ptr), _dp(comps)))
        self._n_mix = int(edge.size)

    def set_mixture_null(self, pi_null, scale_null, select=None):
        """pgo_set_mixture_null: every selected edge (default: the active edges with kind != 0; else a mask over the edges)
        gets an inlier component (pi = 1, w = 1) and a null hypothesis (pi_null, scale_null) at its own measurement"""
        m = _mask(select, self.n_edges, "select")
        _check(lib().pgo_set_mixture_null(self._h, _bp(m) if m is not None else None, float(pi_null), float(scale_null)))
        st = MixStats()   # (the library resolved the selection: one measuring select, once per table, tells how many edges it took)
        _check(lib().pgo_mixture_select(self._h, 0, C.byref(st), None, None))
        self._n_mix = int(st.n_mix)

    def mixture_selection(self):
        """pgo_get_mixture_selection: the last applied component per mixture edge, -1 where none"""
        out = np.zeros(max(self._n_mix, 1), np.int32)
        _check(lib().pgo_get_mixture_selection(self._h, _ip(out)))
        return out[:self._n_mix]

    def mixture_select(self, apply=False):
        """pgo_mixture_select at the current poses: per mixture edge the component with the smallest q; apply=True writes its
        mean into the measurement planes and its info_scale into the edge weight plane.  Returns (chosen, q (n_mix, 2) =
        q_best and margin, stats dict)."""
        n = self._n_mix
        chosen, q, st = np.zeros(max(n, 1), np.int32), np.zeros((max(n, 1), 2)), MixStats()
        _check(lib().pgo_mixture_select(self._h, int(bool(apply)), C.byref(st), _ip(chosen), _dp(q)))
        return chosen[:n], q[:n], st.as_dict()

    def mixture_solve(self, **opts):
        """pgo_mixture_solve (METHOD 0): rounds of select + apply and a short LM solve from the current poses until the
        selection stands, then a final solve; opts: inner_iters, final_iters, max_rounds.  Returns (summary dict, list of round
        dicts); the selection stays on the handle (mixture_selection, get_edge_weights)."""
        o = MixtureOptions(**opts)
        cap = max(int(o.max_rounds), 1)
        rounds = (MixtureRound * cap)()
        summ = MixtureSummary()
        _check(lib().pgo_mixture_solve(self._h, C.byref(o), C.byref(summ), rounds, cap))
        return summ.as_dict(), [rounds[k].as_dict() for k in range(min(summ.rounds, cap))]

    def loop_support(self, select=None, window=32, tol_xy=0.1, tol_th=0.05, min_support=1, apply=False):
        """pgo_loop_support: loop_support_plan on the measurements the handle holds on the device; the estimate plays no part.
        apply=True writes the verdict into the edge weight plane (METHOD 0 / 1): every selected edge gets 1 if it has at least
        min_support consistent neighbours, else 0; every other edge keeps its weight.  Returns (records, stats)."""
        m = _mask(select, self.n_edges, "select")
        o = LoopSupportOptions(window=int(window), tol_xy=float(tol_xy), tol_th=float(tol_th), min_support=int(min_support),
                               apply=int(bool(apply)))
        res = (LoopSupportRecord * max(self.n_edges, 1))()
        st = LoopSupportStats()
        _check(lib().pgo_loop_support(self._h, C.byref(o), _bp(m) if m is not None else None, res, C.byref(st)))
        return _support_records(res, self.n_edges), st.as_dict()

    def chordal_init(self, commit=False, apply_weights=False, **opts):
        """pgo_chordal_init: chordal_plan on the measurements the handle holds on the device, with the handle's weight plane,
        active set and constant poses; the estimate plays no part except on the constant poses.  commit=True writes the result
        as the handle's poses (constant poses are not moved; a solve begun with lm_begin is stale); apply_weights=True writes 0
        into the weight plane on the edges the reject rounds (rounds, reject_xy, reject_th) dropped (METHOD 0 / 1).
        Returns (poses (N, 3), res (E, 2), summary dict)."""
        o = ChordalOptions(commit=int(bool(commit)), apply_weights=int(bool(apply_weights)), **opts)
        out, res = np.zeros((max(self.n_poses, 1), 3)), np.zeros((max(self.n_edges, 1), 2))
        summ = ChordalSummary()
        _check(lib().pgo_chordal_init(self._h, C.byref(o), _dp(out), _dp(res), C.byref(summ)))
        return out[:self.n_poses], res[:self.n_edges], summ.as_dict()

    def coarsen(self, stride: int, information: bool = False):
        """pgo_coarsen: the coarse graph of the handle's measurements at `stride` (see coarsen_plan), with the handle's current
        poses at the key poses as its initial poses.  Returns (Graph, origin): origin[e] = the fine edge behind coarse edge e,
        -1 for a composite of the odometry chain.  The handle keeps the composites of this stride for prolong and is
        otherwise left as it was.  information=True: pgo_coarsen_info -- the information matrices carried through the
        composition (coarsen_info_plan); returns (Graph, origin, cov) with cov (n, 6) the coarse edges' covariances, the
        graph carrying their inverses."""
        g = C.c_void_p()
        origin = np.zeros(max(self.n_edges, 1), np.int32)   # (a coarse graph never has more edges than the fine one)
        n = C.c_int32(-1)
        if information:
            cov = np.zeros((max(self.n_edges, 1), 6))
            _check(lib().pgo_coarsen_info(self._h, int(stride), C.byref(g), _ip(origin), _dp(cov), self.n_edges, C.byref(n)))
            return Graph(g), origin[:n.value].copy(), cov[:n.value].copy()
        _check(lib().pgo_coarsen(self._h, int(stride), C.byref(g), _ip(origin), self.n_edges, C.byref(n)))
        return Graph(g), origin[:n.value].copy()

    def prolong(self, stride: int, coarse_poses):
        """pgo_prolong: the coarse poses (K, 3) spread over the handle's poses on the device along the composites that
        coarsen(stride) left; constant poses are not moved.  A solve begun with lm_begin is stale afterwards."""
        X = np.ascontiguousarray(coarse_poses, np.float64).reshape(-1, 3)
        s = int(stride)
        if s >= 1 and len(X) != (self.n_poses + s - 1) // s:
            raise ValueError(f"prolong: {len(X)} coarse poses, expected {(self.n_poses + s - 1) // s}")
        _check(lib().pgo_prolong(self._h, s, _dp(X)))

    def initialize_hierarchical(self, stride: int, coarse_options: "Options | None" = None, device: int = 0,
                                carry_weights: bool = False, information: bool = False) -> Summary:
        """coarsen -> a solver on the coarse graph -> solve -> prolong: the handle's poses start the fine solve near the answer
        of the coarse one.  coarse_options (default: the handle's method, pcg_rtol 1e-10 -- the exact mode --, everything else
        left to the library; a fixed pose that is a key pose stays the fixed pose).  carry_weights: every coarse edge takes the
        weight its fine edge has in the handle's weight plane (after loop_support(apply=True): the coarse solve runs without
        the dropped loops); the composites of the chain have weight 1.  information=True: the coarse graph carries the
        propagated information matrices (coarsen(stride, information=True)) and the default coarse options set
        info_weighting = 1, so the coarse objective is the fine one's; a robust kernel's scale (phi of METHOD 1) then acts on
        chi2 and is the caller's to set through coarse_options.  The weight plane refuses info_weighting = 1, so carried
        weights must be 0 or 1 (ValueError otherwise) and are passed as set_active(edge_active=...).  Returns the coarse
        solve's Summary."""
        s = int(stride)
        graph, origin = self.coarsen(s, information=True)[:2] if information else self.coarsen(s)
        if coarse_options is None:
            f = int(self.options.fixed_pose)
            coarse_options = Options(method=int(self.options.method), pcg_rtol=1e-10,
                                     fixed_pose=(f if f < 0 else (f // s if f % s == 0 else 0)),
                                     info_weighting=1 if information else 0)
        w = None
        if carry_weights:
            w = self.get_edge_weights()
            w = np.where(origin >= 0, w[np.maximum(origin, 0)], 1.0)
            if information and not np.isin(w, (0.0, 1.0)).all():
                raise ValueError("initialize_hierarchical: information=True carries weights 0 and 1 only")
        coarse = Solver(graph, coarse_options, device=device)
        try:
            if w is not None and information:
                coarse.set_active(edge_active=w != 0.0)
            elif w is not None:
                coarse.set_edge_weights(w)
            summary = coarse.solve()
            self.prolong(s, coarse.poses())
        finally:
            coarse.close()
        return summary

    def lm_begin(self):
        _check(lib().pgo_lm_begin(self._h))

    def lm_step(self, n_iters: int = 1):
        s, done = Summary(), C.c_int32()
        _check(lib().pgo_lm_step(self._h, n_iters, C.byref(done), C.byref(s)))
        return bool(done.value), s

    def iter_records(self):
        n = lib().pgo_num_iter_records(self._h)
        arr = (IterRecord * max(n, 1))()
        _check(lib().pgo_get_iter_records(self._h, arr, n))
        return [arr[i].as_dict() for i in range(n)]

    def info(self) -> HandleInfo:
        """what the handle resolved its auto options to (pgo_get_info)"""
        out = HandleInfo()
        _check(lib().pgo_get_info(self._h, C.byref(out)))
        return out

    def poses(self):
        out = np.zeros((self.n_poses, 3))
        _check(lib().pgo_get_poses(self._h, _dp(out)))
        return out

    def switches(self, want_js=False):
        sw = np.ones(self.n_edges)
        js = np.zeros((self.n_edges, 3)) if want_js else None
        _check(lib().pgo_get_switches(self._h, _dp(sw), _dp(js)))
        return (sw, js) if want_js else sw

    def set_poses(self, poses):
        p = np.ascontiguousarray(poses, np.float64)
        _check(lib().pgo_set_poses(self._h, _dp(p)))

    def covariance(self, poses, cross=False, **opts):
        """ceres::Covariance at the current poses (pgo_pose_covariance): poses = indices in the caller's numbering.
        Returns ((n, 3, 3) diagonal blocks, or the (3n, 3n) matrix with cross=True), report dict)."""
        idx = np.ascontiguousarray(np.asarray(poses, np.int64).reshape(-1), np.int32)
        n = idx.size
        o = CovarianceOptions(cross=int(bool(cross)), **opts)
        out = np.zeros((3 * n, 3 * n) if cross else (n, 3, 3))
        rep = CovarianceReport()
        _check(lib().pgo_pose_covariance(self._h, n, _ip(idx), C.byref(o), _dp(out), C.byref(rep)))
        return out, rep.as_dict()

    def sample(self, n, seed=0, first=0, want_deltas=True, want_cov=True, **opts):
        """pgo_posterior_sample: n draws delta ~ N(0, (J'J)^-1) around the current poses (samples first .. first + n - 1 of the
        seed's stream) and their second moment per pose.  Returns (deltas (n, N, 3) or None, cov (N, 3, 3) or None, report
        dict); opts: the other SampleOptions fields (rtol, max_iters, samples_per_pass, solver)."""
        o = SampleOptions(seed=int(seed), first_sample=int(first), **opts)
        n = int(n)
        deltas = np.zeros((max(n, 0), self.n_poses, 3)) if want_deltas else None
        cov = np.zeros((self.n_poses, 3, 3)) if want_cov else None
        rep = CovarianceReport()
        _check(lib().pgo_posterior_sample(self._h, n, C.byref(o), _dp(deltas), _dp(cov), C.byref(rep)))
        return deltas, cov, rep.as_dict()

    def debug_sample_rhs(self, seed, sample):
        """pgo_debug_sample_rhs: (eps (E, 3) in the caller's edge order, b (N, 3) = J' eps (+ R eps_p), unscaled, 0 on the
        constant poses) of one sample"""
        eps, b = np.zeros((self.n_edges, 3)), np.zeros((self.n_poses, 3))
        _check(lib().pgo_debug_sample_rhs(self._h, int(seed), int(sample), _dp(eps), _dp(b)))
        return eps, b

    @staticmethod
    def _gate_args(ia, ib, meas, info):
        ia = np.ascontiguousarray(np.asarray(ia, np.int64).reshape(-1), np.int32)
        ib = np.ascontiguousarray(np.asarray(ib, np.int64).reshape(-1), np.int32)
        n = ia.size
        meas = np.ascontiguousarray(meas, np.float64).reshape(-1, 3)
        w = np.ascontiguousarray(info, np.float64).reshape(-1, 6) if info is not None else None
        if ib.size != n or meas.shape[0] != n or (w is not None and w.shape[0] != n):
            raise ValueError("gate: ia, ib, meas and info must have one entry per candidate")
        return n, ia, ib, meas, w

    @staticmethod
    def _gate_dict(res, n):
        a = np.ctypeslib.as_array(res)[:n]
        return {"r": a["r"].copy(), "J": a["J"].reshape(n, 3, 6).copy(), "P": a["P"].reshape(n, 3, 3).copy(),
                "chi2": a["chi2"].copy(), "chi2_marginal": a["chi2_marginal"].copy(), "info_gain": a["info_gain"].copy(),
                "status": a["status"].copy()}

    def gate(self, ia, ib, meas, info=None, **opts):
        """pgo_edge_gate: candidate loop edges (ia[k], ib[k], meas[k], info[k]) against the current estimate -- they need
        not be edges of the graph.  info = (n, 6) information entries or None (the identity).  Returns (dict of arrays
        r (n, 3), J (n, 3, 6), P (n, 3, 3), chi2, chi2_marginal, info_gain, status (n), report dict); opts: the
        CovarianceOptions fields (poses_per_pass = candidates per pass)."""
        n, ia, ib, meas, w = self._gate_args(ia, ib, meas, info)
        o = CovarianceOptions(**opts)
        res = (EdgeGateResult * max(n, 1))()
        rep = CovarianceReport()
        _check(lib().pgo_edge_gate(self._h, n, _ip(ia), _ip(ib), _dp(meas), _dp(w), C.byref(o), res, C.byref(rep)))
        return self._gate_dict(res, n), rep.as_dict()

    def gate_joint(self, ia, ib, meas, info=None, force=None, chi2_gate=None, min_info_gain=None, full=False, **cov_opts):
        """pgo_edge_gate_joint: the candidates of Solver.gate judged ONE AFTER THE OTHER, in the given order, every accepted one
        conditioning those after it (at most GATE_JOINT_MAX per call).  force = (n) in {-1, 0, 1} or None: -1 applies
        chi2_cond <= chi2_gate and info_gain_cond >= min_info_gain, 0 rejects, 1 accepts.  Returns (out, joint, report): out
        as Solver.gate returns it (bitwise), joint the dict of gate_joint_evaluate -- plus "P_full" (3n, 3n), the joint
        covariance of the predicted residuals, with full=True; cov_opts: the CovarianceOptions fields."""
        n, ia, ib, meas, w = self._gate_args(ia, ib, meas, info)
        f, fp = _force_arg(force, n)
        jo = GateJointOptions(chi2_gate=chi2_gate, min_info_gain=min_info_gain)
        o = CovarianceOptions(**cov_opts)
        res = (EdgeGateResult * max(n, 1))()
        jres = (GateJointResult * max(n, 1))()
        summ, rep = GateJointSummary(), CovarianceReport()
        P_full = np.zeros((3 * n, 3 * n)) if full else None
        _check(lib().pgo_edge_gate_joint(self._h, n, _ip(ia), _ip(ib), _dp(meas), _dp(w), fp, C.byref(jo), C.byref(o), res, jres,
                                         _dp(P_full), C.byref(summ), C.byref(rep)))
        joint = _joint_dict(jres, n, summ)
        if full:
            joint["P_full"] = P_full
        return self._gate_dict(res, n), joint, rep.as_dict()

    def window_solve(self, windows, max_iters=2, commit=False, want_records=False):
        """pgo_window_solve: many small windows of the graph in one kernel launch, one workgroup per window (the layer
        managers' optimize_local_window).  windows = a list of (pose_idx, edge_idx, anchor) -- what window_plan returns --
        of at most WINDOW_MAX_POSES poses and WINDOW_MAX_EDGES edges each; every window starts from the handle's current poses.
        Returns (list of (n_w, 3) final poses in list order, list of WindowResult[, list of iteration-record dicts per window]).
        commit=True also writes the poses into the handle (the lists must be disjoint)."""
        return _window_solve(lib().pgo_window_solve, self._h, windows, False, max_iters, commit, want_records)

    def write_back(self):
        """poses are optimised IN PLACE in Node::p in the reference (main.cpp:99,163)"""
        self.graph.poses[:] = self.poses()

    # ---- kernel-level entry points
    def normal_eq(self):
        g, hd = np.zeros(3 * self.n_poses), np.zeros((self.n_poses, 9))
        _check(lib().pgo_debug_normal_eq(self._h, _dp(g), _dp(hd)))
        return g, hd

    def spmv(self, x):
        x = np.ascontiguousarray(x, np.float64)
        y = np.zeros_like(x)
        _check(lib().pgo_debug_spmv(self._h, _dp(x), _dp(y)))
        return y

    def bench_eval(self, reps=10, with_jacobian=True) -> KernelStats:
        k = KernelStats()
        _check(lib().pgo_bench_eval(self._h, reps, int(with_jacobian), C.byref(k)))
        return k

    def bench_assemble(self, reps=10) -> KernelStats:
        k = KernelStats()
        _check(lib().pgo_bench_assemble(self._h, reps, C.byref(k)))
        return k

    def bench_spmv(self, reps=10) -> KernelStats:
        k = KernelStats()
        _check(lib().pgo_bench_spmv(self._h, reps, C.byref(k)))
        return k

    def system_spmv(self, x, want_d2=False):
        """y = (H + D'D) x through the PCG loop's product kernel, LM diagonal for the current radius (and D'D's diagonal)"""
        x = np.ascontiguousarray(x, np.float64)
        y = np.zeros_like(x)
        d2 = np.zeros_like(x) if want_d2 else None
        _check(lib().pgo_debug_system_spmv(self._h, _dp(x), _dp(y), _dp(d2)))
        return (y, d2) if want_d2 else y

    def direct_solve(self, b, refine=-1):
        """y = (H + D'D)^-1 b by the direct chain + low-rank solve at the current LM state (pgo_debug_direct_solve): refine
        = -1 the handle's own refinement steps, 0 the raw Woodbury result, 1..3 that many"""
        b = np.ascontiguousarray(b, np.float64)
        y = np.zeros_like(b)
        _check(lib().pgo_debug_direct_solve(self._h, _dp(b), int(refine), _dp(y)))
        return y

    def precond(self, r):
        """z = M^-1 r with the preconditioner the next LM iteration applies (debug / restatement tests)"""
        r = np.ascontiguousarray(r, np.float64)
        z = np.zeros_like(r)
        _check(lib().pgo_debug_precond(self._h, _dp(r), _dp(z)))
        return z

    def bench_precond(self, reps=10) -> KernelStats:
        k = KernelStats()
        _check(lib().pgo_bench_precond(self._h, reps, C.byref(k)))
        return k
